/* p?trmr2d through a real BLACS (MKL BLACS over MPICH), one process.
 *
 *   trmr2d_check map    MKL's p{s,d,c,z}trmr2d_ alone (no GPU): for m x n in {5x3, 3x5, 4x4}, every
 *                       (uplo, diag), sub(A) at (2, 3) and sub(B) at (3, 2): one line
 *                       "<type> <uplo> <diag> <m> <n> <m*n flags, row-major: 1 = element written>",
 *                       after checking that written elements hold A's value and that nothing
 *                       outside sub(B) changed ("BAD ..." otherwise).  The test compares the flags
 *                       with the mapping include/costa/scalapack.h states.
 *   trmr2d_check gpu    (built with -DWITH_COSTA) costa_p?trmr2d against MKL's p?trmr2d_ on the
 *                       same inputs: 70x45, 45x70 and 64x64, source blocks 16x24, destination
 *                       blocks 20x12, ia = 3, jb = 2, every (uplo, diag) and type; the whole local
 *                       B is compared bit for bit.
 */
#include <mpi.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void Cblacs_pinfo(int*, int*);
void Cblacs_get(int, int, int*);
void Cblacs_gridinit(int*, char*, int, int);
void Cblacs_gridexit(int);
void descinit_(int*, const int*, const int*, const int*, const int*, const int*, const int*,
               const int*, const int*, int*);

#define TRMR2D_ARGS                                                                          \
    const char *uplo, const char *diag, const int *m, const int *n, const void *a,           \
        const int *ia, const int *ja, const int *desca, void *b, const int *ib, const int *jb, \
        const int *descb, const int *ictxt
typedef void (*trmr2d_fn)(TRMR2D_ARGS);
void pstrmr2d_(TRMR2D_ARGS);
void pdtrmr2d_(TRMR2D_ARGS);
void pctrmr2d_(TRMR2D_ARGS);
void pztrmr2d_(TRMR2D_ARGS);
#ifdef WITH_COSTA
void costa_pstrmr2d(TRMR2D_ARGS);
void costa_pdtrmr2d(TRMR2D_ARGS);
void costa_pctrmr2d(TRMR2D_ARGS);
void costa_pztrmr2d(TRMR2D_ARGS);
#endif

static const char TYPES[4] = {'s', 'd', 'c', 'z'};
static const int REALS[4] = {1, 1, 2, 2};     /* reals per element */
static const int RSIZE[4] = {4, 8, 4, 8};     /* bytes per real */
static trmr2d_fn MKL[4] = {pstrmr2d_, pdtrmr2d_, pctrmr2d_, pztrmr2d_};

/* real r of element k of a buffer of type t */
static void put(void* buf, int t, size_t k, int r, double v) {
    if (RSIZE[t] == 4) ((float*)buf)[k * REALS[t] + r] = (float)v;
    else ((double*)buf)[k * REALS[t] + r] = v;
}
static double get(const void* buf, int t, size_t k, int r) {
    return RSIZE[t] == 4 ? ((const float*)buf)[k * REALS[t] + r] : ((const double*)buf)[k * REALS[t] + r];
}

static void desc_of(int* desc, int M, int N, int mb, int nb, int ctxt) {
    int z = 0, info = 0, lld = M;
    descinit_(desc, &M, &N, &mb, &nb, &z, &z, &ctxt, &lld, &info);
}

static void fill(void* a, void* b, int t, int AM, int AN, int BM, int BN) {
    for (size_t k = 0; k < (size_t)AM * AN; ++k)
        for (int r = 0; r < REALS[t]; ++r) put(a, t, k, r, 1.0 + (double)k * 2 + r);
    for (size_t k = 0; k < (size_t)BM * BN; ++k)
        for (int r = 0; r < REALS[t]; ++r) put(b, t, k, r, -777.0 - (double)(k % 97));
}

static int run_map(int ctxt) {
    const int shapes[3][2] = {{5, 3}, {3, 5}, {4, 4}};
    const int ia = 2, ja = 3, ib = 3, jb = 2, AM = 9, AN = 9, BM = 9, BN = 9;
    int bad = 0;
    for (int t = 0; t < 4; ++t)
        for (int sh = 0; sh < 3; ++sh)
            for (int u = 0; u < 2; ++u)
                for (int dg = 0; dg < 2; ++dg) {
                    const int m = shapes[sh][0], n = shapes[sh][1];
                    const char uplo = "UL"[u], diag = "NU"[dg];
                    int da[9], db[9];
                    desc_of(da, AM, AN, 2, 2, ctxt);
                    desc_of(db, BM, BN, 3, 3, ctxt);
                    const size_t es = (size_t)REALS[t] * RSIZE[t];
                    void* a = malloc(es * AM * AN);
                    void* b = malloc(es * BM * BN);
                    void* b0 = malloc(es * BM * BN);
                    fill(a, b, t, AM, AN, BM, BN);
                    memcpy(b0, b, es * BM * BN);
                    MKL[t](&uplo, &diag, &m, &n, a, &ia, &ja, da, b, &ib, &jb, db, &ctxt);
                    printf("%c %c %c %d %d ", TYPES[t], uplo, diag, m, n);
                    for (int i = 0; i < BM; ++i)
                        for (int j = 0; j < BN; ++j) {
                            const size_t kb = (size_t)i + (size_t)j * BM;
                            const int changed = memcmp((char*)b + kb * es, (char*)b0 + kb * es, es) != 0;
                            const int li = i - (ib - 1), lj = j - (jb - 1);
                            const int inside = li >= 0 && li < m && lj >= 0 && lj < n;
                            if (changed && !inside) bad++;
                            if (changed) {
                                const size_t ka = (size_t)(ia - 1 + li) + (size_t)(ja - 1 + lj) * AM;
                                if (memcmp((char*)b + kb * es, (char*)a + ka * es, es)) bad++;
                            }
                        }
                    for (int li = 0; li < m; ++li)
                        for (int lj = 0; lj < n; ++lj) {
                            const size_t kb = (size_t)(ib - 1 + li) + (size_t)(jb - 1 + lj) * BM;
                            putchar(memcmp((char*)b + kb * es, (char*)b0 + kb * es, es) ? '1' : '0');
                        }
                    putchar('\n');
                    free(a); free(b); free(b0);
                }
    (void)get;
    if (bad) printf("BAD %d\n", bad);
    return bad;
}

#ifdef WITH_COSTA
static trmr2d_fn COSTA[4] = {costa_pstrmr2d, costa_pdtrmr2d, costa_pctrmr2d, costa_pztrmr2d};

static int run_gpu(int ctxt) {
    const int shapes[3][2] = {{70, 45}, {45, 70}, {64, 64}};
    const int ia = 3, ja = 1, ib = 1, jb = 2;
    int failures = 0;
    for (int t = 0; t < 4; ++t)
        for (int sh = 0; sh < 3; ++sh)
            for (int u = 0; u < 2; ++u)
                for (int dg = 0; dg < 2; ++dg) {
                    const int m = shapes[sh][0], n = shapes[sh][1];
                    const int AM = m + ia - 1, AN = n + ja - 1, BM = m + ib - 1, BN = n + jb - 1;
                    const char uplo = "UL"[u], diag = "NU"[dg];
                    int da[9], db[9];
                    desc_of(da, AM, AN, 16, 24, ctxt);
                    desc_of(db, BM, BN, 20, 12, ctxt);
                    const size_t es = (size_t)REALS[t] * RSIZE[t];
                    void* a = malloc(es * AM * AN);
                    void* b1 = malloc(es * BM * BN);
                    void* b2 = malloc(es * BM * BN);
                    fill(a, b1, t, AM, AN, BM, BN);
                    memcpy(b2, b1, es * BM * BN);
                    COSTA[t](&uplo, &diag, &m, &n, a, &ia, &ja, da, b1, &ib, &jb, db, &ctxt);
                    MKL[t](&uplo, &diag, &m, &n, a, &ia, &ja, da, b2, &ib, &jb, db, &ctxt);
                    const int ok = memcmp(b1, b2, es * BM * BN) == 0;
                    printf("p%ctrmr2d %c %c %dx%d %s\n", TYPES[t], uplo, diag, m, n, ok ? "ok" : "FAIL");
                    failures += !ok;
                    free(a); free(b1); free(b2);
                }
    /* m == 0 returns at once */
    {
        int da[9], db[9], zero = 0, n = 4, one = 1;
        desc_of(da, 8, 8, 2, 2, ctxt);
        desc_of(db, 8, 8, 2, 2, ctxt);
        double a[64], b[64], b0[64];
        fill(a, b, 1, 8, 8, 8, 8);
        memcpy(b0, b, sizeof b);
        costa_pdtrmr2d("U", "N", &zero, &n, a, &one, &one, da, b, &one, &one, db, &ctxt);
        const int ok = memcmp(b, b0, sizeof b) == 0;
        printf("pdtrmr2d m=0 no-op %s\n", ok ? "ok" : "FAIL");
        failures += !ok;
    }
    return failures;
}
#endif

int main(int argc, char** argv) {
    MPI_Init(&argc, &argv);
    int me, np, ctxt;
    Cblacs_pinfo(&me, &np);
    Cblacs_get(-1, 0, &ctxt);
    Cblacs_gridinit(&ctxt, "R", 1, np);
    int failures = 1;
    if (argc > 1 && !strcmp(argv[1], "map")) failures = run_map(ctxt);
#ifdef WITH_COSTA
    if (argc > 1 && !strcmp(argv[1], "gpu")) failures = run_gpu(ctxt);
#endif
    Cblacs_gridexit(ctxt);
    MPI_Finalize();
    printf("%s\n", failures ? "FAILED" : "ALL PASSED");
    return failures ? 1 : 0;
}
