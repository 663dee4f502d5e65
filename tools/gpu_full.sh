#!/bin/bash
# full check of the current tree: -m gpu suite, smoke, bench (N=1), cfg 5 'N' / 'T', the
# multi-GPU entries rehearsed on one GPU, rocprofv3 kernel trace of the bench, PMC passes
set -o pipefail
O=gpurun_out/${1:-full}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1 || exit 1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || exit 1
timeout -k 10 300 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err || exit 1
timeout -k 10 300 python3 bench.py --full --workload cfg5 --cfg5-op N --steps 10 --no-cpu-baseline > $O/c5N.json 2> $O/c5N.err || exit 1
timeout -k 10 300 python3 bench.py --full --workload cfg5 --cfg5-op T --steps 10 --no-cpu-baseline > $O/c5T.json 2> $O/c5T.err || exit 1
timeout -k 10 400 python3 bench.py --full --extra cfg3,cfg4:32768,cfg5:N --steps 5 --no-cpu-baseline --no-e2e > $O/extra.json 2> $O/extra.err || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o trace --output-format csv -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-e2e --no-extra > $O/prof.log 2>&1 || exit 1
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 200 rocprofv3 --pmc $c -d $O/pmc_$c -o p --output-format csv -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-e2e --no-extra > $O/pmc_$c.log 2>&1 || exit 1
done
tools/c5_pmc.sh ${1:-full}_c5pmc || exit 1
tools/c34_prof.sh ${1:-full}_c34 || exit 1
