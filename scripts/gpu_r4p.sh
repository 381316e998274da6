#!/bin/bash
# round 4, call r4p: the AUX run lists from the dense sort's scan (k_runs_dense,
# no pass over the sorted keys): the GPU suite, then the bench with and without
# it on the same inputs (SA_FIND_RUNS=1: k_find_runs).
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${TAG:-r4p}
O=$R/gpurun_out/$TAG
IN=/dev/shm/sa_bench_inputs
mkdir -p $O
cd $R
export TMPDIR=/tmp SA_NO_BUILD=1
trap 'rm -rf $IN' EXIT
step() {
    local name=$1; shift
    local t0=$SECONDS
    "$@"; local rc=$?
    echo "$name rc=$rc $((SECONDS - t0))s" >> $O/steps.txt
    if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
}
step tests timeout -k 10 480 python -u -m pytest tests -m gpu -v --timeout 120 --timeout-method thread -o cache_dir=/tmp/pyc > $O/tests.log 2>&1
step write_inputs timeout -k 10 300 python -u bench.py --write-inputs $IN > $O/write_inputs.log 2>&1
step bench_a timeout -k 10 300 python -u bench.py --full --inputs $IN --no-legs --text-leg 0 > $O/bench_a.json 2> $O/bench_a.err
SA_FIND_RUNS=1 step bench_find timeout -k 10 300 python -u bench.py --full --inputs $IN --no-legs --text-leg 0 > $O/bench_find.json 2> $O/bench_find.err
step bench_b timeout -k 10 300 python -u bench.py --full --inputs $IN --no-legs --text-leg 0 > $O/bench_b.json 2> $O/bench_b.err
