#!/bin/bash
# round 4, call r4fin2: the final tree (pass R with batched v_readlane) -- the
# GPU suite, smoke, the default bench with every leg, then 5 / 6 contexts on
# the bench's batches (--no-legs).
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out/${TAG:-r4fin2}
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
    if [ $rc -ne 0 ]; then exit $rc; fi
}
step tests timeout -k 10 480 python -u -m pytest tests -m gpu -v --timeout 120 --timeout-method thread -o cache_dir=/tmp/pyc > $O/tests.log 2>&1
step smoke timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
step bench timeout -k 10 660 python -u bench.py --full --e2e-log $O/e2e.log > $O/bench.json 2> $O/bench.err
step write_inputs timeout -k 10 300 python -u bench.py --write-inputs $IN > $O/write_inputs.log 2>&1
step bench_c6 timeout -k 10 300 python -u bench.py --full --inputs $IN --no-legs --text-leg 0 --contexts 6 > $O/bench_c6.json 2> $O/bench_c6.err
step bench_c5 timeout -k 10 300 python -u bench.py --full --inputs $IN --no-legs --text-leg 0 --contexts 5 > $O/bench_c5.json 2> $O/bench_c5.err
