#!/bin/bash
# round 6, call r6u: the bucket replay's common path without lane branches
# (inactive and shared-context lanes write spare LDS slots): GPU suite, bench
# x2, kernel statistics under the bench's load and alone.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${TAG:-r6u}
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
    if [ $rc -ne 0 ]; then exit $rc; fi
}
step tests timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread -o cache_dir=/tmp/pyc > $O/tests.log 2>&1
step write_inputs timeout -k 10 300 python -u bench.py --write-inputs $IN > $O/write_inputs.log 2>&1
for rep in 1 2; do
    step ab_$rep timeout -k 10 300 python -u bench.py --full --inputs $IN --no-legs > $O/ab_$rep.json 2>> $O/ab.err
done
cd /tmp
B="$R/bench.py --full --inputs $IN --no-legs --no-verify --text-leg 0"
step prof timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o run -- python3 -u $B --steps 10 > $O/prof_bench.json 2> $O/prof_bench.err
step solo timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/solo -o run -- python3 -u $B --contexts 1 --steps 6 > $O/solo_bench.json 2> $O/solo_bench.err
cd $R
for d in prof solo; do
    K=$(find $O/$d -name '*kernel_stats.csv' | head -1)
    T=$(find $O/$d -name '*kernel_trace.csv' | head -1)
    python3 scripts/kstats_csv.py $K > $O/${d}_kernel_stats.txt 2>&1 || true
    python3 scripts/front_cycle.py $T > $O/${d}_front_cycle.txt 2>&1 || true
done
find $O -name '*kernel_trace.csv' -delete
find $O -name '*.csv' -size +4M -delete
true
