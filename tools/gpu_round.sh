#!/bin/bash
# One GPU session: GPU test suite, full bench line (--full), rocprofv3 kernel stats of the same workload.  usage: tools/gpu_round.sh <tag> [pytest args]
TAG=$1; shift
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$(realpath -m ${OUT:-$ROOT/results})      # logs, bench lines and kernel stats go here
mkdir -p $OUT
cd $ROOT
timeout -k 10 900 python -m pytest tests -m gpu -q "$@" > $OUT/${TAG}_tests.log 2>&1
echo "tests rc=$?"; tail -3 $OUT/${TAG}_tests.log
timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -5 $OUT/${TAG}_bench.err; exit 1; }
cat $OUT/${TAG}_bench.json | cut -c1-600
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o p -- python3 $ROOT/bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-kernel-timing --serial > $OUT/${TAG}_prof.log 2>&1
echo "rocprof rc=$?"
find $OUT/${TAG}_prof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/${TAG}_kernel_stats.csv
find $OUT/${TAG}_prof -name "*kernel_trace.csv" -delete
head -25 $OUT/${TAG}_kernel_stats.csv | cut -c1-160
