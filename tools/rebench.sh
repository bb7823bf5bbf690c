#!/bin/bash
# The bench line and the kernel trace of refresh_profiles.sh alone (steps 1 and 2), once a new gemv_traffic.json is in place.
set -e
R=${R:-r03}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/profiles_out/refresh}
TR=$(mktemp -d)
export TMPDIR=$TR
mkdir -p $OUT
cd $ROOT
timeout -k 10 600 python3 bench.py --full > $OUT/${R}_bench_n1.json 2> $OUT/bench.err
cd $TR
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TR/kt -o ${R} -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${R}_bench_n1_under_rocprof.json 2> $OUT/kt.err
cd $ROOT
python3 tools/prof_summary.py $TR/kt 60 > $OUT/${R}_bench_n1_kernel_summary.txt
cp $TR/kt/${R}_kernel_stats.csv $OUT/${R}_bench_n1_kernel_stats.csv
tail -c 600 $OUT/${R}_bench_n1.json
