#!/bin/bash
# Regenerates the round's measurement artefacts (R=r03) on a GPU box; results under $OUT (default: profiles_out/refresh/ in the
# checkout; copy into profiles/).  Each rocprofv3 step runs python3 directly (no wrapper between the profiler and the program).
# Every section of the bench line, and every kernel in the traces, comes from `bench.py --full`.
set -e
R=${R:-r03}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/profiles_out/refresh}
TR=$(mktemp -d)
export TMPDIR=$TR
mkdir -p $OUT
cd $ROOT
echo "[1] bench (no profiler)"; timeout -k 10 600 python3 bench.py --full > $OUT/${R}_bench_n1.json 2> $OUT/bench.err
echo "[2] kernel trace of the driver's command"
cd $TR
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $TR/kt -o ${R} -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${R}_bench_n1_under_rocprof.json 2> $OUT/kt.err
cd $ROOT
python3 tools/prof_summary.py $TR/kt 60 > $OUT/${R}_bench_n1_kernel_summary.txt
cp $TR/kt/${R}_kernel_stats.csv $OUT/${R}_bench_n1_kernel_stats.csv
echo "[3] PMC pass (FETCH_SIZE only)"
cd $TR
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $TR/pmc -o bench -- python3 $ROOT/bench.py --steps 4 --warmup 1 --full --no-cpu-baseline --ttft-prompts 1 --no-speculation > $OUT/pmc_bench.json 2> $OUT/pmc.err
cd $ROOT
python3 tools/pmc_summary.py $TR/pmc $OUT/${R}_gemv_traffic.json > /dev/null
echo "[4] Qwen2.5-7B INT8"; timeout -k 10 600 python3 bench.py --model qwen25_7b --full --no-cpu-baseline > $OUT/${R}_bench_n1_qwen25_7b_int8.json 2> $OUT/qwen.err
for T in 2 4 8; do
  echo "[5] TP $T loopback kernel trace"
  cd $TR
  timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d $TR/tp$T -o tp -- python3 $ROOT/bench.py --gpus $T --tp-loopback --steps 8 --warmup 2 --full --ttft-prompts 1 --no-cpu-baseline > $OUT/tp${T}_bench.json 2> $OUT/tp$T.err
  cd $ROOT
  python3 tools/tp_kernel_summary.py $TR/tp$T $T > $OUT/${R}_tp${T}_loopback_kernels.json
done
echo "[6] 70B TP 8 loopback kernel trace"
cd $TR
timeout -k 10 900 rocprofv3 --kernel-trace --output-format csv -d $TR/tp70 -o tp -- python3 $ROOT/bench.py --model llama33_70b --gpus 8 --tp-loopback --steps 8 --warmup 2 --full --ttft-prompts 1 --no-cpu-baseline > $OUT/tp70_bench.json 2> $OUT/tp70.err
cd $ROOT
python3 tools/tp_kernel_summary.py $TR/tp70 8 > $OUT/${R}_tp8_llama33_70b_loopback_kernels.json
ls -la $OUT
echo done
