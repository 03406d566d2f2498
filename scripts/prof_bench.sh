#!/bin/bash
# rocprofv3 --kernel-trace --stats over bench.py --full without the CPU baseline; the summaries land beside the trace directory (copy to profiles/).
export TMPDIR=/tmp
R=$PWD
OUT=$R/gpurun_out/benchprof
rm -rf $OUT
D=$(dirname "$OUT")
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $OUT -o p -- python3 bench.py --full --no-cpu-baseline > $D/bench_under_rocprof.log 2>&1 || exit 1
DB=$(ls $OUT/*.db | head -1)
python3 scripts/rocpd_summary.py $DB > $R/gpurun_out/bench_kernel_trace_stats.csv || exit 1
python3 scripts/rocpd_summary.py $DB bygrid > $R/gpurun_out/bench_kernel_trace_bygrid.csv || exit 1
rm -rf $OUT
grep -h "i8_syrk" $R/gpurun_out/bench_kernel_trace_bygrid.csv | cut -c1-160
grep -o '"avg_launch_ms": [0-9.]*' $R/gpurun_out/bench_under_rocprof.log | head -2
