#!/bin/bash
# kernel trace of the full bench (decoder + C3 pipeline) for per-kernel time shares
set -e
TAG=${1:-pipe}
export TMPDIR=/tmp
O=${OUT:-bench_out}/$TAG
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -T -d $O/trace -o kt -- python3 bench.py --steps 4 --warmup 1 --no-cpu-baseline --full > $O/trace.log 2>&1
cat $O/trace/kt_kernel_stats.csv
