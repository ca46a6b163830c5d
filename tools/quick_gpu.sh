#!/bin/bash
# quick GPU iteration: parity tests, bench, kernel trace + SQ counters for the decoder kernel
set -e
TAG=${1:-quick}
export TMPDIR=/tmp
O=${OUT:-bench_out}/$TAG
mkdir -p $O
timeout -k 10 600 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $O/pytest.log 2>&1 || { tail -30 $O/pytest.log; exit 1; }
tail -2 $O/pytest.log
timeout -k 10 300 python bench.py --steps 10 --warmup 2 --no-cpu-baseline --full > $O/bench.json 2> $O/bench.err
cat $O/bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -T -d $O/trace -o kt -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --full > $O/trace.log 2>&1
cat $O/trace/kt_kernel_stats.csv
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_VMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE --kernel-trace --output-format csv -T -d $O/pmc_sq -o pmc -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --full > $O/pmc_sq.log 2>&1
python3 tools/pmc_summary.py $O/pmc_sq/pmc_counter_collection.csv
