#!/bin/bash
# r05 GPU record: the -m gpu suite (or the given test files), smoke, the default bench (compact line
# + detail file), optionally a kernel trace (--stats) of the headline leg and the FETCH/WRITE PMC
# passes. Every GPU step under its own time limit; stops at the first failure.
# Usage: tools/r05_gpu.sh TAG [bench|nobench] [trace|notrace] [pmc|nopmc] [TESTS...]
set -e
export TMPDIR=/tmp
TAG=${1:-r05}
MODE=${2:-bench}
TRACE=${3:-notrace}
PMC=${4:-nopmc}
shift 4 || shift $#
TESTS=${@:-tests}
O=$GRAFT_REPO_ROOT/gpurun_out/$TAG
mkdir -p $O
cd $GRAFT_REPO_ROOT
if [ "$TESTS" != none ]; then
  timeout -k 10 700 python -u -m pytest $TESTS -m gpu -v --timeout 200 --timeout-method thread -p no:cacheprovider > $O/pytest.log 2>&1 || { tail -40 $O/pytest.log; exit 1; }
  tail -1 $O/pytest.log
  timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { tail -20 $O/smoke.log; exit 1; }
  tail -1 $O/smoke.log
fi
if [ "$MODE" = bench ]; then
  timeout -k 10 700 python bench.py --full --detail $O/bench_detail.json > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
  echo bench done; wc -c $O/bench.json
fi
if [ "$TRACE" = trace ]; then
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_headline -o kt -- python3 bench.py --no-cpu-baseline --legs none --steps 20 --detail $O/trace_detail.json > $O/trace_headline.log 2>&1 || { tail -20 $O/trace_headline.log; exit 1; }
  echo headline trace done
fi
if [ "$PMC" = pmc ]; then
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout -s KILL 180 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/pmc_$c -o pmc -- python3 bench.py --no-cpu-baseline --legs none --steps 3 --warmup 1 --detail $O/pmc_detail.json > $O/pmc_$c.log 2>&1 || { tail -5 $O/pmc_$c.log; exit 1; }
  done
  python3 tools/pmc_pipeline.py $O/pmc_FETCH_SIZE/pmc_counter_collection.csv $O/pmc_WRITE_SIZE/pmc_counter_collection.csv $O/pmc_pipeline.json
fi
echo all done
