#!/bin/bash
# the GPU test suite, then (optional) the default bench line; every GPU step under its own limit
set -o pipefail
export PYTHONUNBUFFERED=1
export OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/suite.log 2>&1 || { echo "suite rc=$?"; tail -30 $OUT/suite.log; exit 1; }
tail -3 $OUT/suite.log
if [ "$1" = "bench" ]; then
  timeout -k 10 600 python bench.py --full > $OUT/bench_od.json 2> $OUT/bench_od.err || { echo "bench rc=$?"; tail -20 $OUT/bench_od.err; exit 1; }
  cat $OUT/bench_od.json
fi
