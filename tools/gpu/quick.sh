#!/bin/bash
# dev: a few GPU test files (args) then the default bench line without the CPU baseline
set -o pipefail
export PYTHONUNBUFFERED=1
export OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest -x -v --timeout 200 --timeout-method thread "$@" > $OUT/quick.log 2>&1 || { echo "tests rc=$?"; tail -40 $OUT/quick.log; exit 1; }
tail -3 $OUT/quick.log
timeout -k 10 600 python bench.py --full --no-cpu-baseline --no-latency > $OUT/bench_q.json 2> $OUT/bench_q.err || { echo "bench rc=$?"; tail -20 $OUT/bench_q.err; exit 1; }
python - <<'PY'
import json, os
d = json.loads(open(os.environ['OUT'] + '/bench_q.json').read())
print('value', d['value'], 'roof', d['roofline']['frac'], 'stages', d['stages'])
print('parity', {k: d['parity'][k] for k in ('logp_err_net', 'logp_max_abs_err', 'img_lsb_pixels', 'argmax_agree')})
print('f32', d['precision_f32']['value'], d['precision_f32']['argmax_differs_from_f16x3'])
PY
