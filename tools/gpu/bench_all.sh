#!/bin/bash
# Round measurement: the four bench workloads (default = the headline OD pipeline) + rocprof kernel
# stats of the OD pipeline.  Outputs under $OUT/ (default bench_out/; copied into profiles/ by hand).
cd $GRAFT_REPO_ROOT
export OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 python3 -u bench.py --full > $OUT/bench_od.json.log 2>&1 || exit $?
grep '^{' $OUT/bench_od.json.log > $OUT/bench_od.json
timeout -k 10 600 python3 -u bench.py --full --workload si_pipeline > $OUT/bench_si.json.log 2>&1 || exit $?
grep '^{' $OUT/bench_si.json.log > $OUT/bench_si.json
timeout -k 10 600 python3 -u bench.py --full --workload si_pipeline --classes 8 > $OUT/bench_si8.json.log 2>&1 || exit $?
grep '^{' $OUT/bench_si8.json.log > $OUT/bench_si8.json
timeout -k 10 600 python3 -u bench.py --full --workload od_features > $OUT/bench_fe.json.log 2>&1 || exit $?
grep '^{' $OUT/bench_fe.json.log > $OUT/bench_fe.json
timeout -k 10 600 python3 -u bench.py --full --workload noise_gate > $OUT/bench_nr.json.log 2>&1 || exit $?
grep '^{' $OUT/bench_nr.json.log > $OUT/bench_nr.json
rm -rf $OUT/prof_bench
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o od -- python3 -u bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-f32 --no-parity --no-latency > $OUT/prof_bench.log 2>&1 || exit $?
python3 - <<'PY'
import json, os
for f in ('od', 'si', 'si8', 'fe', 'nr'):
    d = json.load(open(os.environ['OUT'] + f'/bench_{f}.json'))
    print(f, d['value'], d['unit'], 'ms/step', round(d['ms_per_step'], 2), 'roof', {k: d['roofline'][k] for k in ('kernel', 'achieved', 'peak', 'frac') if k in d['roofline']}, 'cpu', (d.get('cpu_baseline') or {}).get('value'))
PY
# keep only the stats summaries (traces exceed gpurun's copy-back limit)
find $OUT/prof_bench -type f ! -name '*_stats.csv' -delete
