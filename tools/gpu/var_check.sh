#!/bin/bash
# variant check: parity sample of a variant build on a workload, then A/B against the product build
#   var_check.sh <variant.so> <workload> [rounds]
cd $GRAFT_REPO_ROOT
export OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
V=$1; wl=$2; r=${3:-2}
timeout -k 10 300 python3 tools/bench_with_lib.py $V --full --workload $wl --no-cpu-baseline --no-f32 --no-latency --steps 1 --warmup 1 > $OUT/vc.log 2>&1 || { tail -20 $OUT/vc.log; exit 1; }
grep '^{' $OUT/vc.log | python3 -c "import json,sys;d=json.loads(sys.stdin.read());print('$(basename $V) parity', {k: v for k, v in d['parity'].items() if k != 'sample'})"
bash tools/gpu/ab.sh $wl mmla_audio_amd/libmmla.so $V $r
