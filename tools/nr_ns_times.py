"""The non-stationary noise gate beside the stationary one, timed (profiles/r11_nr_ns_times.txt).

  python tools/nr_ns_times.py measure --variant stationary|nonstationary --out times.jsonl [--runs 3]
  python tools/nr_ns_times.py table times.jsonl [more.jsonl ...]

measure runs ONE variant per process (run the two in alternating processes on one box) and appends one
JSON line per case and run:
  gate   nr_reduce (a bank of one) or nr_reduce_ns on device pointers, 1, 64 and 512 clips of 40 960
         samples: kernel ms of the call's launches from the context's event timer (stage 'nr'), --runs
         times after a warm-up.
  tick   64 microphones x 1 clip, one gate pass + silence removal, host pointers,
         room_pipeline_conditioned with a bank of 64 profiles or with nonstationary=True: wall ms, and the
         per-stage kernel ms of one more run.
--skip-tick leaves the tick out (for a kernel-trace run of the gate alone)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

L = 40960
COUNTS = (1, 64, 512)


def _clips(n):
    from oracle import synth
    rng = np.random.default_rng(7)
    pool = []
    for s in range(8):
        x = synth.clip(5 * s, L).astype(np.float64) + 60.0 * rng.standard_normal(L)
        pool.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return np.stack(pool)[np.arange(n) % 8]


def measure_gate(_lib, ns, runs, emit):
    import torch
    ctx = _lib.Context(0)
    if not ns:
        ctx.nr_set_noise((0.002 * np.random.default_rng(50).standard_normal(16000)).astype(np.float32))
    fn = ctx.nr_reduce_ns_dev if ns else ctx.nr_reduce_dev
    for n in COUNTS:
        y = torch.from_numpy(_clips(n).astype(np.float32) / np.float32(32768.0)).cuda()
        out = torch.empty_like(y)
        torch.cuda.synchronize()
        for r in range(-1, runs):                     # -1: the warm-up (workspace allocation)
            ctx.profile_enable(True)
            ctx.profile_read(True)
            fn(y.data_ptr(), n, L, L, out.data_ptr())
            ctx.synchronize()
            ms, launches, _ = ctx.profile_read(True)['nr']
            ctx.profile_enable(False)
            if r >= 0:
                emit(dict(kind='gate', variant='nonstationary' if ns else 'stationary', clips=n, run=r,
                          ms=ms, launches=launches))
        assert torch.isfinite(out).all() and bool(out.any())
    ctx.close()


def measure_tick(_lib, ns, runs, emit):
    from mmla_audio_amd import weights
    mics = 64
    x = _clips(mics)
    c = _lib.Context(0)
    c.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=1)), 2)
    c.load_weights(weights.SI, weights.pack(weights.SI, weights.synthetic(weights.SI, seed=2, n_classes=8), 8),
                   8, _lib.HEAD_SIGMOID)
    mic = None
    if not ns:
        c.nr_set_noise_bank([(0.002 * 2 ** (p % 4) * np.random.default_rng(50 + p).standard_normal(16000))
                             .astype(np.float32) for p in range(mics)])
        mic = np.arange(mics, dtype=np.int32)
    c.vad_reset(mics, 3)
    variant = 'nonstationary' if ns else 'stationary'

    def tick():
        return c.room_pipeline_conditioned(x, None, mic, 1, True, 1, nonstationary=ns)

    tick()
    for r in range(runs):
        t = time.perf_counter()
        tick()
        emit(dict(kind='tick', variant=variant, run=r, wall_ms=1e3 * (time.perf_counter() - t)))
    c.profile_enable(True)
    c.profile_read(True)
    kept = tick()[5]
    stages = {s: [ms, n] for s, (ms, n, _) in c.profile_read(True).items()}
    c.profile_enable(False)
    emit(dict(kind='tick_stages', variant=variant, stages=stages, kept=[int(k) for k in kept]))
    c.close()


def table(paths):
    rows = [json.loads(ln) for p in paths for ln in open(p) if ln.strip()]

    def cells(v):
        return ' '.join(f'{x:.3f}' for x in v)

    print('gate kernel ms (event timer, stage nr), clips of 40 960 samples, device pointers; every run')
    print('| clips | stationary (bank of one) | non-stationary | ratio of the minima |')
    print('|---|---|---|---|')
    for n in COUNTS:
        v = {k: [r['ms'] for r in rows if r['kind'] == 'gate' and r['clips'] == n and r['variant'] == k]
             for k in ('stationary', 'nonstationary')}
        if v['stationary'] and v['nonstationary']:
            print(f"| {n} | {cells(v['stationary'])} | {cells(v['nonstationary'])} | "
                  f"{min(v['nonstationary']) / min(v['stationary']):.2f} |")
    print()
    print('room tick, 64 microphones x 1 clip, one gate pass + silence removal, host pointers')
    print('| variant | wall ms, every run | kernel ms: nr / glue / od_fe / si_fe / conv / lstm / head (launches) |')
    print('|---|---|---|')
    for k in ('stationary', 'nonstationary'):
        wall = [r['wall_ms'] for r in rows if r['kind'] == 'tick' and r['variant'] == k]
        st = [r for r in rows if r['kind'] == 'tick_stages' and r['variant'] == k]
        cell = ''
        if st:
            s = st[-1]['stages']
            cell = ' / '.join(f'{s[q][0]:.2f}' for q in ('nr', 'glue', 'od_fe', 'si_fe', 'conv', 'lstm', 'head'))
            cell += f' ({sum(v[1] for v in s.values())})'
        if wall:
            print(f'| {k} | {cells(wall)} | {cell} |')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    m = sub.add_parser('measure')
    m.add_argument('--variant', choices=('stationary', 'nonstationary'), required=True)
    m.add_argument('--out', required=True)
    m.add_argument('--runs', type=int, default=3)
    m.add_argument('--skip-tick', action='store_true')
    t = sub.add_parser('table')
    t.add_argument('files', nargs='+')
    args = ap.parse_args()
    if args.cmd == 'table':
        return table(args.files)
    from mmla_audio_amd import _lib
    _lib.load_library()
    ns = args.variant == 'nonstationary'
    with open(args.out, 'a') as f:
        def emit(row):
            f.write(json.dumps(row) + '\n')
            f.flush()
        measure_gate(_lib, ns, args.runs, emit)
        if not args.skip_tick:
            measure_tick(_lib, ns, args.runs, emit)


if __name__ == '__main__':
    main()
