"""The speech detector's two kernels and the room tick, timed (profiles/r10_vad_times.txt).

  python tools/vad_times.py measure --tag new --out times.jsonl [--lib path/to/libmmla.so]
  python tools/vad_times.py table times.jsonl [more.jsonl ...]

measure appends one JSON line per case and variant:
  detector   vad_remove_silence on device pointers, clips of 40 960 samples: 1, 64, 512 and 4096 streams
             x 1 item and 1 stream x 64 items.  Kernel ms from the context's event timer: the call's
             launches (detector + collector) minus the collector's own launch on the same flags.
             Variants: 'thread' (a context under MMLA_NO_VADW=1) and 'wave' (MMLA_VADW=1), alternating,
             --runs times after a warm-up of each.
  tick       64 microphones x 1 clip, one gate pass + silence removal, host pointers: the joint call,
             the two single calls on two contexts; wall ms and the per-stage kernel ms of one more run.
A library from before this kernel (--lib, e.g. a build of the parent commit) has neither the switches nor
the joint call: its variants are 'thread' and the single calls only.  Run the two libraries in
alternating processes on one box; table prints min-max per tag."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

L = 40960
CASES = ((1, 1), (64, 1), (512, 1), (4096, 1), (1, 64))    # (streams, items per stream)
NEW_SYMBOLS = ('mmla_room_pipeline_conditioned', 'mmla_debug_vad_path')


def _load(path):
    import ctypes
    from mmla_audio_amd import _lib
    if path:
        try:
            import torch  # noqa: F401  (its HIP runtime first, as load_library does)
        except ImportError:
            pass
        probe = ctypes.CDLL(path)
        old = not all(hasattr(probe, s) for s in NEW_SYMBOLS)
        if old:
            for s in NEW_SYMBOLS:
                _lib.SIGNATURES.pop(s, None)
        _lib.load_library(path)
        return _lib, old
    _lib.load_library()
    return _lib, False


def _ctx_under(_lib, name):
    os.environ[name] = '1'
    try:
        return _lib.Context(0)
    finally:
        del os.environ[name]


def _clips(n):
    from oracle import synth
    rng = np.random.default_rng(7)
    pool = []
    for s in range(8):
        x = synth.clip(5 * s, L).astype(np.int32)
        a, b = sorted(rng.integers(0, L, 2))
        x[a:b] = rng.integers(-3, 4, b - a)          # a near-silent stretch
        c = int(rng.integers(0, L // 2))
        x[c:c + 4800] = 0                            # a digital-zero gap
        pool.append(x.astype(np.int16))
    return np.stack(pool)[np.arange(n) % 8]


def detector_ms(_lib, ctx, bufs, streams, ips):
    pcm, out, olen, speech, nf = bufs
    n = streams * ips
    ctx.vad_reset(streams, 3)
    ctx.profile_enable(True)
    ctx.profile_read(True)
    ctx._check(ctx.lib.mmla_vad_remove_silence(ctx.h, pcm.data_ptr(), n, L, None, L, ips, out.data_ptr(),
                                               olen.data_ptr(), speech.data_ptr(), nf, _lib.MMLA_DEVICE_PTR),
               'mmla_vad_remove_silence')
    ctx.synchronize()
    both = ctx.profile_read(True)['glue'][0]
    ctx._check(ctx.lib.mmla_vad_collect(ctx.h, pcm.data_ptr(), n, L, None, L, speech.data_ptr(), nf,
                                        out.data_ptr(), olen.data_ptr(), _lib.MMLA_DEVICE_PTR), 'mmla_vad_collect')
    ctx.synchronize()
    col = ctx.profile_read(True)['glue'][0]
    ctx.profile_enable(False)
    return both - col, col


def measure_detector(_lib, old, tag, runs, emit):
    import torch
    ctxs = {'thread': _lib.Context(0) if old else _ctx_under(_lib, 'MMLA_NO_VADW')}
    if not old:
        ctxs['wave'] = _ctx_under(_lib, 'MMLA_VADW')
    nf = (L - 1) // 480
    for streams, ips in CASES:
        n = streams * ips
        pcm = torch.from_numpy(_clips(n)).cuda()
        bufs = (pcm, torch.empty_like(pcm), torch.zeros(n, dtype=torch.int32, device='cuda'),
                torch.zeros((n, nf), dtype=torch.uint8, device='cuda'), nf)
        torch.cuda.synchronize()
        ref = None
        for name, c in ctxs.items():                 # warm-up; the two kernels' flags must agree
            detector_ms(_lib, c, bufs, streams, ips)
            flags = bufs[3].cpu().numpy().copy()
            assert ref is None or np.array_equal(ref, flags), 'the kernels disagree'
            ref = flags
        for r in range(runs):
            for name, c in ctxs.items():
                ms, col = detector_ms(_lib, c, bufs, streams, ips)
                emit(dict(kind='detector', tag=tag, variant=name, streams=streams, ips=ips, run=r,
                          ms=ms, collector_ms=col))
    for c in ctxs.values():
        c.close()


def measure_tick(_lib, old, tag, runs, emit):
    from mmla_audio_amd import weights
    mics = 64
    x = _clips(mics)
    noises = [(0.002 * 2 ** (p % 4) * np.random.default_rng(50 + p).standard_normal(16000)).astype(np.float32)
              for p in range(mics)]
    mic = np.arange(mics, dtype=np.int32)
    packed = (weights.pack(weights.OD, weights.synthetic(weights.OD, seed=1)),
              weights.pack(weights.SI, weights.synthetic(weights.SI, seed=2, n_classes=8), 8))

    def ctx():
        c = _lib.Context(0)
        c.load_weights(weights.OD, packed[0], 2)
        c.load_weights(weights.SI, packed[1], 8, _lib.HEAD_SIGMOID)
        c.nr_set_noise_bank(noises)
        c.vad_reset(mics, 3)
        return c

    a, b = ctx(), ctx()
    variants = {'two single calls': lambda: (a.od_pipeline_conditioned(x, None, mic, 1, True, 1),
                                             b.si_pipeline_conditioned(x, None, mic, 1, True, 1))}
    if not old:
        j = ctx()
        variants['joint call'] = lambda: j.room_pipeline_conditioned(x, None, mic, 1, True, 1)
    for fn in variants.values():
        fn()
    for r in range(runs):
        for name, fn in variants.items():
            t = time.perf_counter()
            fn()
            emit(dict(kind='tick', tag=tag, variant=name, run=r, wall_ms=1e3 * (time.perf_counter() - t)))
    for name, fn in variants.items():                # one more run under the event timer
        cs = (a, b) if name == 'two single calls' else (j,)
        for c in cs:
            c.profile_enable(True)
            c.profile_read(True)
        fn()
        stages = {}
        for c in cs:
            for s, (ms, n, _) in c.profile_read(True).items():
                stages[s] = [stages.get(s, [0, 0])[0] + ms, stages.get(s, [0, 0])[1] + n]
            c.profile_enable(False)
        emit(dict(kind='tick_stages', tag=tag, variant=name, stages=stages))


def table(paths):
    rows = [json.loads(ln) for p in paths for ln in open(p) if ln.strip()]

    def span(v):
        return f'{min(v):.3f}-{max(v):.3f}'

    print('detector kernel ms (event timer, call minus collector), clips of 40 960 samples; min-max over runs')
    keys = sorted({(r['tag'], r['variant']) for r in rows if r['kind'] == 'detector'})
    print('| streams x items | ' + ' | '.join(f'{t} {v}' for t, v in keys) + ' | collector |')
    print('|---|' + '---|' * (len(keys) + 1))
    for streams, ips in CASES:
        sel = [r for r in rows if r['kind'] == 'detector' and r['streams'] == streams and r['ips'] == ips]
        if not sel:
            continue
        cells = [span([r['ms'] for r in sel if (r['tag'], r['variant']) == k]) for k in keys]
        print(f'| {streams} x {ips} | ' + ' | '.join(cells) + f' | {span([r["collector_ms"] for r in sel])} |')
    print()
    print('room tick, 64 microphones x 1 clip, one gate pass + silence removal, host pointers')
    print('| tag | variant | wall ms (min-max) | kernel ms: nr / glue / od_fe / si_fe / conv / lstm / head (launches) |')
    print('|---|---|---|---|')
    for tag, variant in sorted({(r['tag'], r['variant']) for r in rows if r['kind'] == 'tick'}):
        wall = [r['wall_ms'] for r in rows if r['kind'] == 'tick' and (r['tag'], r['variant']) == (tag, variant)]
        st = [r for r in rows if r['kind'] == 'tick_stages' and (r['tag'], r['variant']) == (tag, variant)]
        cell = ''
        if st:
            s = st[-1]['stages']
            cell = ' / '.join(f'{s[k][0]:.2f}' for k in ('nr', 'glue', 'od_fe', 'si_fe', 'conv', 'lstm', 'head'))
            cell += f' ({sum(v[1] for v in s.values())})'
        print(f'| {tag} | {variant} | {span(wall)} | {cell} |')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    m = sub.add_parser('measure')
    m.add_argument('--tag', default='new')
    m.add_argument('--lib', default=None)
    m.add_argument('--out', required=True)
    m.add_argument('--runs', type=int, default=3)
    m.add_argument('--skip-tick', action='store_true')
    t = sub.add_parser('table')
    t.add_argument('files', nargs='+')
    args = ap.parse_args()
    if args.cmd == 'table':
        return table(args.files)
    _lib, old = _load(args.lib)
    with open(args.out, 'a') as f:
        def emit(row):
            f.write(json.dumps(row) + '\n')
            f.flush()
        measure_detector(_lib, old, args.tag, args.runs, emit)
        if not args.skip_tick:
            measure_tick(_lib, old, args.tag, args.runs, emit)


if __name__ == '__main__':
    main()
