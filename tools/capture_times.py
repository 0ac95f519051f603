"""The room tick at the microphones' capture rate, timed (profiles/r12_capture_times.txt).

  python tools/capture_times.py measure --variant capture|parent|host --out times.jsonl [--runs 5]
  python tools/capture_times.py table times.jsonl [more.jsonl ...]

measure runs ONE variant per process (run them in alternating processes on one box) and appends one JSON
line per case and run, for 1, 64 and 512 streams x 1 clip of 122 880 stereo frames at 48 kHz (2.56 s; channel
0 holds tools/nr_ns_times.py's 16 kHz clips thrice, so the converted audio is the parent path's audio):
  capture  convert: capture_convert on device pointers, kernel ms of its two launches (phase + sample) from the
           context's event timer (stage 'glue'), and GB/s over raw-in + converted-out bytes;
           tick: room_pipeline_capture, one stationary gate pass + silence removal, wall ms with host pointers
           and with device pointers (the call + a stream synchronisation)
  parent   tick: room_pipeline_conditioned on the same clips already at 16 kHz mono, host and device pointers
  host     what a live room does today in front of every tick: audioop pick (or tomono) + ratecv per clip with
           its carried state, one core, ms per tick of n streams
Every case: one warm-up, then --runs timed runs, all reported."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

L = 40960
FRAMES = 3 * L
STREAMS = (1, 64, 512)
RATE, CHANNELS, CHANNEL = 48000, 2, 0


def _clips16k(n):
    from oracle import synth
    rng = np.random.default_rng(7)
    pool = []
    for s in range(8):
        x = synth.clip(5 * s, L).astype(np.float64) + 60.0 * rng.standard_normal(L)
        pool.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return np.stack(pool)[np.arange(n) % 8]


def _capture(x):
    raw = np.empty((x.shape[0], FRAMES, 2), np.int16)
    raw[:, :, 0] = np.repeat(x, 3, axis=1)
    raw[:, :, 1] = -(raw[:, ::-1, 0] // 2)
    return raw.reshape(x.shape[0], -1)


def _room_ctx(_lib, n):
    from mmla_audio_amd import weights
    c = _lib.Context(0)
    c.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=1)), 2)
    c.load_weights(weights.SI, weights.pack(weights.SI, weights.synthetic(weights.SI, seed=2, n_classes=8), 8),
                   8, _lib.HEAD_SIGMOID)
    c.nr_set_noise_bank([(0.002 * 2 ** (p % 4) * np.random.default_rng(50 + p).standard_normal(16000))
                         .astype(np.float32) for p in range(n)])
    c.vad_reset(n, 3)
    return c


def _timed(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return out


def _dev_outputs(torch, n, width):
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device='cuda')
    return dict(odp=z((n, 2), torch.float32), oda=z(n, torch.int32), sip=z((n, 8), torch.float32),
                sia=z(n, torch.int32), silent=z(n, torch.uint8), kept=z(n, torch.int32),
                q=z((n, width), torch.int16))


def measure_gpu(_lib, capture, runs, emit):
    import torch
    variant = 'capture' if capture else 'parent'
    for n in STREAMS:
        x16 = _clips16k(n)
        x = _capture(x16) if capture else x16
        mic = np.arange(n, dtype=np.int32)
        c = _room_ctx(_lib, n)
        dx = torch.from_numpy(x).cuda()
        dmic = torch.from_numpy(mic).cuda()
        o = _dev_outputs(torch, n, L)
        torch.cuda.synchronize()
        if capture:
            c.capture_reset(n, RATE, CHANNELS, CHANNEL)
            for r in range(-1, runs):                 # -1: the warm-up (buffers, code objects)
                c.profile_enable(True)
                c.profile_read(True)
                c.capture_convert_dev(dx.data_ptr(), n, x.shape[1], FRAMES, o['q'].data_ptr(), L,
                                      o['kept'].data_ptr())
                c.synchronize()
                ms, launches, _ = c.profile_read(True)['glue']
                c.profile_enable(False)
                if r >= 0:
                    emit(dict(kind='convert', variant=variant, streams=n, run=r, ms=ms, launches=launches,
                              bytes=n * 2 * (FRAMES * CHANNELS + L)))
            assert np.array_equal(o['q'].cpu().numpy(), x16), 'thrice-held capture converts to the 16 kHz clips'

            def host():
                return c.room_pipeline_capture(x, None, mic, 1, True, 1)

            def dev():
                c.room_pipeline_capture_dev(dx.data_ptr(), n, x.shape[1], FRAMES, 1, True, 1, o['odp'].data_ptr(),
                                            o['oda'].data_ptr(), o['sip'].data_ptr(), o['sia'].data_ptr(),
                                            o['silent'].data_ptr(), 0, o['kept'].data_ptr(), 0, dmic.data_ptr())
                c.synchronize()
        else:
            def host():
                return c.room_pipeline_conditioned(x, None, mic, 1, True, 1)

            def dev():
                c.room_pipeline_conditioned_dev(dx.data_ptr(), n, L, L, 1, True, 1, o['odp'].data_ptr(),
                                                o['oda'].data_ptr(), o['sip'].data_ptr(), o['sia'].data_ptr(),
                                                o['silent'].data_ptr(), 0, o['kept'].data_ptr(), 0, dmic.data_ptr())
                c.synchronize()
        for name, fn in (('host', host), ('dev', dev)):
            for r, ms in enumerate(_timed(fn, runs)):
                emit(dict(kind='tick', variant=variant, pointers=name, streams=n, run=r, wall_ms=ms))
        kept = host()[5]
        emit(dict(kind='tick_kept', variant=variant, streams=n, kept_sum=int(kept.sum())))
        c.close()


def measure_host(runs, emit):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        import audioop
    x = _capture(_clips16k(8))
    blobs = [c.tobytes() for c in x]
    for how in ('pick', 'tomono'):
        for n in STREAMS:
            states = [None] * n

            def tick():
                for s in range(n):
                    raw = blobs[s % 8]
                    mono = (np.frombuffer(raw, np.int16)[0::2].tobytes() if how == 'pick'
                            else audioop.tomono(raw, 2, 0.5, 0.5))
                    _, states[s] = audioop.ratecv(mono, 2, 1, RATE, 16000, states[s])

            for r, ms in enumerate(_timed(tick, runs)):
                emit(dict(kind='host', variant='host', how=how, streams=n, run=r, wall_ms=ms))


def table(paths):
    rows = [json.loads(ln) for p in paths for ln in open(p) if ln.strip()]

    def span(v, fmt='{:.3f}'):
        return f'{fmt.format(min(v))} - {fmt.format(max(v))} ({len(v)})' if v else 'not measured'

    print('conversion kernels (capture_phase_kernel + capture_sample_kernel), device pointers, event timer;')
    print('48 kHz stereo -> 16 kHz mono, 122 880 frames per stream; min - max (runs)')
    print('| streams | kernel ms, both launches | GB/s over raw-in + converted-out bytes |')
    print('|---|---|---|')
    for n in STREAMS:
        v = [r for r in rows if r['kind'] == 'convert' and r['streams'] == n]
        if v:
            gbs = [r['bytes'] / (r['ms'] * 1e-3) / 1e9 for r in v]
            print(f"| {n} | {span([r['ms'] for r in v], '{:.4f}')} | {span(gbs, '{:.1f}')} |")
    print()
    print('room tick, one stationary gate pass + silence removal, wall ms; min - max (runs)')
    print('| streams | capture, host ptr | capture, device ptr | parent (16 kHz in), host ptr | parent, device ptr '
          '| host audioop pick + ratecv | host audioop tomono + ratecv |')
    print('|---|---|---|---|---|---|---|')
    for n in STREAMS:
        def tick(variant, pointers):
            return span([r['wall_ms'] for r in rows if r['kind'] == 'tick' and r['variant'] == variant and
                         r['pointers'] == pointers and r['streams'] == n])

        def host(how):
            return span([r['wall_ms'] for r in rows if r['kind'] == 'host' and r['how'] == how and
                         r['streams'] == n])

        print(f"| {n} | {tick('capture', 'host')} | {tick('capture', 'dev')} | {tick('parent', 'host')} | "
              f"{tick('parent', 'dev')} | {host('pick')} | {host('tomono')} |")
    kept = {(r['variant'], r['streams']): r['kept_sum'] for r in rows if r['kind'] == 'tick_kept'}
    same = all(kept.get(('capture', n)) == kept.get(('parent', n)) for n in STREAMS)
    print()
    print(f'kept samples per tick, capture vs parent: {"equal" if same else "DIFFERENT"} '
          f'({[kept.get(("capture", n)) for n in STREAMS]})')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    m = sub.add_parser('measure')
    m.add_argument('--variant', choices=('capture', 'parent', 'host'), required=True)
    m.add_argument('--out', required=True)
    m.add_argument('--runs', type=int, default=5)
    t = sub.add_parser('table')
    t.add_argument('files', nargs='+')
    args = ap.parse_args()
    if args.cmd == 'table':
        return table(args.files)
    with open(args.out, 'a') as f:
        def emit(row):
            f.write(json.dumps(row) + '\n')
            f.flush()
        if args.variant == 'host':
            return measure_host(args.runs, emit)
        from mmla_audio_amd import _lib
        _lib.load_library()
        measure_gpu(_lib, args.variant == 'capture', args.runs, emit)


if __name__ == '__main__':
    main()
