"""GPU: a room that ticks at its microphones' capture rate (mmla_capture_*, mmla_{od,si,room}_pipeline_capture,
room.Room(capture=...)).

Every comparison is byte for byte against the numpy restatement of audioop's streaming ratecv
(tests/capture_ref.py, pinned against stdlib audioop in tests/test_capture_ref_cpu.py): there is no tolerance.
The fused ticks are compared with Room.tick on a second context fed the restatement's converted clips.
Synthetic weights (OD; SI with 8 sigmoid classes); the capture audio is tests/capture_inputs.py's, for which
tests/test_capture_inputs_cpu.py shows with the CPU oracles that both outcomes of the silent rule occur.
"""
import numpy as np
import pytest

import capture_inputs as ci
import capture_ref as cr
import cond_ref
from mmla_audio_amd import _lib, models, room, weights

pytestmark = pytest.mark.gpu

SI_K = 8
STREAMS, IPS, N = ci.STREAMS, ci.IPS, ci.N
RATES = (48000, 44100, 32000, 22050, 16000, 11025, 8000)
FORMATS = ((2, 0), (1, 0), (2, cr.MEAN), (2, 1), (1, 0), (2, cr.MEAN), (2, 1))     # one per rate
NAMES = ('od_probs', 'od_argmax', 'si_probs', 'si_argmax', 'silent', 'kept_len', 'pcm')

_OPEN = []
_W = {}


def _weights(kind):
    if kind not in _W:
        _W[kind] = (weights.synthetic(weights.OD, seed=81) if kind == weights.OD
                    else weights.synthetic(weights.SI, seed=82, n_classes=SI_K))
    return _W[kind]


def _new_ctx():
    c = _lib.Context(0)
    _OPEN.append(c)
    return c


def _models(c):
    od = models.OverlapDetectionModel(_weights(weights.OD), device=c)
    si = models.SpeakerIdModel(_weights(weights.SI), SI_K, _lib.HEAD_SIGMOID, device=c)
    return od, si


@pytest.fixture(autouse=True)
def _close_contexts():
    yield
    while _OPEN:
        _OPEN.pop().close()


@pytest.fixture(scope='module')
def pair():
    """(capture side, reference side): two contexts with both models loaded, kept for the module"""
    cs = []
    for _ in range(2):
        c = _lib.Context(0)
        cs.append((c,) + _models(c))
    yield cs
    for c, _, _ in cs:
        c.close()


@pytest.fixture(scope='module')
def noises():
    return [cond_ref.noise(p) for p in range(cond_ref.N_PROFILES)]


@pytest.fixture(scope='module')
def inputs():
    """per case: (format, the two ticks' raw capture, frames, the restatement's [(clips, out_lens)] per tick,
    its states after tick 2); computed once, read-only"""
    out = {}
    for case in ci.CASES:
        fmt, raws, frames = ci.capture_ticks(case)
        converted, conv = ci.restated(case)
        for a in raws + [q for q, _ in converted]:
            a.setflags(write=False)
        out[case] = (fmt, raws, frames, converted, conv.state_arrays())
    return out


def _same(got, want, what=''):
    assert len(got) == len(want), (what, len(got), len(want))
    for g, w, name in zip(got, want, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


def _gate_exercised(res):
    silent, kept = res[4], res[5]
    assert silent.any() and not silent.all(), kept
    assert np.array_equal(silent, kept < 4000)
    assert np.array_equal(res[1] == -1, silent) and np.array_equal(res[3] == -1, silent)


def _same_state(ctx, want, what=''):
    d, prev = ctx.capture_state()
    assert d.tolist() == want[0].tolist() and prev.tolist() == want[1].tolist(), (what, d, prev, want)


def _same_detectors(a, b, what=''):
    """the detectors of two contexts are in one state: the same decisions on probe audio (which advances both)"""
    probe = cond_ref.clips()
    va, sa = a.vad_remove_silence(probe, items_per_stream=IPS)
    vb, sb = b.vad_remove_silence(probe, items_per_stream=IPS)
    for i in range(len(probe)):
        assert np.array_equal(va[i], vb[i]) and np.array_equal(sa[i], sb[i]), (what, i)


# ---- the conversion alone ---------------------------------------------------------------------------

def _ragged_calls(rng, channels, ips, clip_frames=1000):
    """three consecutive calls for 3 streams x ips clips: raw capture and per-clip frame counts, zero and
    full length included, differing per stream"""
    calls = []
    for call in range(3):
        n = 3 * ips
        raw = (rng.standard_normal((n, clip_frames * channels)) * 9000).clip(-32768, 32767).astype(np.int16)
        raw[0, :8] = [32767, -32768, 32767, -32768, -1, 0, -3, 0]
        frames = rng.integers(1, clip_frames, n).astype(np.int32)
        frames[(call + 1) % n] = 0
        frames[(call + 2) % n] = clip_frames
        frames[(call + 3) % n] = 1
        calls.append((raw, frames))
    return calls


@pytest.mark.parametrize('ips', [1, 3])
@pytest.mark.parametrize('rate,fmt', list(zip(RATES, FORMATS)))
def test_convert_consecutive_calls(rate, fmt, ips):
    channels, channel = fmt
    rng = np.random.default_rng(rate + ips)
    c = _new_ctx()
    c.capture_reset(3, rate, channels, channel)
    ref = cr.Converter(3, rate, channels, channel)
    _same_state(c, ref.state_arrays(), 'fresh')
    for call, (raw, frames) in enumerate(_ragged_calls(rng, channels, ips)):
        want, want_lens = ref.convert(raw, frames, ips)
        got, got_lens = c.capture_convert(raw, frames, ips)
        assert got.shape == want.shape == (3 * ips, cr.out_clip_len(1000, rate))
        assert got_lens.tolist() == want_lens.tolist(), (rate, fmt, ips, call)
        assert got.tobytes() == want.tobytes(), (rate, fmt, ips, call)      # the zero tails included
        _same_state(c, ref.state_arrays(), (rate, fmt, ips, call))
    # frames=None: every clip whole; and the list form with its own lengths
    raw = _ragged_calls(rng, channels, ips)[0][0]
    want, want_lens = ref.convert(raw, None, ips)
    got, got_lens = c.capture_convert(raw, None, ips)
    assert got.tobytes() == want.tobytes() and got_lens.tolist() == want_lens.tolist()
    lst = [raw[i, :(200 + 37 * i) * channels] for i in range(3 * ips)]
    want, want_lens = ref.convert(raw, [200 + 37 * i for i in range(3 * ips)], ips)
    got, got_lens = c.capture_convert(lst, items_per_stream=ips)
    n_out = got.shape[1]
    assert got_lens.tolist() == want_lens.tolist() and got.tobytes() == want[:, :n_out].tobytes()
    assert not want[:, n_out:].any()
    _same_state(c, ref.state_arrays(), 'list')


@pytest.mark.parametrize('rate', [48000, 44100])
def test_chunked_equals_whole(rate):
    """a picked channel: the stream's outputs over consecutive calls, concatenated, are ctx.ratecv (audioop's
    whole-recording conversion from a fresh state) of the concatenated capture"""
    rng = np.random.default_rng(rate)
    c = _new_ctx()
    c.capture_reset(2, rate, 2, 1)
    pieces = [[], []]
    raws = [[], []]
    for frames in ((1000, 3), (0, 999), (517, 1000), (1, 2), (1000, 1000)):
        raw = (rng.standard_normal((2, 2000)) * 9000).clip(-32768, 32767).astype(np.int16)
        out, lens = c.capture_convert(raw, np.array(frames, np.int32))
        for s in range(2):
            pieces[s].append(out[s, :lens[s]])
            raws[s].append(raw[s, :2 * frames[s]])
    for s in range(2):
        whole = c.ratecv(np.concatenate(raws[s]), 2, rate, 16000)
        assert np.array_equal(np.concatenate(pieces[s]), whole[1::2]), (rate, s)


def test_host_pointers_stage_in_pieces_of_whole_streams():
    """more raw capture than one staging piece (64 MiB): 5 streams x 2 clips of 550 000 frames of 8 channels
    at 384 kHz, 8.8 MB per clip, go over in pieces of 3 + 2 streams; the device-pointer call on the same
    capture takes it in one piece.  Also the highest rate and channel count (ir = 24, or = 1)."""
    import torch
    rate, channels, channel, clip_frames, ips = 384000, 8, 5, 550000, 2
    rng = np.random.default_rng(384)
    base = (rng.standard_normal(7919 * channels) * 9000).clip(-32768, 32767).astype(np.int16)
    raw = np.stack([np.resize(np.roll(base, 131 * i), clip_frames * channels) for i in range(5 * ips)])
    frames = np.array([clip_frames, 7, 0, clip_frames, 549999, clip_frames, 1, 300000, clip_frames, 23], np.int32)
    assert raw.nbytes > 64 << 20 and 3 * ips * raw[0].nbytes <= 64 << 20 < 4 * ips * raw[0].nbytes
    ref = cr.Converter(5, rate, channels, channel)
    c, cd = _new_ctx(), _new_ctx()
    c.capture_reset(5, rate, channels, channel)
    cd.capture_reset(5, rate, channels, channel)
    x = torch.from_numpy(raw).cuda()
    L = cr.out_clip_len(clip_frames, rate)
    for call in range(2):
        want, want_lens = ref.convert(raw, frames, ips)
        got, got_lens = c.capture_convert(raw, frames, ips)
        assert got_lens.tolist() == want_lens.tolist() and got.tobytes() == want.tobytes(), call
        _same_state(c, ref.state_arrays(), ('pieces', call))
        out = torch.full((5 * ips, L), 7, dtype=torch.int16, device='cuda')
        lens = torch.zeros(5 * ips, dtype=torch.int32, device='cuda')
        fr = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        cd.capture_convert_dev(x.data_ptr(), 5 * ips, raw.shape[1], clip_frames, out.data_ptr(), L, lens.data_ptr(),
                               ips, fr.data_ptr())
        cd.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes() and lens.cpu().numpy().tolist() == want_lens.tolist()
        _same_state(cd, ref.state_arrays(), ('one piece', call))
        frames = frames[::-1].copy()


def test_room_convert_is_stateless_and_whole(pair):
    """Room.convert: a whole recording in the room's format from a fresh state, in chunks of one stream, the
    live converters untouched"""
    c, od, si = pair[0]
    r = room.Room(od, si, None, capture=room.CaptureFormat(44100, 2, room.MEAN))
    c.capture_reset(3, 44100, 2, room.MEAN)
    rng = np.random.default_rng(5)
    live = (rng.standard_normal((3, 600)) * 9000).astype(np.int16)
    c.capture_convert(live)
    before = c.capture_state()
    rec = (rng.standard_normal(2 * 10007) * 9000).clip(-32768, 32767).astype(np.int16)
    want, _ = cr.ratecv_fast(cr.mono(rec, 2, cr.MEAN), 44100, cr.fresh(44100))
    assert np.array_equal(r.convert(rec), want)
    assert np.array_equal(r.convert(rec, chunk_frames=1234), want)
    _same_state(c, before, 'live converters')


# ---- the fused ticks against the composition ---------------------------------------------------------

VARIANTS = {
    # name: (case, noises?, passes, silence_remove)
    '48k stereo pick 0': ('48k_stereo', True, 1, True),
    '44.1k mono ragged': ('441_mono', True, 1, True),
    'no noise recordings': ('48k_stereo', False, 1, True),
    'two passes': ('48k_stereo', True, 2, True),
    'no silence removal': ('441_mono', True, 1, False),
}


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_fused_tick_equals_tick_on_restated_clips(pair, inputs, noises, variant):
    case, with_noise, passes, sr = VARIANTS[variant]
    fmt, raws, frames, converted, states = inputs[case]
    (ca, od_a, si_a), (cb, od_b, si_b) = pair
    nz = noises if with_noise else None
    fused = room.Room(od_a, si_a, nz, capture=room.CaptureFormat(*fmt))
    plain = room.Room(od_b, si_b, nz)
    for t in range(2):
        first = t == 0
        got = fused.tick(raws[t], lens=frames, passes=passes, silence_remove=sr, items_per_stream=IPS,
                         reset_vad=first, reset_capture=first, return_pcm=True)
        q, out_lens = converted[t]
        want = plain.tick(q, lens=out_lens, passes=passes, silence_remove=sr, items_per_stream=IPS,
                          reset_vad=first, return_pcm=True)
        _same(tuple(got), tuple(want), (variant, 'tick', t))
        _gate_exercised(got)
    _same_state(ca, states, variant)
    if sr:
        _same_detectors(ca, cb, variant)


def _room_call(c, raw, frames, passes=1, sr=True, ips=IPS, **kw):
    return c.room_pipeline_capture(raw, frames, None, passes, sr, ips, return_pcm=True, nonstationary=True, **kw)


def _prepare(c, fmt, streams=STREAMS):
    c.capture_reset(streams, *fmt)
    c.vad_reset(streams, 3)


def test_state_advances_once_per_clip_under_microbatches(pair, inputs):
    """micro-batches of one stream: the conversion still runs once, in front of them"""
    fmt, raws, frames, converted, states = inputs['441_mono']
    (ca, _, _), (cb, _, _) = pair
    for c in (ca, cb):
        _prepare(c, fmt)
    ca.set_microbatch(od=IPS, si=IPS)
    try:
        for t in range(2):
            got = _room_call(ca, raws[t], frames)
            want = _room_call(cb, raws[t], frames)
            _same(got, want, ('micro-batches', t))
            _gate_exercised(got)
    finally:
        ca.set_microbatch()
    _same_state(ca, states, 'micro-batches')
    _same_state(cb, states, 'plain')
    _same_detectors(ca, cb, 'micro-batches')


def test_state_advances_once_per_clip_when_an_allocation_fails(monkeypatch, pair, inputs):
    """MMLA_DEBUG_FAIL_ALLOC=1 fails the context's first workspace allocation, inside the first conditioned
    micro-batch behind the conversion; only a micro-batch of more than 64 clips is halved, so the tick is
    tiled to 66 clips = 33 streams x 2 (-> 64 + 2).  The re-run re-reads the clips already converted."""
    fmt, raws, _, _, _ = inputs['48k_stereo']
    monkeypatch.setenv('MMLA_DEBUG_FAIL_ALLOC', '1')
    dbg, small = _new_ctx(), _new_ctx()
    monkeypatch.delenv('MMLA_DEBUG_FAIL_ALLOC')
    _models(dbg)
    _models(small)
    # the hook is live in this path: a tick of 6 clips, too few to halve, reports the failure
    _prepare(small, fmt)
    with pytest.raises(_lib.MmlaError) as e:
        small.room_pipeline_capture(raws[0], None, None, 0, True, IPS)
    assert e.value.code == -4, e.value
    cb = pair[1][0]
    for c in (dbg, cb):
        _prepare(c, fmt, 33)
    for t in range(2):
        raw = np.ascontiguousarray(np.tile(raws[t], (11, 1)))
        got = dbg.room_pipeline_capture(raw, None, None, 0, True, IPS, return_pcm=True)
        want = cb.room_pipeline_capture(raw, None, None, 0, True, IPS, return_pcm=True)
        _same(got, want, ('allocation failure', t))
        _gate_exercised(got)
    da, db = dbg.capture_state(), cb.capture_state()
    assert da[0].tolist() == db[0].tolist() == [-1] * 33 and da[1].tolist() == db[1].tolist()


def test_single_model_calls_and_device_twins(pair, inputs):
    import torch
    fmt, raws, frames, converted, states = inputs['441_mono']
    (ca, _, _), (cb, _, _) = pair
    width = raws[0].shape[1]
    L = cr.out_clip_len(width // fmt[1], fmt[0])
    dfr = torch.from_numpy(frames).cuda()
    for kind in ('od', 'si', 'room', 'convert'):
        for c in (ca, cb):
            _prepare(c, fmt)
        for t in range(2):
            want = _room_call(cb, raws[t], frames)
            x = torch.from_numpy(raws[t].copy()).cuda()
            odp = torch.zeros((N, 2), dtype=torch.float32, device='cuda')
            sip = torch.zeros((N, SI_K), dtype=torch.float32, device='cuda')
            oda = torch.zeros(N, dtype=torch.int32, device='cuda')
            sia = torch.zeros(N, dtype=torch.int32, device='cuda')
            silent = torch.zeros(N, dtype=torch.uint8, device='cuda')
            q = torch.full((N, L), 7, dtype=torch.int16, device='cuda')
            kept = torch.zeros(N, dtype=torch.int32, device='cuda')
            torch.cuda.synchronize()
            if kind == 'od':
                p, a, s, k, o = ca.od_pipeline_capture(raws[t], frames, None, 1, True, IPS, return_pcm=True,
                                                       nonstationary=True)
                _same((p, a, s, k, o), (want[0], want[1], want[4], want[5], want[6]), ('od', t))
            elif kind == 'si':
                p, a, s, k, o = ca.si_pipeline_capture(raws[t], frames, None, 1, True, IPS, return_pcm=True,
                                                       nonstationary=True)
                _same((p, a, s, k, o), (want[2], want[3], want[4], want[5], want[6]), ('si', t))
            elif kind == 'room':
                ca.room_pipeline_capture_dev(x.data_ptr(), N, width, width // fmt[1], 1, True, IPS, odp.data_ptr(),
                                             oda.data_ptr(), sip.data_ptr(), sia.data_ptr(), silent.data_ptr(),
                                             q.data_ptr(), kept.data_ptr(), dfr.data_ptr(), nonstationary=True)
                ca.synchronize()
                got = tuple(v.cpu().numpy() for v in (odp, oda, sip, sia, silent, kept, q))
                _same(got[:4] + (got[4].astype(bool),) + got[5:], want, ('room dev', t))
                assert ca.range_check() == 0
            else:
                ca.capture_convert_dev(x.data_ptr(), N, width, width // fmt[1], q.data_ptr(), L, kept.data_ptr(),
                                       IPS, dfr.data_ptr())
                ca.synchronize()
                assert q.cpu().numpy().tobytes() == converted[t][0].tobytes()
                assert kept.cpu().numpy().tolist() == converted[t][1].tolist()
        _same_state(ca, states, kind)
    # the device twins of the single-model calls, on a first tick
    for c in (ca, cb):
        _prepare(c, fmt)
    want = _room_call(cb, raws[0], frames)
    x = torch.from_numpy(raws[0].copy()).cuda()
    for kind, k, fn in (('od', 2, ca.od_pipeline_capture_dev), ('si', SI_K, ca.si_pipeline_capture_dev)):
        _prepare(ca, fmt)
        p = torch.zeros((N, k), dtype=torch.float32, device='cuda')
        a = torch.zeros(N, dtype=torch.int32, device='cuda')
        silent = torch.zeros(N, dtype=torch.uint8, device='cuda')
        kept = torch.zeros(N, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        fn(x.data_ptr(), N, width, width // fmt[1], 1, True, IPS, p.data_ptr(), a.data_ptr(), silent.data_ptr(),
           0, kept.data_ptr(), dfr.data_ptr(), nonstationary=True)
        ca.synchronize()
        i = 0 if kind == 'od' else 2
        _same((p.cpu().numpy(), a.cpu().numpy(), silent.cpu().numpy().astype(bool), kept.cpu().numpy()),
              (want[i], want[i + 1], want[4], want[5]), (kind, 'dev'))


def test_device_frames_are_clamped():
    import torch
    c = _new_ctx()
    c.capture_reset(2, 48000, 1, 0)
    ref = cr.Converter(2, 48000, 1, 0)
    raw = (np.random.default_rng(9).standard_normal((2, 900)) * 9000).astype(np.int16)
    want, want_lens = ref.convert(raw, np.array([0, 900], np.int32))
    x = torch.from_numpy(raw).cuda()
    fr = torch.tensor([-5, 100000], dtype=torch.int32, device='cuda')
    out = torch.full((2, 300), 7, dtype=torch.int16, device='cuda')
    lens = torch.zeros(2, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    c.capture_convert_dev(x.data_ptr(), 2, 900, 900, out.data_ptr(), 300, lens.data_ptr(), 1, fr.data_ptr())
    c.synchronize()
    assert lens.cpu().numpy().tolist() == want_lens.tolist()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    _same_state(c, ref.state_arrays())


# ---- errors, and capture=None ------------------------------------------------------------------------

def test_invalid_arguments_leave_the_states(pair, inputs, noises):
    fmt, raws, frames, _, _ = inputs['441_mono']
    c = pair[0][0]

    def invalid(fn, *args, code=-1, **kw):
        with pytest.raises(_lib.MmlaError) as e:
            fn(*args, **kw)
        assert e.value.code == code, e.value

    fresh = _new_ctx()
    invalid(fresh.capture_state)
    with pytest.raises(_lib.MmlaError):
        fresh.capture_convert(raws[0][:, :100])                       # no capture_reset at all
    scratch = np.zeros((6, 100), np.int16)
    rc = fresh.lib.mmla_capture_convert(fresh.h, raws[0].ctypes.data, 6, 100, None, 100, 1,
                                        scratch.ctypes.data, 100, scratch.ctypes.data, 0)
    assert rc == -1
    for bad in ((0, 1, 0), (384001, 1, 0), (48000, 0, 0), (48000, 9, 0), (48000, 2, 2), (48000, 1, 1),
                (48000, 2, -2), (48000, 1, cr.MEAN), (48000, 3, cr.MEAN)):
        invalid(fresh.capture_reset, 3, *bad)
    invalid(fresh.capture_reset, 0, 48000, 2, 0)

    _prepare(c, fmt)
    c.capture_convert(raws[0][:, :1000], np.full(N, 777, np.int32), IPS)     # move the states off fresh
    before = c.capture_state()
    assert before[0].tolist() != [cr.fresh(fmt[0])[0]] * STREAMS
    small = np.ascontiguousarray(raws[0][:, :1000])
    short = np.full(N, 500, np.int32)
    calls = (c.capture_convert, lambda *a, **k: c.room_pipeline_capture(*a, **k, passes=0),
             lambda *a, **k: c.od_pipeline_capture(*a, **k, passes=0),
             lambda *a, **k: c.si_pipeline_capture(*a, **k, passes=0))
    for fn in calls:
        invalid(fn, small, np.array([500, 500, -1, 500, 500, 500], np.int32), items_per_stream=IPS)
        invalid(fn, small, np.array([500, 500, 1001, 500, 500, 500], np.int32), items_per_stream=IPS)
        invalid(fn, small, short, items_per_stream=1)          # 6 streams, 3 were created
        invalid(fn, small, short, items_per_stream=3)          # 2 streams
        invalid(fn, small, short, items_per_stream=4)          # not whole streams
        invalid(fn, small, short, items_per_stream=0)
        invalid(fn, small[:4], short[:4], items_per_stream=IPS)
    # out_clip_len > 600 000: 1 653 751 frames at 44.1 kHz are 600 001 samples
    big = np.zeros((STREAMS, 1653751), np.int16)
    invalid(c.capture_convert, big, None, 1)
    invalid(c.room_pipeline_capture, big, None, None, 0, False, 1)
    # clip_stride < clip_frames * channels, null pointers
    o, ol = np.zeros((N, 1000), np.int16), np.zeros(N, np.int32)
    lib = c.lib
    assert lib.mmla_capture_convert(c.h, small.ctypes.data, N, 999, None, 1000, IPS, o.ctypes.data, 1000,
                                    ol.ctypes.data, 0) == -1
    assert lib.mmla_room_pipeline_capture(c.h, small.ctypes.data, N, 999, None, 1000, None, 0, 1, IPS, None, None,
                                          None, None, None, None, None, 0) == -1
    assert lib.mmla_capture_convert(c.h, None, N, 1000, None, 1000, IPS, o.ctypes.data, 1000, ol.ctypes.data,
                                    0) == -1
    assert lib.mmla_capture_convert(c.h, small.ctypes.data, N, 1000, None, 1000, IPS, o.ctypes.data, 300,
                                    ol.ctypes.data, 0) == -1          # out_stride < out_clip_len
    assert lib.mmla_capture_convert(c.h, small.ctypes.data, N, 1000, None, 1000, IPS, None, 1000, ol.ctypes.data,
                                    0) == -1
    # what mmla_condition rejects, checked before the conversion: the gate without a bank, nr_passes < 0, a
    # host profile outside the bank, silence removal without detectors of that stream count
    nb = _new_ctx()
    _models(nb)
    nb.capture_reset(STREAMS, *fmt)
    nb.capture_convert(small, np.full(N, 333, np.int32), IPS)
    nb_before = nb.capture_state()
    invalid(nb.room_pipeline_capture, small, short, None, 1, False, IPS)
    invalid(nb.room_pipeline_capture, small, short, None, 0, True, IPS)
    nb.vad_reset(STREAMS + 1, 3)
    invalid(nb.room_pipeline_capture, small, short, None, 0, True, IPS)
    nb.vad_reset(STREAMS, 3)
    invalid(nb.room_pipeline_capture, small, short, None, -1, True, IPS)
    nb.nr_set_noise_bank(noises)
    invalid(nb.room_pipeline_capture, small, short, [0, 1, 2, 3, 0, 0], 1, True, IPS)
    _same_state(nb, nb_before, 'mmla_condition checks')
    # a model that is not loaded: MMLA_E_NOWEIGHTS, states unchanged
    nw = _new_ctx()
    nw.load_weights(weights.OD, weights.pack(weights.OD, _weights(weights.OD)), 2)
    nw.si_classes = SI_K
    _prepare(nw, fmt)
    invalid(nw.room_pipeline_capture, small, short, None, 0, True, IPS, code=-3)
    invalid(nw.si_pipeline_capture, small, short, None, 0, True, IPS, code=-3)
    _same_state(nw, (np.full(STREAMS, cr.fresh(fmt[0])[0]), np.zeros(STREAMS)), 'no weights')
    _same_state(c, before, 'after every rejected call')
    # ... and the context still converts
    ref = cr.Converter(STREAMS, *fmt)
    ref.states = list(zip(before[0].tolist(), before[1].tolist()))
    want, want_lens = ref.convert(small, short, IPS)
    got, got_lens = c.capture_convert(small, short, IPS)
    assert got.tobytes() == want.tobytes() and got_lens.tolist() == want_lens.tolist()
    with pytest.raises(ValueError):
        room.CaptureFormat(48000, 1, room.MEAN)
    with pytest.raises(ValueError):
        room.CaptureFormat(0)
    assert room.CaptureFormat(48000) == (48000, 1, 0)


def test_capture_none_is_the_parent_path(pair, inputs, noises):
    """Room without a capture format and the models' predict_wavs_conditioned(capture=None) are the calls they
    were: the conditioned entry points on 16 kHz clips"""
    _, _, _, converted, _ = inputs['441_mono']
    (ca, od_a, si_a), (cb, od_b, si_b) = pair
    q, lens = converted[0]
    r = room.Room(od_a, si_a, noises)
    assert r.capture is None
    got = r.tick(q, lens=lens, items_per_stream=IPS, reset_vad=True, return_pcm=True)
    cb.nr_set_noise_bank(noises)
    cb.vad_reset(STREAMS, 3)
    mic = np.arange(N, dtype=np.int32) // IPS
    want = cb.room_pipeline_conditioned(q, lens, mic, 1, True, IPS, return_pcm=True)
    _same(tuple(got), want, 'room')
    _gate_exercised(got)
    cb.vad_reset(STREAMS, 3)
    p, a, s, k = od_a.predict_wavs_conditioned(q, noises, lens=lens, items_per_stream=IPS, reset_vad=True)
    _same((p, a), want[:2], 'od')
    assert np.array_equal(s, want[4]) and np.array_equal(k, want[5])
    p, a, s, k = si_a.predict_wavs_conditioned(q, noises, lens=lens, items_per_stream=IPS, reset_vad=True)
    _same((p, a), want[2:4], 'si')


def test_models_take_a_capture_format(pair, inputs, noises):
    """predict_wavs_conditioned(capture=...) of either model is its half of the room's tick; the converters are
    kept from call to call and reset on request"""
    fmt, raws, frames, converted, states = inputs['441_mono']
    (ca, od_a, si_a), (cb, od_b, si_b) = pair
    cf = room.CaptureFormat(*fmt)
    ticks = []
    r = room.Room(od_b, si_b, noises, capture=cf)
    for t in range(2):
        ticks.append(r.tick(raws[t], lens=frames, items_per_stream=IPS, reset_vad=t == 0, reset_capture=t == 0))
    for model, i in ((od_a, 0), (si_a, 2)):
        for t in range(2):
            p, a, s, k = model.predict_wavs_conditioned(raws[t], noises, lens=frames, items_per_stream=IPS,
                                                        reset_vad=t == 0, capture=cf, reset_capture=t == 0)
            _same((p, a, s, k), (ticks[t][i], ticks[t][i + 1], ticks[t].silent, ticks[t].kept_len), (i, t))
        _same_state(ca, states, 'kept from call to call')
