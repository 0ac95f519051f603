"""GPU: both detectors for a room from one conditioning (mmla_room_pipeline_conditioned, room.Room).

The joint call must equal, byte for byte, mmla_od_pipeline_conditioned and mmla_si_pipeline_conditioned,
each run on a context of its own (own noise bank, own freshly reset detectors) with the same arguments:
od_probs, od_argmax, si_probs, si_argmax, silent, kept_len, out_pcm -- on a first tick and on a second
tick on new audio, which shows the detector state the first left behind.  Synthetic weights (OD; SI with
8 sigmoid classes); 12 clips = 6 streams x 2 of tests/cond_ref.py's clips, 40 960 samples, three noise
profiles, the streams' microphones not the identity."""
import numpy as np
import pytest

import cond_ref
from mmla_audio_amd import _lib, weights

pytestmark = pytest.mark.gpu

L = cond_ref.L
SI_K = 8
STREAMS, IPS = 6, 2
N = STREAMS * IPS
MIC = np.repeat(np.array([0, 2, 1, 1, 0, 2], np.int32), IPS)       # stream s listens on microphone MIC[2 s]
LENS = np.array([L, 12000, L, 3999, L, L, 30000, L, L, 481, L, 4000], np.int32)
NAMES = ('od_probs', 'od_argmax', 'si_probs', 'si_argmax', 'silent', 'kept_len', 'out_pcm')

_OPEN = []
_PACKED = {}


def _packed(kind):
    if kind not in _PACKED:
        if kind == weights.OD:
            _PACKED[kind] = weights.pack(weights.OD, weights.synthetic(weights.OD, seed=81))
        else:
            _PACKED[kind] = weights.pack(weights.SI, weights.synthetic(weights.SI, seed=82, n_classes=SI_K), SI_K)
    return _PACKED[kind]


def _new_ctx(od=True, si=True):
    c = _lib.Context(0)
    _OPEN.append(c)
    if od:
        c.load_weights(weights.OD, _packed(weights.OD), 2)
    if si:
        c.load_weights(weights.SI, _packed(weights.SI), SI_K, _lib.HEAD_SIGMOID)
    return c


@pytest.fixture(autouse=True)
def _close_contexts():
    yield
    while _OPEN:
        _OPEN.pop().close()


@pytest.fixture(scope='module')
def ctxs():
    """(joint, OD single, SI single): three contexts, each with its own bank and detectors"""
    cs = [_new_ctx() for _ in range(3)]
    for c in cs:
        _OPEN.remove(c)
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope='module')
def ticks():
    """two ticks of 12 clips: the six clips in two orders, then other pairings"""
    x = cond_ref.clips()
    a = np.ascontiguousarray(np.concatenate([x, x[[5, 0, 2, 1, 3, 4]]]))
    b = np.ascontiguousarray(np.concatenate([x[[0, 5, 1, 4, 2, 3]], x[::-1]]))
    for t in (a, b):
        t.setflags(write=False)
    return a, b


@pytest.fixture(scope='module')
def noises():
    return [cond_ref.noise(p) for p in range(cond_ref.N_PROFILES)]


def _prepare(c, noises, passes, silence_remove, streams=STREAMS):
    if passes > 0:
        c.nr_set_noise_bank(noises)
    if silence_remove:
        c.vad_reset(streams, 3)


def _singles(od_ctx, si_ctx, x, lens, mic, passes, sr, ips=IPS):
    """the two single calls -> the joint call's tuple; their shared outputs must agree already"""
    p, a, s, k, q = od_ctx.od_pipeline_conditioned(x, lens, mic, passes, sr, ips, return_pcm=True)
    p2, a2, s2, k2, q2 = si_ctx.si_pipeline_conditioned(x, lens, mic, passes, sr, ips, return_pcm=True)
    assert np.array_equal(s, s2) and np.array_equal(k, k2) and np.array_equal(q, q2)
    return p, a, p2, a2, s, k, q


def _same(got, want, what=''):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


def _gate_exercised(res):
    silent, kept = res[4], res[5]
    assert silent.any() and not silent.all()
    assert np.array_equal(silent, kept < 4000)
    assert np.array_equal(res[1] == -1, silent) and np.array_equal(res[3] == -1, silent)


def _two_ticks(joint, od_ctx, si_ctx, ticks, noises, lens=None, passes=1, sr=True, what=''):
    for c in (joint, od_ctx, si_ctx):
        _prepare(c, noises, passes, sr)
    for t, x in enumerate(ticks):
        want = _singles(od_ctx, si_ctx, x, lens, MIC, passes, sr)
        got = joint.room_pipeline_conditioned(x, lens, MIC, passes, sr, IPS, return_pcm=True)
        _same(got, want, (what, 'tick', t))
        _gate_exercised(got)


def test_joint_equals_the_single_calls(ctxs, ticks, noises):
    _two_ticks(*ctxs, ticks, noises, what='plain')


def test_microbatches(ctxs, ticks, noises):
    joint = ctxs[0]
    joint.set_microbatch(od=4, si=4)          # three micro-batches of two streams
    try:
        _two_ticks(*ctxs, ticks, noises, what='micro-batches')
    finally:
        joint.set_microbatch()


def test_lens(ctxs, ticks, noises):
    _two_ticks(*ctxs, ticks, noises, lens=LENS, what='lens')


def test_three_passes(ctxs, ticks, noises):
    _two_ticks(*ctxs, ticks, noises, lens=LENS, passes=3, what='three passes')


def test_off_switch_is_the_two_plain_pipelines(ctxs, ticks):
    joint, od_ctx, si_ctx = ctxs
    for ln in (None, LENS):
        p0, a0, s0 = od_ctx.od_pipeline(ticks[0], lens=ln)
        p1, a1, s1 = si_ctx.si_pipeline(ticks[0], lens=ln)
        got = joint.room_pipeline_conditioned(ticks[0], ln, None, 0, False, 1, return_pcm=True)
        kept = np.full(N, L, np.int32) if ln is None else ln
        want = (p0, a0, p1, a1, s0, kept, cond_ref.zero_tails(np.array(ticks[0]), ln))
        _same(got, want, 'off')
        assert np.array_equal(s0, s1)
    assert got[4].any() and not got[4].all()


def test_device_pointers(ctxs, ticks, noises):
    import torch
    joint, od_ctx, si_ctx = ctxs
    for c in ctxs:
        _prepare(c, noises, 1, True)
    dl = torch.from_numpy(LENS).cuda()
    dm = torch.from_numpy(MIC).cuda()
    for t, xh in enumerate(ticks):
        want = _singles(od_ctx, si_ctx, xh, LENS, MIC, 1, True)
        x = torch.from_numpy(xh.copy()).cuda()
        odp = torch.zeros((N, 2), dtype=torch.float32, device='cuda')
        sip = torch.zeros((N, SI_K), dtype=torch.float32, device='cuda')
        oda = torch.zeros(N, dtype=torch.int32, device='cuda')
        sia = torch.zeros(N, dtype=torch.int32, device='cuda')
        silent = torch.zeros(N, dtype=torch.uint8, device='cuda')
        q = torch.full((N, L), 7, dtype=torch.int16, device='cuda')
        kept = torch.zeros(N, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        joint.room_pipeline_conditioned_dev(x.data_ptr(), N, L, L, 1, True, IPS, odp.data_ptr(), oda.data_ptr(),
                                            sip.data_ptr(), sia.data_ptr(), silent.data_ptr(), q.data_ptr(),
                                            kept.data_ptr(), dl.data_ptr(), dm.data_ptr())
        joint.synchronize()
        got = tuple(v.cpu().numpy() for v in (odp, oda, sip, sia, silent, kept, q))
        got = got[:4] + (got[4].astype(bool),) + got[5:]
        _same(got, want, ('device', t))
        _gate_exercised(got)
        assert joint.range_check() == 0


def _debug_ctx(monkeypatch, name, value):
    monkeypatch.setenv(name, value)
    c = _new_ctx()
    monkeypatch.delenv(name)
    return c


def test_split_lstm_rerun_repeats_the_network_alone(monkeypatch, ctxs, ticks, noises):
    """MMLA_DEBUG_LSTM_SPIN=-1: the split BiLSTM of either network gives up and the unsplit one repeats that
    network on the conditioning already made; two micro-batches (8 + 4 clips), two ticks"""
    dbg = _debug_ctx(monkeypatch, 'MMLA_DEBUG_LSTM_SPIN', '-1')
    dbg.set_microbatch(od=8, si=8)
    _two_ticks(dbg, ctxs[1], ctxs[2], ticks, noises, lens=LENS, what='split re-run')
    f32_reruns, split_reruns = dbg.debug_counters()
    assert f32_reruns == 0 and split_reruns == 8, (f32_reruns, split_reruns)   # 2 ticks x 2 micro-batches x 2 nets


def test_oom_retry_keeps_vad_state(monkeypatch, ctxs, ticks):
    """MMLA_DEBUG_FAIL_ALLOC=1 fails the context's first workspace allocation inside the joint call (no
    gate: building a bank allocates); only a micro-batch of more than 64 clips is halved: 66 clips as 33
    streams x 2 -> 64 + 2"""
    x = np.ascontiguousarray(np.tile(ticks[0][:6], (11, 1)))
    dbg = _debug_ctx(monkeypatch, 'MMLA_DEBUG_FAIL_ALLOC', '1')
    for c in (dbg, ctxs[1], ctxs[2]):
        c.vad_reset(33, 3)
    for call in (0, 1):
        want = _singles(ctxs[1], ctxs[2], x, None, None, 0, True)
        got = dbg.room_pipeline_conditioned(x, None, None, 0, True, IPS, return_pcm=True)
        _same(got, want, ('oom', call))
        _gate_exercised(got)


def test_the_conditioning_runs_once(ctxs, ticks, noises):
    joint, od_ctx, si_ctx = ctxs

    def launches(c, fn):
        _prepare(c, noises, 1, True)
        c.profile_enable(True)
        try:
            c.profile_read(reset=True)
            fn()
            prof = c.profile_read(reset=True)
        finally:
            c.profile_enable(False)
        return prof['nr'][1], prof['glue'][1]

    x = ticks[0]
    cond = launches(od_ctx, lambda: od_ctx.condition(x, LENS, MIC, 1, True, IPS))
    od = launches(od_ctx, lambda: od_ctx.od_pipeline_conditioned(x, LENS, MIC, 1, True, IPS))
    si = launches(si_ctx, lambda: si_ctx.si_pipeline_conditioned(x, LENS, MIC, 1, True, IPS))
    room = launches(joint, lambda: joint.room_pipeline_conditioned(x, LENS, MIC, 1, True, IPS))
    print('launches (nr, glue): condition', cond, 'od', od, 'si', si, 'room', room)
    assert cond[0] > 0 and od[0] == cond[0] and si[0] == cond[0]
    assert room[0] == od[0]
    assert room[1] == od[1] + si[1] - cond[1]
    # the conditioning's own plan, in absolute numbers: one micro-batch of N <= 512 clips of L samples, p
    # passes and silence removal -- one gate launch per pass (8 N L each); glue: the float conversion (6 N L),
    # a PCM_16 round trip per pass (8 N L, the last one to int16: 6 N L), the detector and the collector
    # (N L each), the tail fill (2 N L)
    for p in (1, 3):
        od_ctx.nr_set_noise_bank(noises)
        od_ctx.vad_reset(STREAMS, 3)
        od_ctx.profile_enable(True)
        try:
            od_ctx.profile_read(reset=True)
            od_ctx.condition(x, LENS, MIC, p, True, IPS)
            prof = od_ctx.profile_read(reset=True)
        finally:
            od_ctx.profile_enable(False)
        print('condition alone, passes', p, {k: v[1:] for k, v in prof.items()})
        assert prof['nr'][1:] == (p, 8 * N * L * p)
        assert prof['glue'][1:] == (p + 4, N * L * (8 * p + 8))
        assert all(prof[s][1] == 0 for s in _lib.STAGES if s not in ('nr', 'glue'))


def test_misuse(ticks, noises):
    x = ticks[0]
    c = _new_ctx(si=False)
    c.nr_set_noise_bank(noises)
    c.vad_reset(STREAMS, 3)
    c.si_classes = SI_K
    with pytest.raises(_lib.MmlaError) as e:
        c.room_pipeline_conditioned(x, None, MIC, 1, True, IPS)
    assert e.value.code == -3 and 'SI' in str(e.value), e.value
    c = _new_ctx(od=False)
    c.nr_set_noise_bank(noises)
    c.vad_reset(STREAMS, 3)
    with pytest.raises(_lib.MmlaError) as e:
        c.room_pipeline_conditioned(x, None, MIC, 1, True, IPS)
    assert e.value.code == -3 and 'OD' in str(e.value), e.value

    c = _new_ctx()

    def invalid(*args, **kw):
        with pytest.raises(_lib.MmlaError) as e:
            c.room_pipeline_conditioned(*args, **kw)
        assert e.value.code == -1, e.value

    invalid(x, None, None, 1, False, 1)          # the gate without a bank
    invalid(x, None, None, 0, True, 1)           # silence removal without detectors
    c.nr_set_noise_bank(noises)
    c.vad_reset(STREAMS, 3)
    invalid(x, None, None, -1, True, IPS)        # nr_passes < 0
    invalid(x, None, None, 1, True, 5)           # 12 clips are not whole streams of 5
    invalid(x, None, None, 1, True, 3)           # ... and 4 streams are not the 6 created
    invalid(x, None, None, 1, True, 0)
    invalid(x, None, [0, 1, 2, 3] + [0] * 8, 1, True, IPS)                 # a host profile index outside the bank
    invalid(np.zeros((1, 600001), np.int16), None, None, 1, False, 1)     # more than one gate chunk
    with pytest.raises(_lib.MmlaError) as e:                               # clip_stride < clip_len
        c._check(c.lib.mmla_room_pipeline_conditioned(c.h, x.ctypes.data, 2, 100, None, L, None, 0, 0, 1,
                                                      None, None, None, None, None, None, None, 0), 'stride')
    assert e.value.code == -1
    rc = c.lib.mmla_room_pipeline_conditioned(c.h, None, 2, L, None, L, None, 0, 0, 1, None, None, None, None,
                                              None, None, None, 0)         # clips without a pcm pointer
    assert rc == -1
    c.room_pipeline_conditioned(x, None, MIC, 1, True, IPS)               # and the context still works


def test_room_tick_and_labels(ticks, noises):
    from mmla_audio_amd import models, room
    c = _new_ctx(od=False, si=False)
    od = models.OverlapDetectionModel(weights.synthetic(weights.OD, seed=81), device=c)
    si = models.SpeakerIdModel(weights.synthetic(weights.SI, seed=82, n_classes=SI_K), SI_K,
                               _lib.HEAD_SIGMOID, device=c)
    other = models.SpeakerIdModel(si.W, SI_K, _lib.HEAD_SIGMOID, device=_new_ctx(od=False, si=False))
    with pytest.raises(ValueError):
        room.Room(od, other, noises)
    r = room.Room(od, si, noises)
    first = r.tick(ticks[0], mic=MIC, lens=LENS, items_per_stream=IPS, return_pcm=True)
    assert c.nr_bank_builds == 1
    second = r.tick(ticks[1], mic=MIC, lens=LENS, items_per_stream=IPS, return_pcm=True)
    assert c.nr_bank_builds == 1, 'the bank is rebuilt only when a noise clip changes'
    # the Context call on freshly reset detectors gives the first tick, then the second
    c.vad_reset(STREAMS, 3)
    _same(c.room_pipeline_conditioned(ticks[0], LENS, MIC, 1, True, IPS, return_pcm=True), tuple(first))
    _same(c.room_pipeline_conditioned(ticks[1], LENS, MIC, 1, True, IPS, return_pcm=True), tuple(second))
    # reset_vad starts afresh; the result without return_pcm carries no clips
    again = r.tick(ticks[0], mic=MIC, lens=LENS, items_per_stream=IPS, reset_vad=True)
    assert again.pcm is None
    _same(tuple(again)[:6], tuple(first)[:6])
    _gate_exercised(first)
    spk = {str(i): f'speaker{i}' for i in range(SI_K)}
    od_labels, si_labels = room.Room.labels(first, spk)
    for i in range(N):
        if first.silent[i]:
            assert first.od_argmax[i] == -1 and first.si_argmax[i] == -1
            assert od_labels[i] == 'silent' and si_labels[i] == 'silent'
        else:
            assert od_labels[i] == ('non-overlapped', 'overlapped')[first.od_argmax[i]]
            assert si_labels[i] == f'speaker{first.si_argmax[i]}'
    assert 'silent' in si_labels and any(s != 'silent' for s in si_labels)
