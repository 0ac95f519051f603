"""GPU: mmla_si_enrol_embed -- registration recordings conditioned, windowed and embedded in one call.

Every result is compared byte for byte with a composition of calls the library already has, run on a
second context: mmla_condition on freshly reset detectors (or, past one gate chunk, nr_reduce_bank ->
pcm16 -> vad_remove_silence), si_features_seq per conditioned recording, one si_embed of the zero-filled
[n_rec * w_max] batch."""
import numpy as np
import pytest

import capture_inputs
import cond_ref
import enrol_inputs
from mmla_audio_amd import _lib, models, room, weights

pytestmark = pytest.mark.gpu

SI_K = 8
CLIP, LENS, PROFILE = enrol_inputs.CLIP, enrol_inputs.LENS, enrol_inputs.PROFILE
W_MAX = enrol_inputs.windows(CLIP)


@pytest.fixture(scope='module')
def si_w():
    return weights.synthetic(weights.SI, seed=82, n_classes=SI_K)


def _ctx(si_w, bank=True):
    c = _lib.Context(0)
    c.load_weights(weights.SI, weights.pack(weights.SI, si_w, SI_K), SI_K, _lib.HEAD_SIGMOID)
    if bank:
        c.nr_set_noise_bank(enrol_inputs.noises())
    return c


@pytest.fixture(scope='module')
def ctxs(si_w):
    """(the context that enrols, the context of the composition), each with its own bank"""
    cs = [_ctx(si_w), _ctx(si_w)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope='module')
def recs():
    return enrol_inputs.recordings()


@pytest.fixture(scope='module')
def enrolled(ctxs, recs):
    """test (a)'s call, made once: (emb, n_windows, kept_len, out_pcm)"""
    out = ctxs[0].si_enrol_embed(recs, lens=LENS, profile=PROFILE, passes=1, silence_remove=True,
                                 return_pcm=True)
    for a in out:
        a.setflags(write=False)
    return out


def test_three_recordings_equal_the_composition(ctxs, recs, enrolled):
    emb, nw, kept, pcm = enrolled
    ref = ctxs[1]
    ref.vad_reset(3, 3)
    q, k = ref.condition(recs, LENS, PROFILE, 1, True, 1)
    print('kept_len', kept.tolist(), 'of', LENS.tolist(), 'n_windows', nw.tolist())
    assert kept.dtype == np.int32 and kept.tobytes() == k.tobytes()
    assert pcm.shape == (3, CLIP) and pcm.dtype == np.int16 and pcm.tobytes() == q.tobytes()
    # not vacuous: the silence removal took something out of one recording and left something of one
    assert (LENS - kept >= 480).any() and (kept >= 4000).any() and kept[2] == 0
    assert nw.tolist() == [enrol_inputs.windows(int(m)) for m in kept]
    assert nw[2] == 0 and nw.max() >= 1
    feat = np.zeros((3, W_MAX, 256, 39), np.float32)
    for i in range(3):
        if kept[i] > 0:
            feat[i, :nw[i]] = ref.si_features_seq(q[i, :kept[i]])
    want = ref.si_embed(feat.reshape(3 * W_MAX, 256, 39)).reshape(3, W_MAX, 512)
    assert emb.shape == want.shape and emb.dtype == np.float32
    assert emb.tobytes() == want.tobytes()
    assert np.isfinite(emb).all() and np.ptp(emb[0, 0]) > 0


def test_independent_of_the_microbatch(ctxs, recs, enrolled):
    c = ctxs[0]
    c.set_microbatch(si=1)            # one recording per conditioning, one window per network pass
    try:
        again = c.si_enrol_embed(recs, lens=LENS, profile=PROFILE, passes=1, silence_remove=True,
                                 return_pcm=True)
    finally:
        c.set_microbatch()
    for got, want in zip(again, enrolled):
        assert got.tobytes() == want.tobytes()


def test_device_pointers(ctxs, recs, enrolled):
    import torch
    c = ctxs[0]
    x = torch.from_numpy(recs.copy()).cuda()
    dl = torch.from_numpy(LENS).cuda()
    dp = torch.from_numpy(PROFILE).cuda()
    emb = torch.zeros((3, W_MAX, 512), dtype=torch.float32, device='cuda')
    q = torch.full((3, CLIP), 7, dtype=torch.int16, device='cuda')
    kept = torch.zeros(3, dtype=torch.int32, device='cuda')
    nw = torch.zeros(3, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    c.si_enrol_embed_dev(x.data_ptr(), 3, CLIP, CLIP, emb.data_ptr(), 1, True, 3, q.data_ptr(), kept.data_ptr(),
                         nw.data_ptr(), dl.data_ptr(), dp.data_ptr())
    c.synchronize()
    for got, want in zip((emb, nw, kept, q), enrolled):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    assert c.range_check() == 0


def test_a_recording_longer_than_one_gate_chunk(ctxs):
    x = enrol_inputs.long_recording()
    n = enrol_inputs.LONG
    assert n > 600000 and n % 480
    emb, nw, kept, pcm = ctxs[0].si_enrol_embed(x[None], profile=[1], return_pcm=True)
    ref = ctxs[1]
    y = x.astype(np.float32) / np.float32(32768.0)
    q = ref.pcm16(ref.nr_reduce_bank(y, profile=1))
    ref.vad_reset(1, 3)
    voiced, _ = ref.vad_remove_silence(q[None])
    print('kept', kept.tolist(), 'of', n, 'n_windows', nw.tolist())
    assert kept[0] == len(voiced[0]) and 4000 <= kept[0] <= n - 480
    assert pcm[0, :kept[0]].tobytes() == voiced[0].tobytes() and not pcm[0, kept[0]:].any()
    assert nw[0] == enrol_inputs.windows(int(kept[0]))
    assert emb.shape == (1, enrol_inputs.windows(n), 512)
    feat = ref.si_features_seq(voiced[0])
    assert emb[0, :nw[0]].tobytes() == ref.si_embed(feat).tobytes()


def _room(si_w, fmt):
    c = _lib.Context(0)
    od = models.OverlapDetectionModel(weights.synthetic(weights.OD, seed=81), device=c)
    si = models.SpeakerIdModel(si_w, SI_K, _lib.HEAD_SIGMOID, device=c)
    noises = [cond_ref.noise(p) for p in range(cond_ref.N_PROFILES)]
    return room.Room(od, si, noises, capture=room.CaptureFormat(*fmt))


def test_the_live_state_is_untouched(si_w):
    """a room in a capture format ticks, enrols two speakers, ticks again: the second tick's converters,
    detectors and OD results are those of a twin room that did not enrol in between"""
    fmt, raws, frames = capture_inputs.capture_ticks('441_mono')
    mic = np.repeat(np.array([0, 2, 1], np.int32), capture_inputs.IPS)
    a, b = _room(si_w, fmt), _room(si_w, fmt)
    try:
        kw = dict(mic=mic, lens=frames, items_per_stream=capture_inputs.IPS, return_pcm=True)
        ra, rb = a.tick(raws[0], **kw), b.tick(raws[0], **kw)
        for got, want in zip(ra, rb):
            assert got.tobytes() == want.tobytes()
        state = [s.copy() for s in a.ctx.capture_state()]
        speakers = np.stack([enrol_inputs.voiced(120.0, 70, cond_ref.L, [(9000, 20000)]),
                             enrol_inputs.voiced(210.0, 71, cond_ref.L, [(25000, 33000)])])
        reg = a.register(list(capture_inputs.capture_441_mono(speakers)), ['ann', 'bo'], mic=[1, 2], epochs=2)
        assert (reg.kept_len >= 4000).all() and reg.n_windows.tolist() == [1, 1]
        assert a.si.n_classes == 2
        for got, want in zip(a.ctx.capture_state(), state):
            assert got.tobytes() == want.tobytes(), 'the enrolment moved a live converter'
        ra, rb = a.tick(raws[1], **kw), b.tick(raws[1], **kw)
        for name in ('od_probs', 'od_argmax', 'silent', 'kept_len', 'pcm'):
            assert getattr(ra, name).tobytes() == getattr(rb, name).tobytes(), name
        assert ra.si_probs.shape == (capture_inputs.N, 2) and rb.si_probs.shape == (capture_inputs.N, SI_K)
        for got, want in zip(a.ctx.capture_state(), b.ctx.capture_state()):
            assert got.tobytes() == want.tobytes()
        assert ra.silent.any() and not ra.silent.all()
    finally:
        a.ctx.close()
        b.ctx.close()


def test_nonstationary_gate_and_misuse(si_w, recs):
    c = _ctx(si_w, bank=False)
    ref = _ctx(si_w, bank=False)
    try:
        with pytest.raises(_lib.MmlaError) as e:           # the stationary gate without a bank
            c.si_enrol_embed(recs, lens=LENS)
        assert e.value.code == -1, e.value
        emb, nw, kept, pcm = c.si_enrol_embed(recs, lens=LENS, nonstationary=True, return_pcm=True)
        ref.vad_reset(3, 3)
        q, k = ref.condition(recs, LENS, None, 1, True, 1, nonstationary=True)
        assert kept.tobytes() == k.tobytes() and pcm.tobytes() == q.tobytes()
        assert nw.tolist() == [enrol_inputs.windows(int(m)) for m in kept] and np.isfinite(emb).all()

        def invalid(*args, **kw):
            with pytest.raises(_lib.MmlaError) as e:
                c.si_enrol_embed(*args, **kw)
            assert e.value.code == -1, e.value

        too_long = np.zeros((1, _lib.ENROL_MAX_SAMPLES + 1), np.int16)
        invalid(too_long, passes=0, silence_remove=False)              # the length limit
        invalid(recs, lens=LENS, passes=0, vad_mode=4)                 # the detector's mode
        invalid(recs, lens=LENS, passes=-1, nonstationary=True)
        invalid(recs, lens=LENS, profile=[0, 0, 0])                    # still no bank
        # the existing calls keep their limit
        ref.vad_reset(1, 3)
        with pytest.raises(_lib.MmlaError) as e:
            ref.condition(np.zeros((1, 600001), np.int16), None, None, 0, True, 1)
        assert e.value.code == -1
        bare = _lib.Context(0)
        try:
            with pytest.raises(_lib.MmlaError) as e:       # no SI weights
                bare.si_enrol_embed(recs, lens=LENS, passes=0)
            assert e.value.code == -3, e.value
        finally:
            bare.close()
        # and the context still works: no gate, no silence removal -> the recordings themselves
        emb, nw, kept, pcm = c.si_enrol_embed(recs, lens=LENS, passes=0, silence_remove=False, return_pcm=True)
        assert kept.tolist() == LENS.tolist() and nw.tolist() == [2, 1, 0]
        assert pcm.tobytes() == cond_ref.zero_tails(np.array(recs), LENS).tobytes()
    finally:
        c.close()
        ref.close()
