"""GPU non-stationary noise gate (nr.hip nr_ns_* kernels; mmla_nr_reduce_ns and MMLA_NR_NONSTATIONARY)
against its numpy / scipy restatement tests/nr_ns_ref.py (noisereduce 2.0.x SpectralGateNonStationary;
parity with the library itself is unpinned: it is not installed).

Bar of the parity cases: |got - want| <= 1e-6 x max|want| at EVERY sample.  The mask is a smooth
function of the spectrum (no threshold decisions that could flip), the internals are float64 on both
sides and the one float32 step is the output cast (2^-24 = 6e-8 of a sample), so 1e-6 leaves a factor
16 over what the arithmetic predicts.  Each case prints its measured maximum; on an MI355X it is 0 (equal
float32 outputs) on every 40 000-sample case and 8.9e-14 on the 620 000-sample signal.

Every context here is created by this module and never gets a noise bank: without the feature the fused
cases are MMLA_E_INVALID ("nr_passes > 0: mmla_nr_set_noise must be called first").
"""
import numpy as np
import pytest

import cond_ref
import nr_ns_ref as ref
from mmla_audio_amd import _lib, weights

pytestmark = pytest.mark.gpu

BAR = 1e-6
SI_K = 8
_OPEN = []      # contexts a test created: closed when the test ends


def _new_ctx(load=True):
    c = _lib.Context(0)
    _OPEN.append(c)
    if load:
        c.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=81)), 2)
        c.load_weights(weights.SI, weights.pack(weights.SI, weights.synthetic(weights.SI, seed=82,
                                                                              n_classes=SI_K), SI_K),
                       SI_K, _lib.HEAD_SIGMOID)
    return c


@pytest.fixture(autouse=True)
def _close_contexts():
    yield
    while _OPEN:
        _OPEN.pop().close()


def _module_ctx(load):
    c = _new_ctx(load)
    _OPEN.remove(c)
    return c


@pytest.fixture(scope='module')
def ctx():
    """the context of the fused calls and of the gate alone"""
    c = _module_ctx(True)
    yield c
    c.close()


@pytest.fixture(scope='module')
def comp():
    """a second context: the composition of public calls runs on its gate, detectors and networks"""
    c = _module_ctx(True)
    yield c
    c.close()


@pytest.fixture(scope='module')
def inputs():
    x = ref.named_inputs()
    for a in x.values():
        a.setflags(write=False)
    return x


@pytest.fixture(scope='module')
def want(inputs):
    """the restatement of every parity input, computed once and shared read-only"""
    out = {name: ref.reduce_noise(y) for name, y in inputs.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


def _close(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    peak = np.abs(want).max()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / peak
    print(f'{what}: max |got - want| / max |want| = {err:.3e}')
    assert np.isfinite(got).all() and err <= BAR, (what, err)


# ---- 1. parity with the restatement ----------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tone', 'speech', 'noise'] + [f'speech[:{n}]' for n in ref.PREFIXES] +
                         ['long'])
def test_matches_restatement(ctx, inputs, want, name):
    _close(ctx.nr_reduce_ns(inputs[name]), want[name], name)


def test_other_parameters(inputs):
    c = _new_ctx(load=False)
    c.nr_set_nonstationary(0.5, 1.5, 5.0)
    y = inputs['speech']
    w = ref.reduce_noise(y, 16000, 0.5, 1.5, 5.0)
    _close(c.nr_reduce_ns(y), w, 'speech (0.5 s, 1.5, 5)')
    assert np.abs(w - ref.reduce_noise(y)).max() > 1e-3 * np.abs(w).max()     # the parameters matter
    c.nr_set_nonstationary()
    assert np.array_equal(c.nr_reduce_ns(y), _new_ctx(load=False).nr_reduce_ns(y))


# ---- 2. stale scratch -----------------------------------------------------------------------------------

def test_frames_outside_the_launched_range_are_zero_not_scratch(inputs, want):
    """80 000-sample loud signals first: the scratch is full of nonzero spectra under another layout.
    Then signals whose frames are mostly all-zero windows, outside the launched range or inside it."""
    c = _new_ctx(load=False)
    rng = np.random.default_rng(17)
    c.nr_reduce_ns((0.5 * rng.standard_normal((4, 80000))).astype(np.float32))
    got = c.nr_reduce_ns(ref.stale_scratch_signals())
    for i in range(3):
        _close(got[i], want[f'stale{i}'], f'stale{i}')


# ---- 3. batching ------------------------------------------------------------------------------------------

def test_batched_rows_equal_single_calls(ctx, inputs):
    rows = np.stack([inputs['tone'], np.zeros(40000, np.float32), inputs['speech'], inputs['noise'],
                     inputs['stale2']])
    single = [ctx.nr_reduce_ns(y) for y in rows]
    assert not single[1].any() and all(s.any() for i, s in enumerate(single) if i != 1)
    for n in (1, 2, 5):
        batch = ctx.nr_reduce_ns(rows[:n])
        for i in range(n):
            assert batch[i].tobytes() == single[i].tobytes(), (n, i)
    back = ctx.nr_reduce_ns(rows[::-1].copy())            # a signal's result does not depend on its row
    for i in range(5):
        assert back[4 - i].tobytes() == single[i].tobytes(), i


# ---- 4. the drop-in function ------------------------------------------------------------------------------

def test_reduce_noise_nonstationary(inputs):
    from mmla_audio_amd import noisereduce as nr
    y2 = np.stack([inputs['speech'], inputs['tone']])
    both = nr.reduce_noise_nonstationary(y2, 16000)
    assert both.dtype == np.float32 and both.shape == y2.shape
    for ch in range(2):
        assert np.array_equal(both[ch], nr.reduce_noise_nonstationary(y2[ch], 16000))
    y64 = inputs['speech'].astype(np.float64)
    out = nr.reduce_noise_nonstationary(y64, 16000)
    assert out.dtype == np.float64 and np.array_equal(out, both[0].astype(np.float64))
    other = nr.reduce_noise_nonstationary(y2[0], 16000, time_constant_s=0.5, thresh_n_mult_nonstationary=1.5,
                                          sigmoid_slope_nonstationary=5)
    assert not np.array_equal(other, both[0])
    with pytest.raises(NotImplementedError):               # the dispatch of reduce_noise stays as it was
        nr.reduce_noise(y=y2[0], sr=16000, stationary=False)


# ---- 5. fused = composed, byte for byte --------------------------------------------------------------------

N = 5
CLIP_LENS = {40960: np.array([40960, 0, 479, 12000, 40960], np.int32),
             12000: np.array([12000, 0, 479, 12000, 12000], np.int32)}


@pytest.fixture(scope='module')
def clips():
    # voiced (full), digital zeros (lens 0), a burst in noise (479), voiced + noise tail (12 000), voiced with a gap (full)
    x = cond_ref.clips()[[0, 4, 2, 5, 1]]
    x.setflags(write=False)
    return x


def composed_condition(c, pcm, lens, passes, silence_remove):
    """mmla_condition(MMLA_NR_NONSTATIONARY) from the public calls: per pass pcm / 32768 in float32 ->
    nr_reduce_ns on the zero-extended clip -> pcm16 -> zeros from lens[c] on; then vad_remove_silence on
    freshly reset detectors, one stream per clip -> (int16 [n, L], kept_len [n])"""
    q = cond_ref.zero_tails(np.array(pcm, np.int16), lens)
    n, width = q.shape
    for _ in range(passes):
        y = q.astype(np.float32) / np.float32(32768.0)
        q = cond_ref.zero_tails(c.pcm16(c.nr_reduce_ns(y)), lens)
    if not silence_remove:
        return q, np.asarray(lens, np.int32).copy()
    c.vad_reset(n, 3)
    voiced, _ = c.vad_remove_silence(q, lens=lens, items_per_stream=1)
    out = np.zeros_like(q)
    kept = np.zeros(n, np.int32)
    for i, o in enumerate(voiced):
        out[i, :len(o)] = o
        kept[i] = len(o)
    return out, kept


CASES = [(40960, 1, True), (40960, 2, False), (12000, 2, True), (12000, 1, False)]


@pytest.fixture(scope='module')
def composed(comp, clips):
    """(q, kept) of every case by the composition, computed once"""
    out = {}
    for clip_len, passes, sr in CASES:
        q, kept = composed_condition(comp, clips[:, :clip_len], CLIP_LENS[clip_len], passes, sr)
        q.setflags(write=False)
        kept.setflags(write=False)
        out[clip_len, passes, sr] = (q, kept)
    return out


def _fused_condition(c, x, lens, passes, sr, **kw):
    if sr:
        c.vad_reset(len(x), 3)
    return c.condition(x, lens, None, passes, sr, 1, nonstationary=True, **kw)


@pytest.mark.parametrize('clip_len,passes,sr', CASES)
def test_condition_equals_composed(ctx, clips, composed, clip_len, passes, sr):
    x, lens = np.ascontiguousarray(clips[:, :clip_len]), CLIP_LENS[clip_len]
    wq, wk = composed[clip_len, passes, sr]
    q, kept = _fused_condition(ctx, x, lens, passes, sr)
    print('kept', kept)
    assert q.tobytes() == wq.tobytes() and kept.tobytes() == wk.tobytes()
    assert kept[1] == 0 and not q[1].any()
    if clip_len == 40960 or not sr:              # (short clips can lose everything to the silence removal)
        assert q[0].any() and q[4].any() and kept[0] > 0 and kept[4] > 0
    assert wq.tobytes() != cond_ref.zero_tails(x.copy(), lens).tobytes()          # the gate did something
    ctx.set_microbatch(od=2)                     # micro-batches of 2 clips: 2 + 2 + 1
    try:
        q, kept = _fused_condition(ctx, x, lens, passes, sr)
    finally:
        ctx.set_microbatch()
    assert q.tobytes() == wq.tobytes() and kept.tobytes() == wk.tobytes()


def test_condition_device_pointers(ctx, clips, composed):
    import torch
    clip_len, passes, sr = CASES[0]
    wq, wk = composed[clip_len, passes, sr]
    x = torch.from_numpy(np.ascontiguousarray(clips[:, :clip_len])).cuda()
    dl = torch.from_numpy(CLIP_LENS[clip_len]).cuda()
    q = torch.full((N, clip_len), 7, dtype=torch.int16, device='cuda')
    kept = torch.zeros(N, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.vad_reset(N, 3)
    ctx.condition_dev(x.data_ptr(), N, clip_len, clip_len, passes, sr, 1, q.data_ptr(), kept.data_ptr(),
                      dl.data_ptr(), nonstationary=True)
    ctx.synchronize()
    assert q.cpu().numpy().tobytes() == wq.tobytes() and kept.cpu().numpy().tobytes() == wk.tobytes()


@pytest.mark.parametrize('clip_len,passes,sr', [CASES[0], CASES[2]])
def test_pipelines_equal_plain_pipelines_on_composed_clips(ctx, comp, clips, composed, clip_len, passes, sr):
    x, lens = np.ascontiguousarray(clips[:, :clip_len]), CLIP_LENS[clip_len]
    wq, wk = composed[clip_len, passes, sr]
    od = comp.od_pipeline(wq, lens=wk)
    si = comp.si_pipeline(wq, lens=wk)

    def same(got, net, what):
        for g, w, name in zip(got, net + (wk,), ('probs', 'argmax', 'silent', 'kept_len')):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, name)

    ctx.vad_reset(N, 3)
    got = ctx.od_pipeline_conditioned(x, lens, None, passes, sr, 1, nonstationary=True)
    same(got, od, 'od')
    assert got[2][1] and got[1][1] == -1 and not got[2].all()      # lens = 0: silent, argmax -1
    ctx.vad_reset(N, 3)
    got = ctx.si_pipeline_conditioned(x, lens, None, passes, sr, 1, nonstationary=True)
    same(got, si, 'si')
    assert got[2][1] and got[1][1] == -1
    ctx.vad_reset(N, 3)
    op, oa, sp, sa, silent, kept, q = ctx.room_pipeline_conditioned(x, lens, None, passes, sr, 1,
                                                                    return_pcm=True, nonstationary=True)
    same((op, oa, silent, kept), od, 'room od')
    same((sp, sa, silent, kept), (si[0], si[1], od[2]), 'room si')
    assert q.tobytes() == wq.tobytes() and oa[1] == -1 and sa[1] == -1


def test_allocation_failure_rerun_gives_the_same_bytes(monkeypatch, ctx, clips):
    """MMLA_DEBUG_FAIL_ALLOC=1 fails the context's first workspace allocation, which falls into the
    conditioned call (no bank was built); only a micro-batch of more than 64 clips is halved: 65 clips
    -> 64 + 1, the detectors restored for the re-run"""
    x = np.ascontiguousarray(np.tile(clips[:, :12000], (13, 1)))
    lens = np.tile(CLIP_LENS[12000], 13)
    monkeypatch.setenv('MMLA_DEBUG_FAIL_ALLOC', '1')
    dbg = _new_ctx()
    monkeypatch.delenv('MMLA_DEBUG_FAIL_ALLOC')
    res = []
    for c in (ctx, dbg):
        c.vad_reset(65, 3)
        res.append(c.od_pipeline_conditioned(x, lens, None, 1, True, 1, return_pcm=True, nonstationary=True))
    for g, w in zip(res[1], res[0]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert res[0][2].any() and not res[0][2].all()


# ---- 6. the edge loop's denoise-and-compare gate --------------------------------------------------------

def test_od_pipeline_gated(ctx, comp, clips):
    x, lens, passes, thr = np.ascontiguousarray(clips[[0, 2, 4], :24000]), np.array([24000, 9000, 24000], np.int32), 2, 0.3
    feats = dict(db=False, norm=False, zcr=False)
    img_a = comp.od_features(x, lens=lens, **feats)['img']
    q = cond_ref.zero_tails(x.copy(), lens)
    for _ in range(passes):
        q = cond_ref.zero_tails(comp.pcm16(comp.nr_reduce_ns(q.astype(np.float32) / np.float32(32768.0))), lens)
    img_b = comp.od_features(q, lens=lens, **feats)['img']
    s = comp.ssim_u8(img_a, img_b)
    probs = comp.od_forward(img_b)
    silent = (lens < 4000) | (s < np.float32(thr))
    am = np.where(silent, -1, (probs[:, 1] > probs[:, 0]).astype(np.int32)).astype(np.int32)
    got = ctx.od_pipeline_gated(x, lens, passes, thr, nonstationary=True)
    print('ssim', got[3])
    for g, w, name in zip(got, (probs, am, silent, s), ('probs', 'argmax', 'silent', 'ssim')):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    assert (s < 1).all()


# ---- 7. the flag is needed; arguments ----------------------------------------------------------------------

def test_without_the_flag_a_bankless_context_is_invalid(clips):
    c = _new_ctx()
    x, lens = np.ascontiguousarray(clips[:, :12000]), CLIP_LENS[12000]
    for fn in (c.condition, c.od_pipeline_conditioned, c.si_pipeline_conditioned, c.room_pipeline_conditioned):
        with pytest.raises(_lib.MmlaError) as e:
            fn(x, lens, None, 1, False, 1)
        assert e.value.code == -1, e.value
        fn(x, lens, None, 1, False, 1, nonstationary=True)
    with pytest.raises(_lib.MmlaError) as e:
        c.od_pipeline_gated(x, lens, 1, 0.3)
    assert e.value.code == -1, e.value
    with pytest.raises(_lib.MmlaError) as e:
        c.nr_reduce(np.zeros(1000, np.float32))
    assert e.value.code == -1, e.value


def test_set_nonstationary_arguments():
    c = _new_ctx(load=False)
    for args in ((0.0, 2.0, 10.0), (-1.0, 2.0, 10.0), (float('nan'), 2.0, 10.0), (float('inf'), 2.0, 10.0),
                 (2.0, 2.0, 0.0), (2.0, 2.0, -10.0), (2.0, 2.0, float('nan')), (2.0, float('nan'), 10.0)):
        with pytest.raises(_lib.MmlaError) as e:
            c.nr_set_nonstationary(*args)
        assert e.value.code == -1, (args, e.value)
    with pytest.raises(_lib.MmlaError) as e:
        c.nr_set_nonstationary(2.0, 2.0, 10.0, sr=8000)       # its smoothing filter is not 33 x 7
    assert e.value.code == -1, e.value
    c.nr_set_nonstationary(2.0, 2.0, 10.0, sr=15500)          # 33 x 7 too ...
    c.nr_set_nonstationary()
    c.nr_set_noise(np.ones(2000, np.float32))
    with pytest.raises(_lib.MmlaError) as e:                  # ... but not the sr of the bank held now
        c.nr_set_nonstationary(2.0, 2.0, 10.0, sr=15500)
    assert e.value.code == -1, e.value
    c.nr_set_nonstationary(1.0, 2.0, 10.0, sr=16000)


def test_room_without_noise_recordings(comp, clips):
    from mmla_audio_amd import models
    from mmla_audio_amd.room import Room
    c = _new_ctx(load=False)
    od = models.OverlapDetectionModel(weights.synthetic(weights.OD, seed=81), device=c)
    si = models.SpeakerIdModel(weights.synthetic(weights.SI, seed=82, n_classes=SI_K), SI_K,
                               _lib.HEAD_SIGMOID, device=c)
    x = np.ascontiguousarray(clips[[0, 4]])
    res = Room(od, si, None).tick(x, return_pcm=True)
    comp.vad_reset(2, 3)
    want = comp.room_pipeline_conditioned(x, None, None, 1, True, 1, return_pcm=True, nonstationary=True)
    for g, w, name in zip(res, want, res._fields):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    assert not hasattr(c, 'nr_bank_builds')                   # no bank was built
    with pytest.raises(ValueError):
        Room(od, si, None).tick(x, mic=np.zeros(3, np.int32))
    p = od.predict_wavs_conditioned(x, None, reset_vad=True)
    assert p[0].tobytes() == want[0].tobytes() and p[3].tobytes() == want[5].tobytes()
    g = od.predict_wavs_gated(x[:, :24000], None, passes=1)
    assert g[0].shape == (2, 2) and (g[3] < 1).all()
