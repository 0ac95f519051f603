"""GPU: the PC loop's pre-conditioning as one batched call (mmla_condition, mmla_od_pipeline_conditioned,
mmla_si_pipeline_conditioned; record_on_pc.py save_wave_file(noise_reduce=True, silence_remove=True)):
every clip gated against its microphone's noise profile, written as PCM_16, its silence removed by its
stream's persistent detector, 'silent' below 4000 kept samples, then the network.

The fused calls must be bit-identical to the composition of the public calls they fuse
(cond_ref.composed_condition + od_pipeline / si_pipeline), whatever the micro-batch size, however the
clips are split over calls and whether a micro-batch was re-run; the silence removal must be the CPU
oracle's on the GPU's own denoised samples.  Synthetic weights (OD; SI with 8 sigmoid classes); the six
clips and three profiles of tests/cond_ref.py, as 3 streams x 2 clips with stream s on profile s."""
import numpy as np
import pytest

import cond_ref
from mmla_audio_amd import _lib, weights

pytestmark = pytest.mark.gpu

L = cond_ref.L
PROFILE = np.array([0, 0, 1, 1, 2, 2], np.int32)
LENS = np.array([L, 12000, L, 3999, L, L], np.int32)
SI_K = 8
NAMES = ('probs', 'argmax', 'silent', 'kept_len', 'out_pcm')


_OPEN = []      # contexts a test created: closed (their HIP stream destroyed) when the test ends


def _new_ctx(load=True):
    c = _lib.Context(0)
    _OPEN.append(c)
    if not load:
        return c
    c.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=81)), 2)
    c.load_weights(weights.SI, weights.pack(weights.SI, weights.synthetic(weights.SI, seed=82, n_classes=SI_K),
                                            SI_K), SI_K, _lib.HEAD_SIGMOID)
    return c


@pytest.fixture(autouse=True)
def _close_contexts():
    """every context owns a HIP stream: a test leaves none behind, whatever still refers to the object
    (a model and its context refer to each other), so the streams later test modules create are
    placed as if this module had not run"""
    yield
    while _OPEN:
        _OPEN.pop().close()


@pytest.fixture(scope='module')
def ctx():
    c = _new_ctx()
    _OPEN.remove(c)
    yield c
    c.close()


@pytest.fixture(scope='module')
def clips():
    x = cond_ref.clips()
    x.setflags(write=False)
    return x


@pytest.fixture(scope='module')
def noises():
    return [cond_ref.noise(p) for p in range(cond_ref.N_PROFILES)]


def _net(ctx, kind, q, kept):
    return (ctx.od_pipeline if kind == 'od' else ctx.si_pipeline)(q, lens=kept)


def composed(ctx, kind, x, noises, profile=PROFILE, lens=None, passes=1, silence_remove=True, ips=2):
    """the public-call chain -> (probs, argmax, silent, kept_len, out_pcm)"""
    q, kept = cond_ref.composed_condition(ctx, x, noises, profile, lens, passes, silence_remove, ips)
    return _net(ctx, kind, q, kept) + (kept, q)


def fused(ctx, kind, x, noises, profile=PROFILE, lens=None, passes=1, silence_remove=True, ips=2,
          streams=3):
    """the fused call on a fresh bank and (with silence removal) freshly reset detectors"""
    if passes > 0:
        ctx.nr_set_noise_bank(noises)
    if silence_remove:
        ctx.vad_reset(streams, 3)
    fn = ctx.od_pipeline_conditioned if kind == 'od' else ctx.si_pipeline_conditioned
    return fn(x, lens, profile, passes, silence_remove, ips, return_pcm=True)


def _same(got, want, what=''):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


@pytest.fixture(scope='module')
def reference(ctx, clips, noises):
    """the composed chain with lens, one pass, for both networks: computed once, shared read-only"""
    out = {k: composed(ctx, k, clips, noises, lens=LENS) for k in ('od', 'si')}
    for res in out.values():
        for a in res:
            a.setflags(write=False)
    return out


# ---- 3. fused equals composed ------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['od', 'si'])
def test_fused_equals_composed(ctx, clips, noises, reference, kind):
    want = reference[kind]
    got = fused(ctx, kind, clips, noises, lens=LENS)
    print(kind, 'kept', got[3], 'silent', got[2], 'argmax', got[1])
    _same(got, want, 'lens')
    probs, am, silent, kept, q = got
    assert silent.any() and not silent.all()
    assert np.array_equal(silent, kept < 4000) and np.array_equal(am == -1, silent)
    assert (kept % 480 == 0).all() and kept[3] == 0 and 0 < kept[1] <= 12000 - 480
    assert (kept >= L - 480).any() and ((kept > 0) & (kept < L - 4800)).any()
    for i in range(6):
        assert not q[i, kept[i]:].any()
    # the micro-batch size does not enter: 5 -> whole streams of 2 -> micro-batches of 4 + 2 clips
    ctx.set_microbatch(**{kind: 5})
    try:
        _same(fused(ctx, kind, clips, noises, lens=LENS), want, 'micro-batches')
    finally:
        ctx.set_microbatch()
    # without lens
    _same(fused(ctx, kind, clips, noises), composed(ctx, kind, clips, noises), 'no lens')


@pytest.mark.parametrize('kind', ['od', 'si'])
def test_three_passes(ctx, clips, noises, kind):
    """standardize_audio's three passes, across a micro-batch boundary"""
    want = composed(ctx, kind, clips, noises, lens=LENS, passes=3)
    ctx.set_microbatch(**{kind: 5})
    try:
        got = fused(ctx, kind, clips, noises, lens=LENS, passes=3)
    finally:
        ctx.set_microbatch()
    _same(got, want)
    assert got[2].any() and not got[2].all()


def test_condition_alone_equals_composed(ctx, clips, noises, reference):
    ctx.nr_set_noise_bank(noises)
    ctx.vad_reset(3, 3)
    q, kept = ctx.condition(clips, LENS, PROFILE, 1, True, 2)
    assert q.tobytes() == reference['od'][4].tobytes() and kept.tobytes() == reference['od'][3].tobytes()


# ---- 4. the detectors' state carries across calls -----------------------------------------------------

@pytest.mark.parametrize('kind', ['od', 'si'])
def test_state_carries_across_calls(ctx, clips, noises, reference, kind):
    """clips 0, 2, 4 then clips 1, 3, 5, one clip per stream and call = the six clips as 3 x 2"""
    want = reference[kind]
    ctx.nr_set_noise_bank(noises)
    ctx.vad_reset(3, 3)
    fn = ctx.od_pipeline_conditioned if kind == 'od' else ctx.si_pipeline_conditioned
    for first in (0, 1):
        idx = np.arange(first, 6, 2)
        got = fn(np.ascontiguousarray(clips[idx]), LENS[idx], PROFILE[idx], 1, True, 1, return_pcm=True)
        _same(got, tuple(w[idx] for w in want), f'call {first}')


# ---- 5. re-runs do not advance the detectors twice -----------------------------------------------------

def _debug_ctx(monkeypatch, name, value):
    monkeypatch.setenv(name, value)
    c = _new_ctx()
    monkeypatch.delenv(name)
    return c


def test_split_lstm_rerun_keeps_vad_state(monkeypatch, ctx, clips, noises):
    """MMLA_DEBUG_LSTM_SPIN=-1: the network of every micro-batch of a host call runs twice (the split
    BiLSTM gives up, the unsplit one repeats it) on the conditioning already made, which is not repeated:
    the detectors must have advanced once.  Two consecutive calls: the second shows the state left behind."""
    dbg = _debug_ctx(monkeypatch, 'MMLA_DEBUG_LSTM_SPIN', '-1')
    for c in (ctx, dbg):
        c.nr_set_noise_bank(noises)
        c.vad_reset(3, 3)
    dbg.set_microbatch(od=4, si=4)       # 4 + 2 clips: the second micro-batch's streams start at 2
    for kind in ('od', 'si'):
        for call in (0, 1):
            res = []
            for c in (ctx, dbg):
                fn = c.od_pipeline_conditioned if kind == 'od' else c.si_pipeline_conditioned
                res.append(fn(clips, LENS, PROFILE, 1, True, 2, return_pcm=True))
            _same(res[1], res[0], (kind, call))
    f32_reruns, split_reruns = dbg.debug_counters()
    assert f32_reruns == 0 and split_reruns >= 8, (f32_reruns, split_reruns)


def test_f32_rerun_of_a_conditioned_call(clips, noises):
    """OD weights whose block-4 BatchNorm drives its conv input past the fp16 range (the recipe of
    test_gpu_range_guard._hot_od): every micro-batch of a host call trips the range guard and is re-run
    in exact f32.  Every output of two consecutive calls (the second shows the state left behind) equals,
    byte for byte, a context with the same weights that runs exact f32 throughout."""
    W = weights.synthetic(weights.OD, seed=5)
    W['layer_with_weights-14/gamma'] = W['layer_with_weights-14/gamma'] * 2.0e5
    W['layer_with_weights-14/beta'] = np.abs(W['layer_with_weights-14/beta']) * 2.0e5
    hot, exact = _new_ctx(load=False), _new_ctx(load=False)
    for c in (hot, exact):
        c.load_weights(weights.OD, weights.pack(weights.OD, W), 2)
        c.nr_set_noise_bank(noises)
        c.vad_reset(3, 3)
        c.set_microbatch(od=4)           # 4 + 2 clips
    exact.set_precision(_lib.PREC_F32)
    for call in (0, 1):
        want = exact.od_pipeline_conditioned(clips, LENS, PROFILE, 1, True, 2, return_pcm=True)
        got = hot.od_pipeline_conditioned(clips, LENS, PROFILE, 1, True, 2, return_pcm=True)
        assert np.isfinite(got[0]).all()
        _same(got, want, call)
    print('debug counters: guarded', hot.debug_counters(), 'exact', exact.debug_counters())
    assert hot.debug_counters() == (4, 0)            # 2 calls x 2 micro-batches, no split re-run
    assert exact.debug_counters() == (0, 0)


def test_oom_retry_keeps_vad_state(monkeypatch, ctx, clips):
    """MMLA_DEBUG_FAIL_ALLOC=1 fails the context's first workspace allocation, which has to fall into
    the conditioned call for it to be retried (hence no noise gate here: building a bank allocates),
    and only a micro-batch of more than 64 clips is halved: 66 clips as 33 streams x 2 -> 64 + 2."""
    x = np.tile(clips, (11, 1))
    dbg = _debug_ctx(monkeypatch, 'MMLA_DEBUG_FAIL_ALLOC', '1')
    for c in (ctx, dbg):
        c.vad_reset(33, 3)
    for call in (0, 1):
        want = ctx.od_pipeline_conditioned(x, None, None, 0, True, 2, return_pcm=True)
        got = dbg.od_pipeline_conditioned(x, None, None, 0, True, 2, return_pcm=True)
        _same(got, want, call)
    assert want[2].any() and not want[2].all()


# ---- 6. off switches and misuse ------------------------------------------------------------------------

def test_off_switch_is_the_plain_pipeline(clips):
    c = _new_ctx()                   # no bank, no detectors
    for ln in (None, LENS):
        n_samples = np.full(6, L, np.int32) if ln is None else ln
        p0, a0, s0 = c.od_pipeline(clips, lens=ln)
        probs, am, silent, kept, q = c.od_pipeline_conditioned(clips, ln, None, 0, False, 1, return_pcm=True)
        assert probs.tobytes() == p0.tobytes() and am.tobytes() == a0.tobytes()
        assert np.array_equal(silent, s0) and np.array_equal(kept, n_samples)
        assert np.array_equal(q, cond_ref.zero_tails(np.array(clips), ln))
        p1, a1, s1 = c.si_pipeline(clips, lens=ln)
        probs, am, silent, kept = c.si_pipeline_conditioned(clips, ln, None, 0, False, 1)
        assert probs.tobytes() == p1.tobytes() and am.tobytes() == a1.tobytes()
        assert np.array_equal(silent, s1) and np.array_equal(kept, n_samples)
    assert s0[3] and a0[3] == -1


def test_gate_alone_and_silence_removal_alone(ctx, clips, noises):
    # the gate alone needs no detectors: a file of 3999 samples is 'silent' though not empty
    c = _new_ctx()
    want = composed(c, 'od', clips, noises, lens=LENS, silence_remove=False)
    got = fused(c, 'od', clips, noises, lens=LENS, silence_remove=False)
    _same(got, want)
    assert np.array_equal(got[3], LENS) and got[2][3] and got[1][3] == -1
    assert got[4][1, :12000].any() and not got[4][1, 12000:].any()
    assert list(got[2]) == [False, False, False, True, False, False]
    # silence removal alone needs no bank
    c = _new_ctx()
    want = composed(c, 'si', clips, noises, lens=LENS, passes=0)
    got = fused(c, 'si', clips, noises, lens=LENS, passes=0)
    _same(got, want)
    assert got[2].any() and not got[2].all()


def test_misuse_is_invalid(clips, noises):
    c = _new_ctx()

    def invalid(*args, **kw):
        with pytest.raises(_lib.MmlaError) as e:
            c.od_pipeline_conditioned(*args, **kw)
        assert e.value.code == -1, e.value
        with pytest.raises(_lib.MmlaError) as e:
            c.si_pipeline_conditioned(*args, **kw)
        assert e.value.code == -1, e.value
        with pytest.raises(_lib.MmlaError) as e:
            c.condition(*args, **kw)
        assert e.value.code == -1, e.value

    invalid(clips, None, None, 1, False, 1)          # the gate without a bank
    invalid(clips, None, None, 0, True, 1)           # silence removal without detectors
    c.nr_set_noise_bank(noises)
    c.vad_reset(3, 3)
    invalid(clips, None, None, -1, True, 2)          # nr_passes < 0
    invalid(clips, None, None, 1, True, 4)           # 6 clips are not whole streams of 4
    invalid(clips, None, None, 1, True, 3)           # ... and 2 streams are not the 3 created
    invalid(clips, None, None, 1, True, 0)
    invalid(clips, None, [0, 1, 2, 3, 0, 0], 1, True, 2)   # a host profile index outside the bank
    invalid(np.zeros((1, 600001), np.int16), None, None, 1, False, 1)   # more than one gate chunk
    c.od_pipeline_conditioned(clips, None, PROFILE, 1, True, 2)         # and the context still works


# ---- 7. device pointers ---------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['od', 'si'])
def test_device_pointers_equal_host_pointers(ctx, clips, noises, reference, kind):
    import torch
    k = 2 if kind == 'od' else SI_K
    x = torch.from_numpy(clips.copy()).cuda()
    dl = torch.from_numpy(LENS).cuda()
    dp = torch.from_numpy(PROFILE).cuda()
    probs = torch.zeros((6, k), dtype=torch.float32, device='cuda')
    am = torch.zeros(6, dtype=torch.int32, device='cuda')
    silent = torch.zeros(6, dtype=torch.uint8, device='cuda')
    q = torch.full((6, L), 7, dtype=torch.int16, device='cuda')
    kept = torch.zeros(6, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    fn = ctx.od_pipeline_conditioned_dev if kind == 'od' else ctx.si_pipeline_conditioned_dev
    ctx.nr_set_noise_bank(noises)

    def host(t):
        a = t.cpu().numpy()
        return a.astype(bool) if t is silent else a

    ctx.vad_reset(3, 3)
    fn(x.data_ptr(), 6, L, L, 1, True, 2, probs.data_ptr(), am.data_ptr(), silent.data_ptr(),
       q.data_ptr(), kept.data_ptr(), dl.data_ptr(), dp.data_ptr())
    ctx.synchronize()
    _same(tuple(host(t) for t in (probs, am, silent, kept, q)), reference[kind], 'all outputs')
    # out_pcm and kept_len null: the conditioned clips live in the workspace only
    for t in (probs, am, silent):
        t.zero_()
    torch.cuda.synchronize()
    ctx.vad_reset(3, 3)
    fn(x.data_ptr(), 6, L, L, 1, True, 2, probs.data_ptr(), am.data_ptr(), silent.data_ptr(),
       lens=dl.data_ptr(), profile=dp.data_ptr())
    ctx.synchronize()
    _same(tuple(host(t) for t in (probs, am, silent)), reference[kind][:3], 'no out_pcm / kept_len')


def test_condition_device_pointers(ctx, clips, noises, reference):
    import torch
    x = torch.from_numpy(clips.copy()).cuda()
    dl = torch.from_numpy(LENS).cuda()
    dp = torch.tensor([0, 0, 1, 1, 9, 2], dtype=torch.int32, device='cuda')   # 9: clamped to profile 2
    q = torch.full((6, L), 7, dtype=torch.int16, device='cuda')
    kept = torch.zeros(6, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.nr_set_noise_bank(noises)
    ctx.vad_reset(3, 3)
    ctx.condition_dev(x.data_ptr(), 6, L, L, 1, True, 2, q.data_ptr(), kept.data_ptr(), dl.data_ptr(),
                      dp.data_ptr())
    ctx.synchronize()
    assert q.cpu().numpy().tobytes() == reference['od'][4].tobytes()
    assert kept.cpu().numpy().tobytes() == reference['od'][3].tobytes()


# ---- 8. against the CPU oracle ---------------------------------------------------------------------------

def test_silence_removal_is_the_cpu_oracles(ctx, clips, noises, reference):
    """the GPU's own denoised int16 (public calls, no silence removal) through oracle.vad.remove_silence
    with one oracle.webrtc_vad.Vad(3) per stream reproduces the fused call's kept_len and out_pcm exactly.
    (The gate against oracle.noisereduce: test_gpu_noisereduce.py; the networks: the identity above.)"""
    from oracle import vad as ovad
    from oracle import webrtc_vad
    den, _ = cond_ref.composed_condition(ctx, clips, noises, PROFILE, LENS, 1, silence_remove=False)
    want_q = np.zeros_like(den)
    want_kept = np.zeros(6, np.int32)
    for s in range(3):
        det = webrtc_vad.Vad(3)
        for i in (2 * s, 2 * s + 1):
            o, _ = ovad.remove_silence(den[i, :LENS[i]], det.is_speech)
            want_q[i, :len(o)] = o
            want_kept[i] = len(o)
    _, _, _, kept, q = reference['od']
    print('oracle kept', want_kept, 'gpu kept', kept)
    assert np.array_equal(kept, want_kept) and np.array_equal(q, want_q)
    assert want_kept.max() >= L - 480 and (want_kept == 0).any()


# ---- 9. the model methods ----------------------------------------------------------------------------------

def test_model_methods(clips, noises):
    from mmla_audio_amd import models
    c = _new_ctx(load=False)
    od = models.OverlapDetectionModel(weights.synthetic(weights.OD, seed=81), device=c)
    si = models.SpeakerIdModel(weights.synthetic(weights.SI, seed=82, n_classes=SI_K), SI_K,
                               _lib.HEAD_SIGMOID, device=c)
    mic = PROFILE
    first = od.predict_wavs_conditioned(clips, noises, mic=mic, lens=LENS, items_per_stream=2)
    builds = c.nr_bank_builds
    assert builds == 1
    second = od.predict_wavs_conditioned(clips, noises, mic=mic, lens=LENS, items_per_stream=2)
    assert c.nr_bank_builds == builds, 'the bank is rebuilt only when a noise clip changes'
    print('kept, first call', first[3], 'second call', second[3])
    again = od.predict_wavs_conditioned(clips, noises, mic=mic, lens=LENS, items_per_stream=2,
                                        reset_vad=True)
    _same(again, first)
    # the default microphone of a clip is its stream
    c.vad_reset(3, 3)
    _same(od.predict_wavs_conditioned(clips, noises, lens=LENS, items_per_stream=2, reset_vad=True), first)
    assert c.nr_bank_builds == builds
    # ... and the Context calls give the same, the second on the state the first left behind
    c.vad_reset(3, 3)
    _same(c.od_pipeline_conditioned(clips, LENS, mic, 1, True, 2), first)
    _same(c.od_pipeline_conditioned(clips, LENS, mic, 1, True, 2), second)
    c.vad_reset(3, 3)
    want = c.si_pipeline_conditioned(clips, LENS, mic, 1, True, 2)
    _same(si.predict_wavs_conditioned(clips, noises, mic=mic, lens=LENS, items_per_stream=2), want)
    # a changed noise clip rebuilds the bank; one clip for all microphones is a bank of one
    od.predict_wavs_conditioned(clips, noises[1], items_per_stream=2, reset_vad=True)
    assert c.nr_bank_builds == builds + 1
