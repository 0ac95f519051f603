"""GPU: the OD silence gate (mmla_od_pipeline_gated; record_on_pi.py:103-124) -- denoise the clip four
times through PCM_16, compare the feature images of the raw and the denoised clip (SSIM), call the
clip silent below 0.3, and run the network on the denoised image.

The fused call must be bit-identical to the composition of the public calls it fuses, and its
decisions must be those of the CPU oracles (oracle.noisereduce, oracle.od_fe, tests/ssim_ref.py).
Synthetic OD weights; the 12 clips of ssim_ref.gate_clips() (oracle.synth clips, the voiced ones
halved and mixed with noise of the profile's level; clip 11 is noise alone)."""
import numpy as np
import pytest

import ssim_ref
from mmla_audio_amd import _lib, weights

pytestmark = pytest.mark.gpu

CLIP = ssim_ref.GATE_CLIP
THRESHOLD = 0.3
# GPU - oracle SSIM difference on the 12 clips: the gate's and the front-end's few 1-LSB pixels (a
# float32 dB within rounding of a gate threshold or of a quantisation step).  Measured on an MI355X:
# 7.2e-7 at most (clips 4 and 7; 5e-8 or less on nine of the twelve); the tests assert 4 x that.
MEASURED_DIFF = 7.2e-7
ORACLE_BOUND = 4 * MEASURED_DIFF


def _new_ctx():
    c = _lib.Context(0)
    c.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=77)), 2)
    return c


@pytest.fixture(scope='module')
def ctx():
    c = _new_ctx()
    c.nr_set_noise(ssim_ref.gate_noise())
    return c


@pytest.fixture(scope='module')
def clips():
    x = ssim_ref.gate_clips()
    x.setflags(write=False)
    return x


@pytest.fixture(scope='module')
def fused(ctx, clips):
    """the gated call on the 12 clips with the reference's settings, shared read-only"""
    out = ctx.od_pipeline_gated(clips, passes=4, threshold=THRESHOLD)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope='module')
def oracle(clips):
    """SSIM of every clip by the CPU oracle composition (~0.1 s per clip)"""
    noise = ssim_ref.gate_noise()
    s = np.array([ssim_ref.oracle_gate(c, noise)[0] for c in clips])
    s.setflags(write=False)
    return s


def _zero_tails(q, lens):
    if lens is not None:
        for i, m in enumerate(lens):
            q[i, m:] = 0
    return q


def composed(ctx, pcm, lens=None, passes=4, threshold=THRESHOLD):
    """the gate from the public calls: od_features -> pcm / 32768 -> passes x (nr_reduce -> pcm16) ->
    od_features -> ssim_u8 -> od_forward_u8; with lens the clip is zero-extended and its tail zeroed"""
    feats = dict(db=False, norm=False, zcr=False)
    img_a = ctx.od_features(pcm, lens=lens, **feats)['img']
    q = _zero_tails(np.array(pcm, np.int16), lens)
    for _ in range(passes):
        y = q.astype(np.float32) / np.float32(32768.0)
        q = _zero_tails(ctx.pcm16(ctx.nr_reduce(y)), lens)
    img_b = ctx.od_features(q, lens=lens, **feats)['img']
    s = ctx.ssim_u8(img_a, img_b)
    probs = ctx.od_forward(img_b)
    n_samples = np.full(len(pcm), pcm.shape[1]) if lens is None else np.asarray(lens)
    silent = (n_samples < 4000) | (s < np.float32(threshold))
    am = np.where(silent, -1, (probs[:, 1] > probs[:, 0]).astype(np.int32)).astype(np.int32)
    return probs, am, silent, s


def _same(got, want):
    for g, w, name in zip(got, want, ('probs', 'argmax', 'silent', 'ssim')):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name


def test_fused_equals_composed_across_microbatches(ctx, clips, fused):
    ctx.set_microbatch(od=5)       # 12 clips: two micro-batch boundaries
    try:
        got = ctx.od_pipeline_gated(clips, passes=4, threshold=THRESHOLD)
        want = composed(ctx, clips)
    finally:
        ctx.set_microbatch(od=0)
    _same(got, want)
    _same(got, fused)              # ... and the micro-batch size does not enter the result
    assert got[2].any() and not got[2].all()


def test_fused_equals_composed_with_lens(ctx, clips):
    lens = np.full(12, CLIP, np.int32)
    lens[1] = 3999
    lens[5] = 12000
    ctx.set_microbatch(od=5)
    try:
        got = ctx.od_pipeline_gated(clips, lens=lens, passes=4, threshold=THRESHOLD)
        want = composed(ctx, clips, lens=lens)
    finally:
        ctx.set_microbatch(od=0)
    _same(got, want)
    assert got[2][1] and got[1][1] == -1       # 3999 samples: silent by the length rule


def test_device_pointers_equal_host_pointers(ctx, clips, fused):
    import torch
    lens = np.full(12, CLIP, np.int32)
    lens[1] = 3999
    lens[5] = 12000
    want = ctx.od_pipeline_gated(clips, lens=lens, passes=4, threshold=THRESHOLD)
    x = torch.from_numpy(clips.copy()).cuda()
    dl = torch.from_numpy(lens).cuda()
    probs = torch.zeros((12, 2), dtype=torch.float32, device='cuda')
    am = torch.zeros(12, dtype=torch.int32, device='cuda')
    silent = torch.zeros(12, dtype=torch.uint8, device='cuda')
    s = torch.zeros(12, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.od_pipeline_gated_dev(x.data_ptr(), 12, CLIP, CLIP, 4, THRESHOLD, probs.data_ptr(),
                              am.data_ptr(), silent.data_ptr(), s.data_ptr(), dl.data_ptr())
    ctx.synchronize()
    _same((probs.cpu().numpy(), am.cpu().numpy(), silent.cpu().numpy().astype(bool), s.cpu().numpy()),
          want)
    # without lens and without the ssim output (the similarity then lives in a workspace)
    ctx.od_pipeline_gated_dev(x.data_ptr(), 12, CLIP, CLIP, 4, THRESHOLD, probs.data_ptr(),
                              am.data_ptr(), silent.data_ptr())
    ctx.synchronize()
    _same((probs.cpu().numpy(), am.cpu().numpy(), silent.cpu().numpy().astype(bool)), fused[:3])


def test_zero_passes_is_od_pipeline(clips):
    c = _new_ctx()                  # no noise profile
    lens = np.full(12, CLIP, np.int32)
    lens[3] = 3999
    for ln in (None, lens):
        probs, am, silent, s = c.od_pipeline_gated(clips, lens=ln, passes=0, threshold=THRESHOLD)
        p0, a0, s0 = c.od_pipeline(clips, lens=ln)
        assert probs.tobytes() == p0.tobytes() and am.tobytes() == a0.tobytes()
        assert np.array_equal(silent, s0)
        assert np.array_equal(s, np.ones(12, np.float32))
    with pytest.raises(_lib.MmlaError) as e:
        c.od_pipeline_gated(clips, passes=4)
    assert e.value.code == -1
    with pytest.raises(_lib.MmlaError):
        c.od_pipeline_gated(clips, passes=-1)


def test_thresholds(ctx, clips, fused):
    lens = np.full(12, CLIP, np.int32)
    lens[0] = 3999
    _, am, silent, s = ctx.od_pipeline_gated(clips, lens=lens, passes=4, threshold=2.0)
    assert (am == -1).all() and silent.all()
    probs, am, silent, s = ctx.od_pipeline_gated(clips, lens=lens, passes=4, threshold=-2.0)
    assert np.array_equal(silent, lens < 4000)
    assert np.array_equal(am, np.where(lens < 4000, -1, probs[:, 1] > probs[:, 0]))
    assert np.array_equal(s[1:], fused[3][1:])


def test_decisions_match_cpu_oracle(fused, oracle):
    # a condition on the inputs: no clip sits near the threshold
    assert np.abs(oracle - THRESHOLD).min() >= 0.1, oracle
    probs, am, silent, s = fused
    diff = np.abs(s.astype(np.float64) - oracle)
    print('oracle ssim', oracle)
    print('gpu ssim   ', s)
    print('gpu - oracle', diff, 'max', diff.max())
    assert np.array_equal(silent, oracle < THRESHOLD)
    assert np.array_equal(am == -1, silent)
    assert silent[11] and silent[2] and not silent[0]     # noise alone is silent, speech is not
    assert oracle[8] == 1.0 and s[8] == 1.0               # digital zeros: two equal (NaN -> 0) images
    assert diff.max() <= ORACLE_BOUND, diff


def test_zeroed_tail_matters(ctx, clips):
    """a 12000-sample clip through the gated call (denoised zero-extended to 24000, the gate's leakage
    past the true end zeroed) decides as denoising exactly its 12000 samples does"""
    lens = np.array([12000], np.int32)
    probs, am, silent, s = ctx.od_pipeline_gated(clips[:1], lens=lens, passes=4, threshold=THRESHOLD)
    short = np.ascontiguousarray(clips[:1, :12000])
    _, am_s, silent_s, s_s = composed(ctx, short)
    print('gated', s, 'exactly 12000 samples', s_s, 'diff', abs(float(s[0]) - float(s_s[0])))
    assert silent[0] == silent_s[0] and am[0] == am_s[0]
    assert abs(float(s[0]) - float(s_s[0])) <= ORACLE_BOUND


def test_launch_plan_over_the_plain_pipeline(ctx, clips):
    """what the gate adds to od_pipeline's launches and algorithmic work on the same clips (no lens, D =
    min(clip_len, 24000) samples per clip): per pass one gate launch (8 n D) and one PCM_16 round trip (8 n
    D, the last one to int16: 6 n D) behind the float conversion (6 n D), then the second image (reads 2 D
    bytes, writes an image per clip) and the SSIM (reads two images, writes a float per clip); without a
    pass only the fill of the SSIM output with 1"""
    n, D, img = len(clips), min(CLIP, _lib.OD_CLIP), _lib.OD_MELS * _lib.OD_FRAMES * 3

    def profile(fn):
        ctx.profile_enable(True)
        try:
            ctx.profile_read(reset=True)
            fn()
            return {k: v[1:] for k, v in ctx.profile_read(reset=True).items()}
        finally:
            ctx.profile_enable(False)

    plain = profile(lambda: ctx.od_pipeline(clips))
    for p in (2, 0):
        gated = profile(lambda: ctx.od_pipeline_gated(clips, passes=p, threshold=THRESHOLD))
        delta = {k: (gated[k][0] - plain[k][0], gated[k][1] - plain[k][1]) for k in plain}
        print('passes', p, 'plain', plain, 'gated', gated)
        want = dict.fromkeys(plain, (0, 0))
        if p:
            want['nr'] = (p, 8 * n * D * p)
            want['glue'] = (1 + p, n * D * (8 * p + 4))
            want['od_fe'] = (2, n * (2 * D + img) + n * (2 * img + 4))
        else:
            want['glue'] = (1, 4 * n)
        assert delta == want, (p, delta)
