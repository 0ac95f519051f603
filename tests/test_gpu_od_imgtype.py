"""GPU: the gray and viridis feature images (od_fe.hip's colour-map epilogues) and the one-channel OD network,
through every layer -- the front-end entries, the pipelines, loading, forward, training and the Python surface.
Inputs and rules: tests/od_imgtype_cases.py; their conditions are asserted on the CPU in
tests/test_od_imgtype_cpu.py.

No bound is new.  The image is exact: the rule of od_imgtype_cases (``plt.imsave``'s, checked against matplotlib
on the CPU) applied to the norm the same call returns.  Against the float64 oracle the index may differ by
one on at most oracle/compare.py's od_lsb_budget share of the pixels, the bar the ZCR image is held to.  The
one-channel forward is held to LOGP_TOL and the argmax rule like every other forward, its stem alone to the
float32 rounding of one product and one sum, losses / gradients / history to the d32 rule and fitted weights to
the update rule of tests/od_finetune_cases.py.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import od_finetune_cases as C
import od_finetune_ref as ref
import od_imgtype_cases as T
from mmla_audio_amd import _lib, models, overlap_detector, room, tfbundle, weights
from mmla_audio_amd.overlap_features_generator import OverlapFeaturesGenerator
from oracle import compare, nets

pytestmark = pytest.mark.gpu

OD = weights.OD
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM = 'layer_with_weights-0'
E_NOWEIGHTS = -3     # MMLA_E_NOWEIGHTS (include/mmla.h)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def feats(ctx):
    """every output of the int16 entry for each new type, on the 32 clips"""
    pcm, lens = T.clips()
    out = {name: ctx.od_features(pcm, lens, image_type=name) for name in T.TYPES}
    for f in out.values():
        for v in f.values():
            v.setflags(write=False)
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the exact rule ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', T.TYPES)
def test_image_is_the_rule_applied_to_the_norm_of_the_same_call(ctx, feats, name):
    pcm, lens = T.clips()
    f = feats[name]
    assert f['img'].shape == (T.N_CLIPS, 128, 151, 3) and f['img'].dtype == np.uint8
    assert np.array_equal(f['img'], T.rule(f['norm'], name))
    nan = np.isnan(f['norm']).all(axis=(1, 2))
    assert np.array_equal(nan, np.isnan(f['norm']).any(axis=(1, 2)))      # a clip is all NaN or not at all
    assert nan.any() and not f['img'][nan].any()                           # digital silence -> (0, 0, 0)
    assert (lens[nan] > 0).any() and (~nan).sum() >= 20                    # digital zeros, not only empty clips
    idx = T.index(f['norm'][~nan])
    assert idx.min() == 0 and idx.max() == 255                             # the clip's min and max: no autoscale
    if name == 'gray':
        assert (f['img'][..., 0] == f['img'][..., 1]).all() and (f['img'][..., 1] == f['img'][..., 2]).all()
    # the float entry (librosa.load's scale: x / 32768 is exact)
    g = ctx.od_features(pcm.astype(np.float32) / np.float32(32768.0), lens, db=False, zcr=False, image_type=name)
    assert np.array_equal(g['img'], T.rule(g['norm'], name))
    assert _same_bits(g['img'], f['img'])
    # the strided entry: overlapping windows of one signal, int16 and float
    sig = pcm[6]
    for s in (sig, sig.astype(np.float32) / np.float32(32768.0)):
        w = ctx.od_features_strided(s, 3, 8000, 24000, db=False, zcr=False, image_type=name)
        assert np.array_equal(w['img'], T.rule(w['norm'], name)) and w['img'].any()
    # without the norm output (another instantiation of the kernel) the same bytes
    only = ctx.od_features(pcm[:6], lens[:6], db=False, norm=False, zcr=False, image_type=name)
    assert list(only) == ['img'] and _same_bits(only['img'], f['img'][:6])


@pytest.mark.parametrize('name', T.TYPES)
def test_device_pointer_entry_writes_the_same_image(ctx, feats, name):
    import torch
    pcm, lens = T.clips()
    n = 6
    dp = torch.from_numpy(pcm[:n].copy()).cuda()
    dl = torch.from_numpy(lens[:n].copy()).cuda()
    img = torch.zeros((n, 128, 151, 3), dtype=torch.uint8, device='cuda')
    norm = torch.zeros((n, 128, 151), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.od_features_dev(dp.data_ptr(), n, pcm.shape[1], pcm.shape[1], norm=norm.data_ptr(), img=img.data_ptr(),
                        lens=dl.data_ptr(), image_type=name)
    ctx.synchronize()
    assert _same_bits(img.cpu().numpy(), feats[name]['img'][:n])
    assert _same_bits(norm.cpu().numpy(), feats[name]['norm'][:n])


def test_png_files_decode_to_imsave_pixels_with_alpha(ctx, tmp_path):
    """generate_gary_image / generate_viridis_image / generate_images: RGBA of the rule, alpha 0 for a silent clip"""
    import scipy.io.wavfile as wavfile

    from mmla_audio_amd.tf_compat import image as tfimage
    pcm, lens = T.clips()
    ofg = OverlapFeaturesGenerator(wl=25, hl=10, device=0)      # the process's default context of device 0
    for tag, i in (('live', 6), ('zeros', 18)):
        wav = str(tmp_path / f'{tag}.wav')
        wavfile.write(wav, 16000, pcm[i, :lens[i]])
        norm = ctx.od_features(pcm[i:i + 1], lens[i:i + 1], db=False, zcr=False, img=False)['norm'][0]
        out = str(tmp_path / tag) + os.sep
        ofg.generate_gary_image(wav, out, 'g.png')
        ofg.generate_viridis_image(wav, out, 'v.png')
        for fname, name in (('g.png', 'gray'), ('v.png', 'viridis')):
            with open(out + fname, 'rb') as fh:
                rgba = tfimage.decode_png(fh.read(), 4).numpy()
            assert rgba.shape == (128, 151, 4)
            assert np.array_equal(rgba[..., :3], T.rule(norm, name)), (tag, name)
            assert (rgba[..., 3] == (0 if tag == 'zeros' else 255)).all(), (tag, name)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        ofg.generate_images(str(tmp_path / 'live.wav'), 'x.png')
    finally:
        os.chdir(cwd)
    for d in ('mel_spectrum_viridis', 'mel_spectrum_gray', 'mel_spectrum_zcr'):
        assert (tmp_path / d / 'x.png').stat().st_size > 0
    assert (tmp_path / 'mel_spectrum_gray' / 'x.png').read_bytes() == (tmp_path / 'live' / 'g.png').read_bytes()


# ---- 2. against the oracle -----------------------------------------------------------------------------------

def test_index_against_the_float64_oracle_within_the_lsb_budget(feats):
    want = T.index(T.oracle_norms())
    got = T.index(feats['gray']['norm'])
    assert np.array_equal(got < 0, want < 0)                # the same clips are NaN
    assert _same_bits(feats['gray']['norm'], feats['viridis']['norm'])
    d = np.abs(got - want)
    off, tot, live = int(np.count_nonzero(d)), d.size, int((want >= 0).sum())
    print(f'index off by one on {off} of {tot} pixels: share {off / tot:.3e} ({off / max(live, 1):.3e} of the '
          f'{live} live ones); budget 1e-4')
    assert d.max() <= 1
    compare.od_lsb_budget([(off, tot)])
    for name in T.TYPES:                                    # the images differ from the oracle's only there
        ref_img = T.rule(T.oracle_norms(), name)
        diff = (feats[name]['img'] != ref_img).any(axis=-1)
        assert not (diff & (np.flip(d, axis=-2) == 0)).any()


# ---- 3. ZCR unchanged ----------------------------------------------------------------------------------------

def test_no_type_is_an_explicit_zcr_request_bit_for_bit(ctx):
    pcm, lens = T.clips()
    a = ctx.od_features(pcm, lens)
    b = ctx.od_features(pcm, lens, image_type='zcr')
    for k in ('db', 'norm', 'zcr', 'img'):
        assert _same_bits(a[k], b[k]), k
    assert not _same_bits(a['img'], ctx.od_features(pcm, lens, db=False, norm=False, zcr=False,
                                                    image_type='gray')['img'])
    # both flag bits: no type
    img = np.zeros((1, 128, 151, 3), np.uint8)
    p = np.ascontiguousarray(pcm[:1])
    rc = ctx.lib.mmla_od_features(ctx.h, p.ctypes.data, 1, p.shape[1], None, p.shape[1], None, None, None,
                                  img.ctypes.data, 3 << 4)
    assert rc == _lib.MMLA_E_INVALID
    with pytest.raises(ValueError):
        ctx.od_features(pcm[:1], image_type='grey')


# ---- 4. the one-channel forward ------------------------------------------------------------------------------

FE_CLIPS = (2, 6, 11)      # live clips of 24000 / 24000 / 40000 samples


def _forward_inputs(feats):
    """5 images uint8 [5,128,151,1]: channel 0 of three front-end gray images, two random ones"""
    x = np.concatenate([feats['gray']['img'][list(FE_CLIPS)][..., :1], T.forward_random(2)])
    assert x.shape == (5, 128, 151, 1) and x[:3].any()
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def _forward_want(key):
    x = np.frombuffer(key, np.uint8).reshape(5, 128, 151, 1)
    W = T.synthetic1(T.FWD_SEED)
    want = nets.od_forward(x.astype(np.float32), W)
    stem = nets.conv2d(x.astype(np.float64), W[STEM + '/kernel'].astype(np.float64),
                       W[STEM + '/bias'].astype(np.float64))
    return want, stem


def _check_forward(p, x8, tag):
    want, _ = _forward_want(x8.tobytes())
    assert p.shape == (5, 2) and p.dtype == np.float32
    err = compare.logp_err(p, want)
    print(tag, 'max |log p - log p_ref|', err)
    assert err <= compare.LOGP_TOL, tag
    assert compare.argmax_ok(p, want), tag


def test_one_channel_forward_vs_oracle_in_both_arithmetics(ctx, feats):
    W = T.synthetic1(T.FWD_SEED)
    x8 = _forward_inputs(feats)
    ctx.load_weights(OD, T.pack1(W), 2)
    assert ctx.od_channels == 1 and ctx.od_image_type == _lib.OD_IMG_GRAY
    try:
        ctx.set_microbatch(od=2)                                   # 2 + 2 + 1
        for prec, tag in ((_lib.PREC_F16X3, 'f16x3'), (_lib.PREC_F32, 'f32')):
            ctx.set_precision(prec)
            p = ctx.od_forward(x8.astype(np.float32))
            _check_forward(p, x8, tag)
            assert _same_bits(ctx.od_forward(x8), p), tag        # the u8 entry
        ctx.set_microbatch(0, 0)
        assert _same_bits(ctx.od_forward(x8), p)                   # one micro-batch: the same rows
        # the stem alone: one float32 product and one sum per output
        got = ctx.debug_od_trace(x8.astype(np.float32), 0)
        _, stem = _forward_want(x8.tobytes())
        k, b = W[STEM + '/kernel'].astype(np.float64)[0, 0, 0], W[STEM + '/bias'].astype(np.float64)
        bound = 2.0 ** -23 * (x8.astype(np.float64) * np.abs(k) + np.abs(b))
        err = np.abs(got.astype(np.float64) - stem)
        print('stem max err', err.max(), 'max bound', bound.max())
        assert got.shape == (5, 128, 151, 16) and (err <= bound).all()
    finally:
        ctx.set_precision(_lib.PREC_F16X3)
        ctx.set_microbatch(0, 0)


_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mmla_audio_amd import _lib, weights
z = np.load(sys.argv[2])
c = _lib.Context(0)
c.load_weights(weights.OD, z['blob'], 2)
c.set_microbatch(od=2)
out = {}
for prec, tag in ((_lib.PREC_F16X3, 'f16x3'), (_lib.PREC_F32, 'f32')):
    c.set_precision(prec)
    out[tag] = c.od_forward(z['x'].astype(np.float32))
    out[tag + '_u8'] = c.od_forward(z['x'])
np.savez(sys.argv[3], **out)
c.close()
'''


def test_one_channel_forward_on_the_tile_kernels_in_a_child_process(feats, tmp_path):
    x8 = _forward_inputs(feats)
    src, dst = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
    np.savez(src, blob=T.pack1(T.synthetic1(T.FWD_SEED)), x=x8)
    r = subprocess.run([sys.executable, '-c', _CHILD, REPO, src, dst], env=dict(os.environ, MMLA_RB_TILE='1'),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(dst)
    for tag in ('f16x3', 'f32'):
        _check_forward(z[tag], x8, 'tile ' + tag)
        assert _same_bits(z[tag + '_u8'], z[tag])


# ---- 5. pipelines ----------------------------------------------------------------------------------------------

def _live_clips(n=6):
    pcm, lens = T.clips()
    keep = [i for i in range(T.N_CLIPS) if lens[i] >= 24000][:n]
    return np.ascontiguousarray(pcm[keep]), np.ascontiguousarray(lens[keep])


CONFIGS = [(3, 'gray'), (3, 'viridis'), (1, 'gray')]


@pytest.mark.parametrize('ch,name', CONFIGS)
def test_pipelines_make_the_models_image_type(ctx, ch, name):
    W = weights.synthetic(OD, seed=9, channels=ch)
    od = models.OverlapDetectionModel(W, device=ctx, image_type=name)
    assert (od.channels, od.image_type) == (ch, name) and ctx.od_image_type == _lib.OD_IMAGE_TYPES[name]
    pcm, lens = _live_clips()
    probs, am, silent = od.predict_wavs(pcm, lens)
    img = ctx.od_features(pcm, lens, db=False, norm=False, zcr=False, image_type=name)['img']
    x = np.ascontiguousarray(img[..., :ch])
    fwd = od.predict(x)
    assert probs.shape == (len(pcm), 2) and _same_bits(fwd, probs)
    assert np.array_equal(am, probs.argmax(axis=1)) and not silent.any()
    if ch == 3:     # the type matters: the ZCR image gives other probabilities
        zcr = ctx.od_forward(ctx.od_features(pcm, lens, db=False, norm=False, zcr=False)['img'])
        assert not _same_bits(zcr, probs)
    # the strided and device-pointer pipelines and a split into micro-batches follow
    try:
        ctx.set_microbatch(od=4)
        assert _same_bits(ctx.od_pipeline(pcm, lens)[0], probs)
    finally:
        ctx.set_microbatch(0, 0)
    # Room.tick: the same probabilities behind a conditioning that changes nothing
    Wsi = weights.synthetic(weights.SI, seed=2, n_classes=4)
    si = models.SpeakerIdModel(Wsi, 4, _lib.HEAD_SIGMOID, device=ctx)
    r = room.Room(od, si)
    res = r.tick(pcm[:, :24000], passes=0, silence_remove=False)
    whole = od.predict_wavs(pcm[:, :24000])
    assert _same_bits(res.od_probs, whole[0]) and np.array_equal(res.od_argmax, whole[1])
    # predict_mixed: one-layer mixes are the clips themselves
    plan = _lib.MixPlan.from_layers([[(i * 24000, 24000, 0)] for i in range(len(pcm))])
    mixed = od.predict_mixed(np.ascontiguousarray(pcm[:, :24000]).reshape(-1), plan)
    assert _same_bits(mixed[0], whole[0]) and np.array_equal(mixed[1], whole[1])
    # the type set behind the model's back is put right by the next call
    if ch == 3:
        ctx.od_set_image_type('zcr')
        assert _same_bits(od.predict_wavs(pcm, lens)[0], probs)


@pytest.mark.parametrize('ch,name', CONFIGS)
def test_post_processing_of_a_multi_channel_file_follows_the_models_type(ctx, ch, name):
    """predict_frames / _window_images (post_anlysing) on a stereo conversation = the mono pipeline on its
    channel mean: with both channels equal the mean is the int16 signal / 32768, exactly"""
    from mmla_audio_amd import overlap_detection_post_processing as pp
    od = models.OverlapDetectionModel(weights.synthetic(OD, seed=9, channels=ch), device=ctx, image_type=name)
    pcm, _ = T.clips()
    mono = np.ascontiguousarray(np.concatenate([pcm[6, :24000], pcm[11, :36000]]))      # 2.5 windows of 1.5 s
    stereo = np.ascontiguousarray(np.repeat(mono, 2))                                   # interleaved L = R
    want = pp.predict_frames(mono, 1, od)
    got = pp.predict_frames(stereo, 2, od)
    assert want[0].shape == (len(want[1]), 2) and len(want[1]) >= 2
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    win, step, n = pp.segment_bounds(mono.size, 16000, 1.5, 1.5)
    for x, nch in ((mono, 1), (stereo, 2)):
        images, probs = pp._window_images(x, nch, od, 16000, 1.5, 1.5)
        ref = ctx.od_features_strided(mono, n, step, win, db=False, norm=False, zcr=False, image_type=name)['img']
        assert _same_bits(images, ref) and _same_bits(probs, want[0])
    if ch == 3:     # not the ZCR image's probabilities
        zcr = ctx.od_forward(ctx.od_features_strided(mono, n, step, win, db=False, norm=False, zcr=False)['img'])
        assert not _same_bits(zcr, want[0])


# ---- 6. loading and errors -----------------------------------------------------------------------------------

def _od_image(c):
    t, ch = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = c.lib.mmla_od_image(c.h, t.ctypes.data, ch.ctypes.data)
    return rc, int(t[0]), int(ch[0])


def test_loading_three_one_three_channels_gives_each_models_bits_and_resets_the_type(ctx, feats):
    W3, W1 = weights.synthetic(OD, seed=9), T.synthetic1(T.FWD_SEED)
    b3, b1 = weights.pack(OD, W3), T.pack1(W1)
    x1 = _forward_inputs(feats)[:2]
    x3 = np.ascontiguousarray(np.repeat(x1, 3, axis=3))
    ctx.load_weights(OD, b3, 2)
    assert _od_image(ctx) == (0, _lib.OD_IMG_ZCR, 3)
    p3 = ctx.od_forward(x3)
    ctx.od_set_image_type('viridis')
    assert _od_image(ctx) == (0, _lib.OD_IMG_VIRIDIS, 3)
    ctx.load_weights(OD, b1, 2)
    assert _od_image(ctx) == (0, _lib.OD_IMG_GRAY, 1) and ctx.od_channels == 1
    p1 = ctx.od_forward(x1)
    for t in ('viridis', 'zcr'):
        with pytest.raises(_lib.MmlaError) as e:
            ctx.od_set_image_type(t)
        assert e.value.code == _lib.MMLA_E_INVALID
    ctx.od_set_image_type('gray')
    assert ctx.lib.mmla_od_set_image_type(ctx.h, 3) == _lib.MMLA_E_INVALID
    ctx.load_weights(OD, b3, 2)
    assert _od_image(ctx) == (0, _lib.OD_IMG_ZCR, 3)             # reset, not the viridis set before
    assert _same_bits(ctx.od_forward(x3), p3)
    ctx.load_weights(OD, b1, 2)
    assert _same_bits(ctx.od_forward(x1), p1)
    assert not _same_bits(p1, p3)
    # the one-channel model on (g, g, g) is the three-channel model whose stem rows 1 and 2 are zero
    Wz = dict(W1)
    k = np.zeros((1, 1, 3, 16), np.float32)
    k[0, 0, 0] = W1[STEM + '/kernel'][0, 0, 0]
    Wz[STEM + '/kernel'] = k
    ctx.load_weights(OD, weights.pack(OD, Wz), 2)
    assert _same_bits(ctx.od_forward(x3), p1)


def test_errors(ctx, feats):
    fresh = _lib.Context(0)
    try:
        assert fresh.lib.mmla_od_set_image_type(fresh.h, 1) == E_NOWEIGHTS
        assert _od_image(fresh)[0] == E_NOWEIGHTS
    finally:
        fresh.close()
    pcm, lens = _live_clips(2)
    od1 = models.OverlapDetectionModel(T.synthetic1(T.FWD_SEED), device=ctx)
    assert od1.channels == 1 and od1.image_type == 'gray'
    with pytest.raises(ValueError, match=r'\[N,128,151,1\]'):
        od1.predict(np.zeros((2, 128, 151, 3), np.uint8))
    with pytest.raises(ValueError):
        models.OverlapDetectionModel(T.synthetic1(T.FWD_SEED), device=ctx, image_type='viridis')
    with pytest.raises(_lib.MmlaError) as e:
        od1.predict_wavs_gated(pcm, None, lens, passes=0)
    assert e.value.code == _lib.MMLA_E_INVALID
    si = models.SpeakerIdModel(weights.synthetic(weights.SI, seed=2, n_classes=4), 4, _lib.HEAD_SIGMOID, device=ctx)
    with pytest.raises(ValueError, match='1-channel'):
        room.Room(od1, si).overlap_adapt([np.zeros(48000, np.int16)] * 2)
    od3 = models.OverlapDetectionModel(weights.synthetic(OD, seed=9), device=ctx, image_type='viridis')
    with pytest.raises(ValueError, match=r'\[N,128,151,3\]'):
        od3.predict(np.zeros((2, 128, 151, 1), np.uint8))
    with pytest.raises(_lib.MmlaError) as e:
        od3.predict_wavs_gated(pcm, None, lens, passes=0)
    assert e.value.code == _lib.MMLA_E_INVALID
    od3z = models.OverlapDetectionModel(weights.synthetic(OD, seed=9), device=ctx)      # a ZCR model: gated runs
    assert od3z.predict_wavs_gated(pcm, None, lens, passes=0)[0].shape == (2, 2)
    # images of the other channel count never reach the library
    with pytest.raises(ValueError):
        ctx.od_loss_grad(T.pack1(T.synthetic1(1)), np.zeros((1, 9, 8, 3), np.uint8), np.zeros(1, np.int32))


# ---- 7. training -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('h,w,B', list(T.GRAD_CASES))
def test_one_channel_loss_gradient_and_moving_statistics_vs_autograd(ctx, h, w, B):
    W, img, labels, mask = T.grad_case(h, w, B)
    r = T.grad_ref(h, w, B)
    (l64, g64, m64, _), (l32, g32, m32, _) = r['f64'], r['f32']
    blob = T.pack1(W)
    loss, grad, moving = ctx.od_loss_grad(blob, img, labels, C.CLASS_W, mask, moving=True)
    assert grad.size == blob.size == weights.n_params(OD, 2, 1)       # the blob's own layout: no phantom rows
    C.check_d32('loss', loss[0], l64, l32)
    g, mv = T.unpack1(grad), T.unpack1(moving)
    assert g[STEM + '/kernel'].shape == (1, 1, 1, 16) and g[STEM + '/kernel'].any()
    for name, _, role in weights.od_spec(2, 1):
        if ref.is_frozen(role):
            assert not g[name].any(), f'{name}: the gradient slot of a moving statistic is not 0'
            C.check_d32('moving ' + name, mv[name], m64[name], m32[name])
            assert (mv[name] != W[name]).any(), f'{name} did not move'
        else:
            C.check_d32(name, g[name], g64[name], g32[name])
            assert mv[name].tobytes() == W[name].tobytes(), f'{name}: moving_out changed a trainable tensor'


def test_one_channel_fit_history_and_updates(ctx):
    c = T.fit_case()
    cfg = T.FIT
    out, hist, ran = ctx.od_finetune(T.pack1(c['W']), c['img'], c['labels'], c['val_img'], c['val_labels'],
                                     C.CLASS_W, c['lr'], c['perm'], c['masks'], cfg['epochs'], cfg['batch'], 0)
    r = T.fit_ref()
    (W64, h64, ran64, _), (W32, h32, _, _) = r['f64'], r['f32']
    print('history', hist.tolist())
    assert ran == ran64 == cfg['epochs'] and out.size == weights.n_params(OD, 2, 1)
    assert hist.shape == (cfg['epochs'], 5) and np.isfinite(hist).all()
    for col, name in enumerate(('loss', 'acc', 'val_loss', 'val_acc', 'lr')):
        C.check_d32(name, hist[:, col], h64[:, col], h32[:, col])
    got = T.unpack1(out)
    assert got[STEM + '/kernel'].shape == (1, 1, 1, 16) and (got[STEM + '/kernel'] != c['W'][STEM + '/kernel']).any()
    C.check_updates(c['W'], got, W64, C.fit_lr_sum(c, cfg), 'one-channel fit')
    for name, _, role in weights.od_spec(2, 1):
        if ref.is_frozen(role):
            C.check_d32('moving ' + name, got[name], W64[name], W32[name])


def test_train_model_returns_a_one_channel_model_that_round_trips(ctx, tmp_path):
    rng = np.random.default_rng(21)
    n, nv = 8, 4
    img = rng.integers(0, 256, (n + nv, 20, 23, 1)).astype(np.uint8)
    y = np.array([0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 0, 1])       # 5 : 3 -> one blurred copy of every class-1 image
    save = str(tmp_path / 'gray_model')
    model, history = overlap_detector.train_model(img[:n], y[:n], img[n:], y[n:], epochs=2, batch_size=4,
                                                  weighted=True, augmented=True, seed=5, save_path=save, device=ctx)
    assert model.channels == 1 and model.image_type == 'gray' and history.epochs_run == 2
    assert model.W[STEM + '/kernel'].shape == (1, 1, 1, 16) and ctx.od_channels == 1
    W0 = weights.initial_od(5, 2, 1)
    assert (model.W[STEM + '/kernel'] != W0[STEM + '/kernel']).any()
    back = models.load_model(save, device=ctx)
    assert back.channels == 1 and back.image_type == 'gray' and back.n_classes == 2
    assert set(back.W) == set(model.W) and all(back.W[k].tobytes() == model.W[k].tobytes() for k in model.W)
    shapes = tfbundle.variable_shapes(os.path.join(save, 'variables', 'variables.index'))
    assert tuple(shapes[STEM + '/kernel']) == (1, 1, 1, 16)
    x = rng.integers(0, 256, (3, 128, 151, 1)).astype(np.uint8)
    probs = back.predict(x)
    assert probs.shape == (3, 2) and np.isfinite(probs).all()
    m, _, _ = overlap_detector.evaluation(back, x, np.array([0, 1, 0]))
    assert m.sum() == 3
    # continue_train keeps the layout
    plan = overlap_detector.fit_plan(y[:n], 3, 1, val_ratio=0)
    W2, hist, ran = overlap_detector.continue_train(back.W, img[:n], y[:n], plan, 1, 4, device=ctx)
    assert ran == 1 and W2[STEM + '/kernel'].shape == (1, 1, 1, 16) and np.isfinite(hist[:, :2]).all()
