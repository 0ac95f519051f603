"""GPU: OD-NET with a K-way softmax head (2 < K <= 8) through every layer -- loading, the head kernel, the
pipelines' output offsets, loss / gradient / fit (od_bwd.hip's K-class kernels), the K-class AUC and the Python
surface.  Inputs and restatements: tests/od_kclass_cases.py; their conditions are asserted on the CPU in
tests/test_od_kclass_cpu.py.

No bound is new: the forward is held to oracle/compare.py's LOGP_TOL and argmax rule exactly as
test_gpu_parity.test_od_forward_vs_oracle holds K = 2; losses, gradients, moving statistics and history columns
to the d32 rule and fitted weights to the update rule of tests/od_finetune_cases.py; the AUC to AUC_TOL of
tests/test_gpu_od_train.py.  The head alone is held to 16 x the float32-vs-float64 numpy difference on the
same input, floor 16 x 2^-24.
"""
import numpy as np
import pytest

import od_finetune_cases as C
import od_finetune_ref as ref
import od_kclass_cases as KC
from mmla_audio_amd import _lib, metrics, models, overlap_detector, room, weights
from oracle import compare, nets

pytestmark = pytest.mark.gpu

HEAD = KC.HEAD
OD = weights.OD


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _load(ctx, W):
    K = weights.od_classes(W)
    ctx.load_weights(OD, KC.pack(W), K)
    return K


def _clips(n=5, seed=7):
    return np.random.default_rng([seed, 96]).integers(-8000, 8000, (n, _lib.OD_CLIP)).astype(np.int16)


# ---- 1. forward --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', KC.KS)
def test_forward_vs_oracle(ctx, K):
    W = KC.synthetic(1, K)
    _load(ctx, W)
    x8 = KC.forward_inputs()
    x = x8.astype(np.float32)
    p = ctx.od_forward(x)
    want = nets.od_forward(x, W)
    assert p.shape == (5, K) and p.dtype == np.float32
    err = compare.logp_err(p, want)
    print('K', K, 'max |log p - log p_ref|', err)
    assert err <= compare.LOGP_TOL
    assert compare.argmax_ok(p, want)
    assert np.array_equal(ctx.od_forward(x8), p)


# ---- 2. the head alone -------------------------------------------------------------------------------------

def _numpy_head(H, W, dtype):
    alpha = np.float32(0.3).astype(dtype)
    h = H.astype(dtype)
    v = np.where(h > 0, h, h * alpha)
    z = v @ W[HEAD + '/kernel'].astype(dtype) + W[HEAD + '/bias'].astype(dtype)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize('K', KC.KS)
def test_head_alone_on_the_traced_embedding(ctx, K):
    W = KC.synthetic(1, K)
    _load(ctx, W)
    x = KC.forward_inputs().astype(np.float32)
    H = ctx.debug_od_trace(x, 11)
    assert H.shape == (5, 512)
    p = ctx.od_forward(x)
    p64, p32 = _numpy_head(H, W, np.float64), _numpy_head(H, W, np.float32)
    d32 = float(np.abs(p32.astype(np.float64) - p64).max())
    bound = C.FACTOR * max(d32, 2.0 ** -24)
    err = float(np.abs(p.astype(np.float64) - p64).max())
    print('K', K, 'err', err, 'd32', d32, 'bound', bound)
    assert err <= bound


# ---- 3. ties and silent ------------------------------------------------------------------------------------

def test_ties_go_to_the_first_index_and_short_clips_are_silent(ctx):
    W = KC.synthetic(1, 3)
    W[HEAD + '/kernel'] = np.zeros((512, 3), np.float32)
    pcm = _clips(3)
    lens = np.array([_lib.OD_CLIP, _lib.OD_CLIP, 3999], np.int32)
    W[HEAD + '/bias'] = np.full(3, 0.25, np.float32)
    _load(ctx, W)
    probs, am, silent = ctx.od_pipeline(pcm, lens)
    assert probs.shape == (3, 3)
    assert (probs[:, 0] == probs[:, 1]).all() and (probs[:, 1] == probs[:, 2]).all()
    assert am.tolist() == [0, 0, -1] and silent.tolist() == [False, False, True]
    assert (probs.argmax(1)[:2] == am[:2]).all()
    W[HEAD + '/bias'] = np.array([0, 1, 1], np.float32)
    _load(ctx, W)
    probs, am, silent = ctx.od_pipeline(pcm, lens)
    assert (probs[:, 1] == probs[:, 2]).all() and (probs[:, 1] > probs[:, 0]).all()
    assert am.tolist() == [1, 1, -1] and (probs.argmax(1)[:2] == 1).all()


# ---- 4. micro-batch offsets --------------------------------------------------------------------------------

def test_microbatches_and_every_pipeline_write_the_same_k_wide_rows(ctx):
    W = KC.synthetic(1, 3)
    _load(ctx, W)
    Wsi = weights.synthetic(weights.SI, seed=2, n_classes=4)
    ctx.load_weights(weights.SI, weights.pack(weights.SI, Wsi, 4), 4, _lib.HEAD_SIGMOID)
    pcm = _clips(5)
    whole = ctx.od_pipeline(pcm)
    assert whole[0].shape == (5, 3) and len(set(map(bytes, whole[0]))) == 5     # five different rows
    try:
        ctx.set_microbatch(od=2)
        split = ctx.od_pipeline(pcm)
        split_fwd = ctx.od_forward(ctx.od_features(pcm, db=False, norm=False, zcr=False)['img'])
    finally:
        ctx.set_microbatch(0, 0)
    for a, b in zip(whole, split):
        assert a.tobytes() == b.tobytes()
    img = ctx.od_features(pcm, db=False, norm=False, zcr=False)['img']
    fwd = ctx.od_forward(img)
    assert fwd.tobytes() == whole[0].tobytes() and split_fwd.tobytes() == fwd.tobytes()
    got = ctx.room_pipeline_conditioned(pcm, None, None, 0, False, 1)
    assert got[0].shape == (5, 3) and got[0].tobytes() == whole[0].tobytes()
    assert got[1].tobytes() == whole[1].tobytes() and got[2].shape == (5, 4)
    plan = _lib.MixPlan.from_layers([[(i * _lib.OD_CLIP, _lib.OD_CLIP, 0)] for i in range(5)])
    mixed = ctx.od_pipeline_mixed(pcm.reshape(-1), plan)
    assert mixed[0].tobytes() == whole[0].tobytes() and mixed[1].tobytes() == whole[1].tobytes()


# ---- 5. loading --------------------------------------------------------------------------------------------

def test_loading_checks_k_and_the_blob_and_results_follow_the_loaded_model(ctx):
    W3, W2 = KC.synthetic(1, 3), weights.synthetic(OD, seed=1)
    b3, b2 = KC.pack(W3), weights.pack(OD, W2)
    x = KC.forward_inputs()[:2]
    _load(ctx, W3)
    first = ctx.od_forward(x)
    k = np.zeros(1, np.int32)
    assert ctx.lib.mmla_od_classes(ctx.h, k.ctypes.data) == 0 and k[0] == 3

    def rc(blob, n_floats, K):
        return ctx.lib.mmla_load_weights(ctx.h, OD, blob.ctypes.data, n_floats, K, 0)

    assert rc(b3, b3.size, 1) == _lib.MMLA_E_INVALID
    assert rc(b3, b3.size, 9) == _lib.MMLA_E_INVALID
    assert rc(b3, b3.size - 1, 3) == _lib.MMLA_E_INVALID
    assert rc(b2, b2.size, 3) == _lib.MMLA_E_INVALID
    assert ctx.od_forward(x).tobytes() == first.tobytes()        # the refused loads left the model
    ctx.load_weights(OD, b2, 2)
    two = ctx.od_forward(x)
    assert two.shape == (2, 2) and ctx.od_classes == 2
    ctx.load_weights(OD, b3, 3)
    again = ctx.od_forward(x)
    assert again.shape == (2, 3) and again.tobytes() == first.tobytes()
    assert np.abs(two.sum(axis=1) - 1).max() < 1e-6 and np.abs(again.sum(axis=1) - 1).max() < 1e-6


# ---- 6. loss and gradient ----------------------------------------------------------------------------------

@pytest.mark.parametrize('K', KC.KS)
@pytest.mark.parametrize('h,w,B', KC.GRAD_SHAPES)
def test_loss_gradient_and_moving_statistics_vs_autograd(ctx, h, w, B, K):
    W, img, labels, mask = KC.grad_case(h, w, B, K)
    r = KC.grad_ref(h, w, B, K)
    (l64, g64, m64, _), (l32, g32, m32, _) = r['f64'], r['f32']
    loss, grad, moving = ctx.od_loss_grad(KC.pack(W), img, labels, KC.class_w(K), mask, moving=True)
    C.check_d32('loss', loss[0], l64, l32)
    g, mv = KC.unpack(grad, K), KC.unpack(moving, K)
    assert g[HEAD + '/kernel'].shape == (512, K) and g[HEAD + '/bias'].shape == (K,)
    for name, _, role in KC.spec(K):
        if ref.is_frozen(role):
            assert not g[name].any(), f'{name}: the gradient slot of a moving statistic is not 0'
            C.check_d32('moving ' + name, mv[name], m64[name], m32[name])
        else:
            C.check_d32(name, g[name], g64[name], g32[name])
            assert mv[name].tobytes() == W[name].tobytes(), f'{name}: moving_out changed a trainable tensor'
    assert g[HEAD + '/kernel'].any() and g[HEAD + '/bias'].any()


def test_clipped_samples_give_the_clip_loss_and_no_gradient(ctx):
    W, img, labels, mask = KC.clip_case()
    cw = KC.class_w(3)
    loss, grad = ctx.od_loss_grad(KC.pack(W), img, labels, cw, mask)
    want = np.float32(np.float64(cw[1]) * -np.log(np.float64(np.float32(1e-7))))
    print('loss', float(loss[0]), 'want', float(want))
    assert abs(float(loss[0]) - float(want)) <= float(np.spacing(want)), (loss, want)
    assert not grad.any(), 'a clipped batch has a gradient'


def test_loss_grad_arguments(ctx):
    W, img, labels, mask = KC.grad_case(9, 8, 1, 3)
    blob = KC.pack(W)
    with pytest.raises(_lib.MmlaError, match='labels'):
        ctx.od_loss_grad(blob, img, np.array([3], np.int32), KC.class_w(3), mask)
    with pytest.raises(ValueError):
        ctx.od_loss_grad(blob, img, labels, (0.3, 0.7), mask)              # class_w is [K]
    with pytest.raises(ValueError):
        ctx.od_loss_grad(blob[:-1], img, labels, None, mask)               # no K has this size
    a = ctx.od_loss_grad(blob, img, labels, None, mask)                    # the default: ones of K
    b = ctx.od_loss_grad(blob, img, labels, np.ones(3), mask)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 7. the fit --------------------------------------------------------------------------------------------

def _train(ctx, c, epochs, batch):
    return ctx.od_train(KC.pack(c['W']), c['img'], c['labels'], c['val_img'], c['val_labels'], c['class_w'],
                        c['lr'][:epochs], c['perm'][:epochs], epochs, batch, KC.DROP_SEED, 0, 1)


def _finetune(ctx, c, epochs, masks):
    return ctx.od_finetune(KC.pack(c['W']), c['img'], c['labels'], c['val_img'], c['val_labels'], c['class_w'],
                           c['lr'][:epochs], c['perm'][:epochs], masks[:epochs], epochs, KC.FIT['batch'], 0)


@pytest.fixture(scope='module')
def trained(ctx):
    r = _train(ctx, KC.fit_case(), KC.FIT['epochs'], KC.FIT['batch'])
    for a in r[:3]:
        if a is not None:
            a.setflags(write=False)
    return r


def test_fit_history_updates_and_moving_statistics(ctx, trained):
    c = KC.fit_case()
    out, _, hist, ran, _ = trained
    r = KC.fit_ref()
    (W64, h64, ran64, _), (W32, h32, _, _) = r['f64'], r['f32']
    E = KC.FIT['epochs']
    print('history', hist.tolist())
    assert ran == ran64 == E and hist.shape == (E, 7) and np.isfinite(hist).all()
    for col, name in enumerate(('loss', 'acc', 'val_loss', 'val_acc', 'lr')):
        C.check_d32(name, hist[:, col], h64[:, col], h32[:, col])
    got = KC.unpack(out, KC.FIT_K)
    C.check_updates(c['W'], got, W64, C.fit_lr_sum(c, KC.FIT), 'fit')
    for name, _, role in KC.spec(KC.FIT_K):
        if ref.is_frozen(role):
            C.check_d32('moving ' + name, got[name], W64[name], W32[name])
    assert (got[HEAD + '/kernel'] != c['W'][HEAD + '/kernel']).any()


def test_train_equals_finetune_on_the_masks_of_the_seed(ctx, trained):
    c = KC.fit_case()
    E, n = KC.FIT['epochs'], KC.FIT['n_train']
    masks = np.stack([ctx.od_drop_mask(KC.DROP_SEED, ep, None, n) for ep in range(E)])
    assert masks.tobytes() == c['masks'].tobytes()
    out2, hist2, ran2 = _finetune(ctx, c, E, masks)
    out, _, hist, ran, _ = trained
    assert ran == ran2 == E
    assert out.tobytes() == out2.tobytes()
    assert hist[:, :5].tobytes() == np.ascontiguousarray(hist2).tobytes()


def test_auc_columns_use_the_k_class_definition(ctx, trained):
    c = KC.fit_case()
    hist = trained[2]
    for e in range(KC.FIT['epochs']):
        blob = _finetune(ctx, c, e + 1, c['masks'])[0]
        probs = ref.forward(KC.unpack(blob, KC.FIT_K), c['val_img'])             # inference mode, float64
        assert probs.shape == (KC.FIT['n_val'], KC.FIT_K)
        assert KC.decided(probs), f'epoch {e}: a validation prob is too close to a threshold; change the seed'
        want = KC.auc(probs.astype(np.float32), c['val_labels'])
        print('val_auc', e, float(hist[e, 6]), float(want))
        assert abs(float(hist[e, 6]) - float(want)) <= KC.AUC_TOL
    # the training column of an epoch of one batch: the training-mode outputs of the initial weights
    _, _, h1, _, _ = _train(ctx, c, 1, 16)
    order = c['perm'][0]
    probs = KC.train_probs(c)
    assert KC.decided(probs), 'a training prob is too close to a threshold; change the seed'
    want = KC.auc(probs.astype(np.float32), c['labels'][order])
    print('auc', float(h1[0, 5]), float(want))
    assert abs(float(h1[0, 5]) - float(want)) <= KC.AUC_TOL


# ---- 8. mmla_od_auc_k --------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', KC.KS)
@pytest.mark.parametrize('n', [1, 65, 1000])
def test_auc_k_equals_the_restatement(ctx, n, K):
    probs, labels = KC.auc_inputs(n, K)
    for lab in (labels, np.zeros(n, np.int32), np.full(n, K - 1, np.int32)):
        got, want = ctx.od_auc(probs, lab), KC.auc(probs, lab)
        print(n, K, float(got), float(want))
        assert got.dtype == np.float32 and abs(float(got) - float(want)) <= KC.AUC_TOL


def test_auc_k_at_two_is_od_auc_and_arguments(ctx):
    probs, labels = KC.auc_inputs(1000, 2)
    a, b = np.empty(1, np.float32), np.empty(1, np.float32)
    p = lambda x: x.ctypes.data                                                # noqa: E731
    assert ctx.lib.mmla_od_auc(ctx.h, p(probs), p(labels), 1000, p(a), 0) == 0
    assert ctx.lib.mmla_od_auc_k(ctx.h, p(probs), p(labels), 1000, 2, p(b), 0) == 0
    assert a.tobytes() == b.tobytes() == ctx.od_auc(probs, labels).tobytes()
    p3, l3 = KC.auc_inputs(65, 3)
    with pytest.raises(_lib.MmlaError, match='labels'):
        ctx.od_auc(p3, np.full(65, 3))
    for K in (1, 9):
        assert ctx.lib.mmla_od_auc_k(ctx.h, p(p3), p(l3), 65, K, p(a), 0) == _lib.MMLA_E_INVALID
    assert ctx.lib.mmla_od_auc_k(ctx.h, p(p3), p(l3), 0, 3, p(a), 0) == _lib.MMLA_E_INVALID
    assert ctx.lib.mmla_od_auc_k(ctx.h, None, p(l3), 65, 3, p(a), 0) == _lib.MMLA_E_INVALID
    assert metrics.auc(p3, np.eye(3)[l3]) == float(ctx.od_auc(p3, l3))          # the wrapper, one-hot rows


# ---- 9. Python ---------------------------------------------------------------------------------------------

def test_train_model_predict_save_load_evaluation_and_room(ctx, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, 'default_context', lambda device=None: ctx)
    rng = np.random.default_rng([43, 97])
    n, nv = 12, 3
    img = rng.integers(0, 256, (n + nv, 20, 23, 3)).astype(np.uint8)
    y = np.eye(3)[np.arange(n + nv) % 3]
    save = str(tmp_path / 'model')
    model, history = overlap_detector.train_model(img[:n], y[:n], img[n:], y[n:], epochs=2, batch_size=4,
                                                  weighted=True, seed=5, save_path=save, device=ctx)
    assert model.n_classes == 3 and history.epochs_run == 2 and len(history.history['auc']) == 2
    assert model.W[HEAD + '/kernel'].shape == (512, 3) and ctx.od_classes == 3
    x = rng.integers(0, 256, (6, 128, 151, 3)).astype(np.uint8)
    probs = model.predict(x)
    assert probs.shape == (6, 3) and np.isfinite(probs).all() and np.allclose(probs.sum(axis=1), 1, atol=1e-5)
    back = models.load_model(save, device=ctx)
    assert back.n_classes == 3 and all(back.W[k].tobytes() == model.W[k].tobytes() for k in model.W)
    assert back.predict(x).tobytes() == probs.tobytes()
    truth = np.arange(6) % 3
    m, recall, precision = overlap_detector.evaluation(back, x, np.eye(3)[truth])
    pred = probs.argmax(1)
    want = np.zeros((3, 3))
    for t, q in zip(truth, pred):
        want[t, q] += 1
    assert m.shape == (3, 3) and m.sum() == 6 and np.array_equal(m, want)
    Wsi = weights.synthetic(weights.SI, seed=2, n_classes=4)
    si = models.SpeakerIdModel(Wsi, 4, _lib.HEAD_SIGMOID, device=ctx)
    r = room.Room(back, si)
    rec = [np.zeros(48000, np.int16)] * 2
    with pytest.raises(ValueError, match='K = 3'):
        r.overlap_check(rec)
    with pytest.raises(ValueError, match='K = 3'):
        r.overlap_adapt(rec)
    res = r.tick(_clips(2), passes=0, silence_remove=False)
    assert res.od_probs.shape == (2, 3) and res.si_probs.shape == (2, 4)
    assert room.Room.labels(res, {str(i): f's{i}' for i in range(4)})[0] == [str(int(a)) for a in res.od_argmax]
