"""GPU: training the SI base model from scratch -- mmla_si_base_drop_mask, mmla_si_base_loss_grad and
mmla_si_base_train (si_base.hip, si_bwd.hip) against the torch-CPU restatement with autograd
(tests/si_base_ref.py), then speaker_identification.train end to end.

The bounds are the two rules of tests/si_finetune_cases.py: every loss, gradient tensor, moving statistic and
history column within 16 x d32 of the helper's float64 run (d32 = the helper's own float32 deviation on the same
inputs, floor 16 x 2^-24 x max|ref|), and fitted weights compared as updates.  The inputs' conditions (ReLU /
pool margins of the gradient seeds, the float32 helper inside the update cap, the stopping and checkpoint
decisions clear of the d32 bound) are asserted on the CPU in tests/test_si_base_ref_cpu.py."""
import warnings

import numpy as np
import pytest

import si_base_cases as C
import si_base_ref as ref
import si_finetune_cases as FC
import si_finetune_ref as ft
from mmla_audio_amd import _lib, models, weights
from mmla_audio_amd import speaker_identification as si
from oracle import nets

pytestmark = pytest.mark.gpu

K = C.FIT_K
HEAD = 'layer_with_weights-42'


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- 1. dropout bits ----------------------------------------------------------------------------------

@pytest.mark.parametrize('epoch', [0, 7])
def test_drop_mask_equals_the_numpy_philox(ctx, epoch):
    ids = np.array([5, 0, 2 ** 24 - 1], np.int32)
    a, b = ctx.si_base_drop_mask(C.DROP_SEED, epoch, ids)
    wa, wb = ref.drop_masks(C.DROP_SEED, epoch, ids)
    assert a.shape == (3, 32, 128) and b.shape == (3, 512)
    assert a.tobytes() == wa.tobytes() and b.tobytes() == wb.tobytes()
    a, b = ctx.si_base_drop_mask(C.DROP_SEED, epoch, None, n=3)
    wa, wb = ref.drop_masks(C.DROP_SEED, epoch, np.arange(3))
    assert a.tobytes() == wa.tobytes() and b.tobytes() == wb.tobytes()


# ---- 2. gradient --------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,Kc', C.GRAD_CASES)
def test_loss_gradient_and_moving_statistics_vs_autograd(ctx, B, Kc):
    W, x, labels, ids, _ = C.grad_case(B, Kc)
    r = C.grad_ref(B, Kc)
    (d64, r64, g64, m64), (d32, r32, g32, m32) = r['f64'], r['f32']
    blob = C.pack(W, Kc)
    loss, grad, moved = ctx.si_base_loss_grad(blob, Kc, x, labels, C.DROP_SEED, C.GRAD_EPOCH, ids, moving=True)
    FC.check_d32('data term', loss[0], d64, d32)
    FC.check_d32('R', loss[1], r64, r32)
    g, mv = C.unpack(grad, Kc), C.unpack(moved, Kc)
    for name, _, role in weights.si_spec(Kc):
        if ft.is_frozen(role):
            assert not g[name].any(), f'{name}: the gradient slot of a moving statistic is not 0'
            FC.check_d32('moving_out ' + name, mv[name], m64[name], m32[name])
            assert (mv[name] != W[name]).all(), f'{name}: a moving statistic did not move'
            continue
        assert mv[name].tobytes() == W[name].tobytes(), f'{name}: moving_out changed a weight'
        if ref.is_dead(name, role):
            assert not g[name].any(), f'{name}: the gradient slot of a Conv1D bias is not 0'
        else:
            FC.check_d32(name, g[name], g64[name], g32[name])


# ---- 3. the head's edges ----------------------------------------------------------------------------------

def _flat_head(logits):
    """the fit case's network with a head that ignores the embedding: z = logits for every sample"""
    c = C.fit_case()
    W = dict(c['W'])
    W[HEAD + '/kernel'] = np.zeros((512, K), np.float32)
    W[HEAD + '/bias'] = np.asarray(logits, np.float32)
    return c, W


def test_head_extreme_logits(ctx):
    c, W = _flat_head([80.0, 0.5, -0.25])
    x = c['x'][:2]
    loss, grad = ctx.si_base_loss_grad(C.pack(W, K), K, x, np.zeros(2, np.int32), C.DROP_SEED)
    assert float(loss[0]) == 0.0 and np.isfinite(grad).all()
    c, W = _flat_head([-80.0, 0.5, -0.25])
    loss, grad = ctx.si_base_loss_grad(C.pack(W, K), K, x, np.zeros(2, np.int32), C.DROP_SEED)
    want = 80.0 + np.log(np.exp(-80.0) + np.exp(0.5) + np.exp(-0.25))
    print('loss', float(loss[0]), 'want', want)
    assert abs(float(loss[0]) - want) <= float(np.spacing(np.float32(want)))
    assert np.isfinite(grad).all()
    gb = C.unpack(grad, K)[HEAD + '/bias'].astype(np.float64)
    p = np.exp(np.array([-80.0, 0.5, -0.25])) / np.exp(np.array([-80.0, 0.5, -0.25])).sum()
    assert np.max(np.abs(gb - (p - np.array([1.0, 0.0, 0.0])))) <= 1e-6        # dz summed over the batch mean


def test_a_tie_counts_for_the_first_maximum_only(ctx):
    c, W = _flat_head([1.0, 1.0, 0.0])
    n, nv = C.FIT['n_train'], C.FIT['n_val']
    for label, acc in ((0, 1.0), (1, 0.0), (2, 0.0)):
        out, _, hist, ran, _ = ctx.si_base_train(
            C.pack(W, K), K, c['x'], np.full(n, label, np.int32), c['val_x'], np.full(nv, label, np.int32),
            c['perm'][:1], 1, C.FIT['batch'], 0.0, C.DROP_SEED)
        assert ran == 1 and hist[0, 1] == acc and hist[0, 3] == acc, (label, hist)


# ---- 4. fit -------------------------------------------------------------------------------------------

def _fit(ctx, c, cfg, **over):
    a = dict(cfg, **over)
    ep = a['epochs']
    return ctx.si_base_train(C.pack(c['W'], K), K, c['x'], c['labels'], c['val_x'], c['val_labels'],
                             c['perm'][:ep], ep, a['batch'], a['lr'], C.DROP_SEED, a['patience'], a['ckpt_period'])


@pytest.fixture(scope='module')
def fitted(ctx):
    res = _fit(ctx, C.fit_case(), C.FIT)
    for a in res[:3]:
        if a is not None:
            a.setflags(write=False)
    return res


def test_fit_history_updates_and_checkpoint(ctx, fitted):
    c = C.fit_case()
    out, best, hist, ran, best_ep = fitted
    r = C.fit_ref()
    (W64, h64, i64), (W32, h32, _) = r['f64'], r['f32']
    print('history', hist.tolist(), 'best epoch', best_ep)
    assert ran == C.FIT['epochs'] and hist.shape == (C.FIT['epochs'], 4) and np.isfinite(hist).all()
    for col, name in enumerate(si.HISTORY_KEYS):
        FC.check_d32(name, hist[:, col], h64[:, col], h32[:, col])
    got = C.unpack(out, K)
    C.check_updates(c['W'], got, W64, 'kernel', C.fit_steps(), C.FIT['lr'])
    for name, _, role in weights.si_spec(K):
        if ft.is_frozen(role):
            FC.check_d32(name, got[name], W64[name], W32[name])
            assert (got[name] != c['W'][name]).all(), f'{name}: a moving statistic did not move'
        elif ref.is_dead(name, role):
            assert got[name].tobytes() == c['W'][name].tobytes(), f'{name}: a Conv1D bias moved'
        else:
            assert (got[name] != c['W'][name]).any(), f'{name} did not move'
    assert best_ep == i64['best_epoch'] and best is not None
    again = _fit(ctx, c, C.FIT, epochs=best_ep + 1, ckpt_period=0)
    assert best.tobytes() == again[0].tobytes(), 'best_out is not the state after its epoch'
    assert again[1] is None and again[4] == -1


def test_early_stop(ctx):
    c = C.stop_case()
    want = ref.early_stop_epochs(C.stop_ref()['f64'][1][:, 2], C.STOP['patience'])
    out, _, hist, ran, best_ep = _fit(ctx, c, C.STOP)
    print('history', hist.tolist())
    assert ran == want and best_ep == -1
    assert np.isfinite(hist[:ran]).all() and np.isnan(hist[ran:]).all() and hist.shape == (C.STOP['epochs'], 4)
    short = _fit(ctx, c, C.STOP, epochs=ran, patience=0)
    assert out.tobytes() == short[0].tobytes() and hist[:ran].tobytes() == short[2].tobytes()


def test_fit_is_bit_reproducible_and_zero_epochs_is_the_identity(ctx, fitted):
    c = C.fit_case()
    out, best, hist, ran, best_ep = _fit(ctx, c, C.FIT)
    assert out.tobytes() == fitted[0].tobytes() and hist.tobytes() == fitted[2].tobytes()
    assert best.tobytes() == fitted[1].tobytes() and (ran, best_ep) == fitted[3:]
    same, none, h0, ran0, b0 = _fit(ctx, c, C.FIT, epochs=0)
    assert same.tobytes() == C.pack(c['W'], K).tobytes() and h0.shape == (0, 4) and none is None
    assert (ran0, b0) == (0, -1)


def test_fit_without_a_validation_set(ctx, fitted):
    c = C.fit_case()
    out, best, hist, ran, best_ep = ctx.si_base_train(
        C.pack(c['W'], K), K, c['x'], c['labels'], None, None, c['perm'], C.FIT['epochs'], C.FIT['batch'],
        C.FIT['lr'], C.DROP_SEED, 3, C.FIT['ckpt_period'])
    assert out.tobytes() == fitted[0].tobytes() and ran == C.FIT['epochs'] and best is None and best_ep == -1
    assert hist[:, :2].tobytes() == fitted[2][:, :2].tobytes() and np.isnan(hist[:, 2:]).all()


def test_device_pointers_match_the_host_calls(ctx, fitted):
    import torch
    c = C.fit_case()
    blob = C.pack(c['W'], K)
    n, nv, ep = C.FIT['n_train'], C.FIT['n_val'], C.FIT['epochs']
    ids = np.array([4, 9, 1, 0, 77], np.int32)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
           for k, v in dict(blob=blob, x=c['x'], labels=c['labels'], val_x=c['val_x'], val_labels=c['val_labels'],
                            perm=c['perm'], ids=ids).items()}
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device='cuda')      # noqa: E731
    out, best, hist, loss, grad, moved = f32(blob.size), f32(blob.size), f32(ep, 4), f32(2), f32(blob.size), \
        f32(blob.size)
    words = torch.full((2,), 99, dtype=torch.int32, device='cuda')
    ma = torch.zeros((n, 32, 128), dtype=torch.uint8, device='cuda')
    mb = torch.zeros((n, 512), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.si_base_train_dev(dev['blob'].data_ptr(), blob.size, K, dev['x'].data_ptr(), dev['labels'].data_ptr(), n,
                          dev['val_x'].data_ptr(), dev['val_labels'].data_ptr(), nv, ep, C.FIT['batch'],
                          C.FIT['lr'], dev['perm'].data_ptr(), C.DROP_SEED, C.FIT['patience'],
                          C.FIT['ckpt_period'], out.data_ptr(), best.data_ptr(), hist.data_ptr(),
                          words.data_ptr(), words.data_ptr() + 4)
    ctx.si_base_loss_grad_dev(dev['blob'].data_ptr(), blob.size, K, dev['x'].data_ptr(), dev['labels'].data_ptr(),
                              n, C.DROP_SEED, 1, dev['ids'].data_ptr(), loss.data_ptr(), grad.data_ptr(),
                              moved.data_ptr())
    ctx.si_base_drop_mask_dev(C.DROP_SEED, 1, dev['ids'].data_ptr(), n, ma.data_ptr(), mb.data_ptr())
    ctx.synchronize()
    assert out.cpu().numpy().tobytes() == fitted[0].tobytes()
    assert best.cpu().numpy().tobytes() == fitted[1].tobytes()
    assert hist.cpu().numpy().tobytes() == fitted[2].tobytes()
    assert tuple(words.cpu().tolist()) == fitted[3:]
    assert dev['blob'].cpu().numpy().tobytes() == blob.tobytes(), 'the input blob was written'
    want = ctx.si_base_loss_grad(blob, K, c['x'], c['labels'], C.DROP_SEED, 1, ids, moving=True)
    for got, w in zip((loss, grad, moved), want):
        assert got.cpu().numpy().tobytes() == w.tobytes()
    wa, wb = ctx.si_base_drop_mask(C.DROP_SEED, 1, ids)
    assert ma.cpu().numpy().tobytes() == wa.tobytes() and mb.cpu().numpy().tobytes() == wb.tobytes()


# ---- 5. arguments -------------------------------------------------------------------------------------

def test_invalid_arguments_are_rejected(ctx):
    c = C.fit_case()
    blob = C.pack(c['W'], K)
    n, nv, ep = C.FIT['n_train'], C.FIT['n_val'], C.FIT['epochs']
    out, best = np.empty_like(blob), np.empty_like(blob)
    hist = np.empty((ep, 4), np.float32)
    loss = np.empty(2, np.float32)
    words = np.zeros(2, np.int32)
    x, lab = np.ascontiguousarray(c['x']), np.ascontiguousarray(c['labels'])
    vx, vl = np.ascontiguousarray(c['val_x']), np.ascontiguousarray(c['val_labels'])
    perm = np.ascontiguousarray(c['perm'])
    ids = np.arange(n, dtype=np.int32)
    ma, mb = np.empty((n, 32, 128), np.uint8), np.empty((n, 512), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    good = dict(packed=blob, n_floats=blob.size, k=K, x=x, labels=lab, n=n, vx=vx, vl=vl, nv=nv, epochs=ep,
                batch=2, lr=1e-4, perm=perm, patience=0, period=2, out=out, best=best, hist=hist, ran=words[:1],
                bep=words[1:], ids=ids, epoch=0, ma=ma, mb=mb)

    def fit_rc(**over):
        a = dict(good, **over)
        return ctx.lib.mmla_si_base_train(
            ctx.h, p(a['packed']), a['n_floats'], a['k'], p(a['x']), p(a['labels']), a['n'], p(a['vx']), p(a['vl']),
            a['nv'], a['epochs'], a['batch'], a['lr'], p(a['perm']), _lib._seed64(C.DROP_SEED), a['patience'], a['period'],
            p(a['out']), p(a['best']), p(a['hist']), p(a['ran']), p(a['bep']), 0)

    def grad_rc(**over):
        a = dict(good, **over)
        return ctx.lib.mmla_si_base_loss_grad(
            ctx.h, p(a['packed']), a['n_floats'], a['k'], p(a['x']), p(a['labels']), a['n'], _lib._seed64(C.DROP_SEED),
            a['epoch'], p(a['ids']), p(loss), p(a['out']), p(a['best']), 0)

    def mask_rc(**over):
        a = dict(good, **over)
        return ctx.lib.mmla_si_base_drop_mask(ctx.h, _lib._seed64(C.DROP_SEED), a['epoch'], p(a['ids']), a['n'], p(a['ma']),
                                              p(a['mb']), 0)

    bad_label = lab.copy()
    bad_label[2] = K
    twice = perm.copy()
    twice[1, 0] = twice[1, 1]
    bad_ids = ids.copy()
    bad_ids[1] = -1
    cases = [dict(k=0), dict(k=_lib.SI_BASE_MAX_CLASSES + 1), dict(n_floats=blob.size - 1),
             dict(n_floats=weights.n_params(weights.SI, K + 1)), dict(batch=0), dict(n=0), dict(nv=-1),
             dict(epochs=-1), dict(patience=-1), dict(period=-1), dict(lr=-1e-4), dict(lr=float('nan')),
             dict(lr=float('inf')), dict(packed=None), dict(x=None), dict(labels=None), dict(out=None),
             dict(best=None), dict(hist=None), dict(ran=None), dict(bep=None), dict(perm=None), dict(vx=None),
             dict(vl=None), dict(labels=bad_label), dict(vl=np.full(nv, -1, np.int32)), dict(perm=twice)]
    for over in cases:
        assert fit_rc(**over) == -1, over
    for over in (dict(k=0), dict(k=_lib.SI_BASE_MAX_CLASSES + 1), dict(n_floats=blob.size + 1), dict(n=0),
                 dict(n=4097), dict(epoch=-1), dict(packed=None), dict(x=None), dict(labels=None), dict(out=None),
                 dict(labels=bad_label), dict(ids=bad_ids)):
        assert grad_rc(**over) == -1, over
    for over in (dict(n=0), dict(epoch=-1), dict(ma=None), dict(mb=None), dict(ids=bad_ids)):
        assert mask_rc(**over) == -1, over
    # the context still works, and the good calls are good; no checkpoint output is needed without the callback
    assert fit_rc() == 0 and grad_rc() == 0 and mask_rc() == 0 and grad_rc(best=None, ids=None) == 0
    assert fit_rc(best=None, period=0) == 0


def test_class_count_limits_old_and_new(ctx):
    K33 = _lib.SI_TRAIN_MAX_CLASSES + 1
    W = C.synthetic(C.FIT_SEED, K33)
    blob = C.pack(W, K33)
    c = C.fit_case()
    x, labels = c['x'][:2], np.array([32, 0], np.int32)
    with pytest.raises(_lib.MmlaError):
        ctx.si_loss_grad(blob, K33, x, labels)
    with pytest.raises(_lib.MmlaError):
        ctx.si_finetune(blob, K33, x, labels, None, None, c['perm'][:1, :2] % 2, 1)
    loss, grad = ctx.si_base_loss_grad(blob, K33, x, labels, C.DROP_SEED)
    assert np.isfinite(loss).all() and np.isfinite(grad).all() and grad.any()
    # and the old entries still work afterwards on a head of their own size
    W3, x3, l3 = FC.grad_case(2)
    loss3, _ = ctx.si_loss_grad(weights.pack(weights.SI, W3, FC.K), FC.K, x3, l3)
    assert np.isfinite(loss3).all()


# ---- 6. train(), save, load, transfer_learning ----------------------------------------------------------------

def _corpus():
    rng = np.random.default_rng(505)
    x = (rng.standard_normal((12, 256, 39)) * 10).astype(np.float32)
    labels = np.repeat(np.arange(3, dtype=np.int32), 4)
    return x, labels, np.eye(3)[labels]


def test_train_save_load_and_transfer_learning(ctx, tmp_path):
    x, labels, y = _corpus()
    tr = np.array([0, 1, 2, 4, 5, 6, 8, 9, 10])
    va = np.array([3, 7, 11])
    ckpt = str(tmp_path / 'ckt')
    model, history = si.train(x[tr], y[tr], x[va], y[va], epochs=2, batch_size=4, checkpoint_path=ckpt,
                              checkpoint_period=1, seed=5, device=ctx)
    h = history.history
    print('history', h, 'best epoch', history.best_epoch)
    assert list(h) == list(si.HISTORY_KEYS) and all(len(v) == 2 and np.isfinite(v).all() for v in h.values())
    assert history.epochs_run == 2 and history.best_epoch in (0, 1)
    assert model.n_classes == 3 and model.head == _lib.HEAD_SOFTMAX and not model.synthetic
    W0 = weights.initial(weights.SI, 5, 3)
    assert any((model.W[k] != W0[k]).any() for k in W0), 'train returned the initial state'
    # the installed model answers at once, with its own weights
    got = model.predict(x[va])
    want = nets.si_forward(x[va].astype(np.float64), model.W, head='softmax', dtype=np.float64)
    err = float(np.max(np.abs(np.log(got.astype(np.float64)) - np.log(want))))
    print('|dlog p|', err)
    assert got.shape == (3, 3) and err <= 1e-4
    # model.save -> load_model: the same tensors, the same answer
    saved = str(tmp_path / 'cnnlstm')
    model.save(saved)
    back = models.load_model(saved, device=ctx)
    assert back.n_classes == 3 and back.head == _lib.HEAD_SOFTMAX and not back.synthetic
    assert all(back.W[k].tobytes() == model.W[k].tobytes() for k in model.W)
    assert back.predict(x[va]).tobytes() == got.tobytes()
    best = models.load_model(ckpt, device=ctx)              # the checkpoint is a base model too
    assert best.n_classes == 3 and set(best.W) == set(model.W)
    # and a registration on it needs no synthetic weights
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)      # the synthetic-weights warning would be one
        acc = si.transfer_learning(x, y, 1, 0, saved, str(tmp_path / 'deployed'), epochs=5, device=ctx)
    assert 0.0 <= acc <= 1.0
    assert models.load_model(str(tmp_path / 'deployed'), device=ctx).head == _lib.HEAD_SIGMOID


def test_make_feature_timit(ctx, tmp_path):
    import scipy.io.wavfile as wavfile
    rng = np.random.default_rng(606)
    lens = (30000, 3000, 50000)                   # 3000: below the 'silent' length, which has no say here
    sigs = [(rng.standard_normal(n) * 3000).astype(np.int16) for n in lens]
    for i, sig in enumerate(sigs):
        wavfile.write(str(tmp_path / f'u{i}.wav'), 16000, sig)
    files = [f'u{i}.wav' for i in range(3)]
    x, y = si.make_feature_timit(files, ['spk_a', 'spk_b', 'spk_a'], str(tmp_path), device=ctx)
    assert x.shape == (3, 256, 39) and x.dtype == np.float64 and y.shape == (3, 630)
    assert (y.sum(axis=1) == 1).all() and (y[0] == y[2]).all() and (y[0] != y[1]).any()
    for i, sig in enumerate(sigs):                # the whole recording's features, padded or cut to 256 frames
        want = ctx.si_features_seq(sig)[0]
        assert np.max(np.abs(x[i] - want)) <= 1e-4 * max(1.0, float(np.max(np.abs(want)))), i
    frames = _lib.si_seq_frames(lens[1])
    assert x[1, :frames].any() and not x[1, frames:].any()
