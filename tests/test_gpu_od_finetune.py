"""GPU: adapting OD-NET -- mmla_od_loss_grad and mmla_od_finetune (od_bwd.hip, conv.hip, si_bwd.hip) against the
torch-CPU restatement with autograd (tests/od_finetune_ref.py).

The bounds are the two rules of tests/od_finetune_cases.py: every loss, gradient tensor, moving statistic and
history column within 16 x d32 of the restatement's float64 run (d32 = its own float32 deviation on the same
inputs, floor 16 x 2^-24 x max|ref|), and fitted weights compared as updates.  The inputs' conditions (pool and
LeakyReLU margins, the early stop's decisive val_loss gap) are asserted on the CPU in
tests/test_od_finetune_ref_cpu.py."""
import numpy as np
import pytest

import od_finetune_cases as C
import od_finetune_ref as ref
from mmla_audio_amd import _lib, overlap_detector, weights

pytestmark = pytest.mark.gpu

SPEC = C.SPEC
HEAD = ref.HEAD


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- 1. gradient ------------------------------------------------------------------------------------

@pytest.mark.parametrize('h,w,B', list(C.GRAD_CASES))
def test_loss_gradient_and_moving_statistics_vs_autograd(ctx, h, w, B):
    W, img, labels, mask = C.grad_case(h, w, B)
    r = C.grad_ref(h, w, B)
    (l64, g64, m64, _), (l32, g32, m32, _) = r['f64'], r['f32']
    loss, grad, moving = ctx.od_loss_grad(C.pack(W), img, labels, C.CLASS_W, mask, moving=True)
    worst = {}
    C.check_d32('loss', loss[0], l64, l32, worst)
    g, mv = C.unpack(grad), C.unpack(moving)
    for name, _, role in SPEC:
        if ref.is_frozen(role):
            assert not g[name].any(), f'{name}: the gradient slot of a moving statistic is not 0'
            C.check_d32('moving ' + name, mv[name], m64[name], m32[name], worst)
            assert (mv[name] != W[name]).any(), f'{name} did not move'
        else:
            C.check_d32(name, g[name], g64[name], g32[name], worst)
            assert mv[name].tobytes() == W[name].tobytes(), f'{name}: moving_out changed a trainable tensor'
    by_role = {}
    for name, _, role in SPEC:
        key = ('moving ' + name) if ref.is_frozen(role) else name
        by_role[role] = max(by_role.get(role, 0.0), worst[key])
    print('worst ratio per role', {k: round(v, 2) for k, v in by_role.items()})


# ---- 2. clip ----------------------------------------------------------------------------------------

def test_clipped_samples_give_the_clip_loss_and_no_gradient(ctx):
    W, img, labels, mask = C.grad_case(20, 23, 3)
    W = dict(W)
    c = 1
    b = W[HEAD + '/bias'].copy()
    b[c] = -40.0                                   # p_c ~ e^-40, far below the clip's 1e-7
    W[HEAD + '/bias'] = b
    cw = np.array(C.CLASS_W, np.float32)
    loss, grad = ctx.od_loss_grad(C.pack(W), img, np.full(3, c, np.int32), cw, mask)
    want = np.float32(np.float64(cw[c]) * -np.log(np.float64(np.float32(1e-7))))
    assert abs(float(loss[0]) - float(want)) <= float(np.spacing(want)), (loss, want)
    assert not grad.any(), 'a clipped batch has a gradient'


# ---- 3. fit -------------------------------------------------------------------------------------------

def _fit(ctx, c, cfg, epochs=None, patience=0):
    epochs = cfg['epochs'] if epochs is None else epochs
    return ctx.od_finetune(C.pack(c['W']), c['img'], c['labels'], c['val_img'], c['val_labels'], C.CLASS_W,
                           c['lr'][:epochs], c['perm'][:epochs], c['masks'][:epochs], epochs, cfg['batch'],
                           patience)


@pytest.fixture(scope='module')
def fitted(ctx):
    out, hist, ran = _fit(ctx, C.fit_case(), C.FIT)
    out.setflags(write=False)
    hist.setflags(write=False)
    return out, hist, ran


def test_fit_history_updates_and_moving_statistics(ctx, fitted):
    c = C.fit_case()
    out, hist, ran = fitted
    r = C.fit_ref()
    (W64, h64, ran64, _), (W32, h32, _, _) = r['f64'], r['f32']
    print('history', hist.tolist())
    assert ran == ran64 == C.FIT['epochs']
    assert hist.shape == (C.FIT['epochs'], 5) and np.isfinite(hist).all()
    for col, name in enumerate(('loss', 'acc', 'val_loss', 'val_acc', 'lr')):
        C.check_d32(name, hist[:, col], h64[:, col], h32[:, col])
    got = C.unpack(out)
    C.check_updates(c['W'], got, W64, C.fit_lr_sum(c, C.FIT), 'fit')
    for name, _, role in SPEC:
        if ref.is_frozen(role):
            C.check_d32('moving ' + name, got[name], W64[name], W32[name])
        # (a bias in front of a BatchNorm on batch statistics has no gradient: it stays)
        if np.abs(W64[name] - c['W'][name]).max() > 2.0 ** -20 * np.abs(c['W'][name]).max():
            assert (got[name] != c['W'][name]).any(), f'{name} did not move'


def test_fit_is_bit_reproducible_and_zero_epochs_is_the_identity(ctx, fitted):
    c = C.fit_case()
    out, hist, ran = _fit(ctx, c, C.FIT)
    assert out.tobytes() == fitted[0].tobytes() and hist.tobytes() == fitted[1].tobytes() and ran == fitted[2]
    same, h0, ran0 = _fit(ctx, c, C.FIT, epochs=0)
    assert same.tobytes() == C.pack(c['W']).tobytes() and h0.shape == (0, 5) and ran0 == 0


def test_device_pointers_match_the_host_calls(ctx, fitted):
    import torch
    c = C.fit_case()
    blob = C.pack(c['W'])
    n, nv, ep, h, w = (C.FIT[k] for k in ('n_train', 'n_val', 'epochs', 'h', 'w'))
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
           for k, v in dict(blob=blob, img=c['img'], labels=c['labels'], val_img=c['val_img'],
                            val_labels=c['val_labels'], perm=c['perm'], masks=c['masks']).items()}
    out = torch.zeros(blob.size, dtype=torch.float32, device='cuda')
    hist = torch.zeros((ep, 5), dtype=torch.float32, device='cuda')
    ran = torch.zeros(1, dtype=torch.int32, device='cuda')
    loss = torch.zeros(1, dtype=torch.float32, device='cuda')
    grad = torch.ones(blob.size, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.od_finetune_dev(dev['blob'].data_ptr(), blob.size, dev['img'].data_ptr(), dev['labels'].data_ptr(), n,
                        dev['val_img'].data_ptr(), dev['val_labels'].data_ptr(), nv, h, w, C.CLASS_W, ep,
                        C.FIT['batch'], c['lr'], dev['perm'].data_ptr(), dev['masks'].data_ptr(), 0,
                        out.data_ptr(), hist.data_ptr(), ran.data_ptr())
    ctx.od_loss_grad_dev(dev['blob'].data_ptr(), blob.size, dev['img'].data_ptr(), dev['labels'].data_ptr(), 4, h,
                         w, C.CLASS_W, dev['masks'].data_ptr(), loss.data_ptr(), grad.data_ptr())
    ctx.synchronize()
    assert out.cpu().numpy().tobytes() == fitted[0].tobytes()
    assert hist.cpu().numpy().tobytes() == fitted[1].tobytes()
    assert int(ran.cpu()[0]) == fitted[2]
    assert dev['blob'].cpu().numpy().tobytes() == blob.tobytes(), 'the input blob was written'
    want_loss, want_grad = ctx.od_loss_grad(blob, c['img'][:4], c['labels'][:4], C.CLASS_W, c['masks'][0, :4])
    assert loss.cpu().numpy().tobytes() == want_loss.tobytes()
    assert grad.cpu().numpy().tobytes() == want_grad.tobytes()


# ---- 4. early stopping ----------------------------------------------------------------------------------

def test_early_stopping_ends_the_fit_where_the_restatement_does(ctx):
    c = C.stop_case()
    r = C.stop_ref()
    (_, h64, ran64, _), (_, h32, _, _) = r['f64'], r['f32']
    assert ran64 < C.STOP['epochs'], 'the case no longer stops early'
    out, hist, ran = _fit(ctx, c, C.STOP, patience=C.STOP['patience'])
    print('history', hist.tolist(), 'epochs_run', ran, 'restatement', ran64)
    assert ran == ran64
    assert np.isfinite(hist[:ran]).all() and np.isnan(hist[ran:]).all()
    C.check_d32('val_loss', hist[:ran, 2], h64[:ran, 2], h32[:ran, 2])
    # without a validation set, and with patience 0, the fit runs every epoch
    _, h_off, ran_off = _fit(ctx, c, C.STOP, patience=0)
    assert ran_off == C.STOP['epochs'] and np.isfinite(h_off).all()
    assert h_off[:ran].tobytes() == hist[:ran].tobytes()


# ---- 5. arguments ---------------------------------------------------------------------------------------

def test_invalid_arguments_are_rejected_and_the_loaded_model_is_untouched(ctx):
    c = C.fit_case()
    blob = C.pack(c['W'])
    n, nv, ep, h, w = (C.FIT[k] for k in ('n_train', 'n_val', 'epochs', 'h', 'w'))
    ctx.load_weights(weights.OD, C.pack(C.synthetic(9)), 2)
    probe = C.images(77, 3, 128, 151)[0]
    before = ctx.od_forward(probe)
    out = np.empty_like(blob)
    hist = np.empty((ep, 5), np.float32)
    loss = np.empty(1, np.float32)
    ran = np.zeros(1, np.int32)
    cw = np.array(C.CLASS_W, np.float32)
    img, lab = np.ascontiguousarray(c['img']), np.ascontiguousarray(c['labels'])
    vi, vl = np.ascontiguousarray(c['val_img']), np.ascontiguousarray(c['val_labels'])
    perm, masks, lr = (np.ascontiguousarray(c[k]) for k in ('perm', 'masks', 'lr'))
    p = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    good = dict(packed=blob, n_floats=blob.size, img=img, labels=lab, n=n, vi=vi, vl=vl, nv=nv, h=h, w=w, cw=cw,
                epochs=ep, batch=4, lr=lr, perm=perm, masks=masks, patience=0, out=out, hist=hist, ran=ran,
                loss=loss)

    def fit_rc(**over):
        a = dict(good, **over)
        return ctx.lib.mmla_od_finetune(ctx.h, p(a['packed']), a['n_floats'], p(a['img']), p(a['labels']), a['n'],
                                        p(a['vi']), p(a['vl']), a['nv'], a['h'], a['w'], p(a['cw']), a['epochs'],
                                        a['batch'], p(a['lr']), p(a['perm']), p(a['masks']), a['patience'],
                                        p(a['out']), p(a['hist']), p(a['ran']), 0)

    def grad_rc(**over):
        a = dict(good, **over)
        return ctx.lib.mmla_od_loss_grad(ctx.h, p(a['packed']), a['n_floats'], p(a['img']), p(a['labels']), a['n'],
                                         a['h'], a['w'], p(a['cw']), None, p(a['loss']), p(a['out']), None, 0)

    bad_label = lab.copy()
    bad_label[2] = 2
    twice = perm.copy()
    twice[1, 0] = twice[1, 1]
    bad_lr = lr.copy()
    bad_lr[1] = np.nan
    neg_lr = lr.copy()
    neg_lr[0] = -1e-3
    cases = [dict(n_floats=blob.size - 1), dict(h=7), dict(h=129), dict(w=7), dict(w=152), dict(batch=0),
             dict(batch=_lib.OD_TRAIN_MAX_BATCH + 1, n=_lib.OD_TRAIN_MAX_BATCH + 1), dict(n=0), dict(nv=-1),
             dict(epochs=-1), dict(patience=-1), dict(packed=None), dict(img=None), dict(labels=None),
             dict(out=None), dict(perm=None), dict(hist=None), dict(lr=None), dict(vi=None), dict(vl=None),
             dict(cw=None), dict(ran=None), dict(cw=np.array([np.inf, 1], np.float32)),
             dict(cw=np.array([1, -0.5], np.float32)), dict(lr=bad_lr), dict(lr=neg_lr), dict(labels=bad_label),
             dict(perm=twice)]
    for over in cases:
        assert fit_rc(**over) == -1, over
    for over in (dict(n_floats=blob.size + 1), dict(h=7), dict(w=152), dict(n=0),
                 dict(n=_lib.OD_TRAIN_MAX_BATCH + 1), dict(packed=None), dict(img=None), dict(labels=None),
                 dict(out=None), dict(loss=None), dict(cw=None), dict(cw=np.array([np.nan, 1], np.float32)),
                 dict(labels=bad_label)):
        assert grad_rc(**over) == -1, over
    assert fit_rc() == 0 and grad_rc() == 0          # the context still works, and the good call is good
    after = ctx.od_forward(probe)
    assert np.asarray(after).tobytes() == np.asarray(before).tobytes(), 'a fit changed the loaded model'


# ---- 6. Python ------------------------------------------------------------------------------------------

def test_cosine_lr_and_class_weights_match_the_script():
    import math
    lr = overlap_detector.cosine_lr(7)
    for e in range(7):
        assert lr[e] == 1e-4 + (1e-2 - 1e-4) * (1 + math.cos(math.pi * e / 100)) / 2
    assert overlap_detector.cosine_lr(3, T_max=2, eta_max=1.0, eta_min=0.0).tolist() == \
        [1.0, (1 + math.cos(math.pi / 2)) / 2, 0.0]
    y = np.eye(2)[[0, 0, 0, 1]]
    assert overlap_detector.cal_weighted_penalty(y).tolist() == [1 - 3 / 4, 1 - 1 / 4]


def test_continue_train_is_the_c_call_on_its_plan(ctx):
    c = C.fit_case()
    img = np.concatenate([c['img'], c['val_img']])
    labels = np.concatenate([c['labels'], c['val_labels']])
    plan = overlap_detector.fit_plan(labels, 3, 2)
    tr, va = plan['train'], plan['val']
    assert len(va) and not set(tr) & set(va) and plan['perm'].shape == (2, len(tr))
    assert plan['drop_mask'].shape == (2, len(tr), 512) and 0.2 < 1 - plan['drop_mask'].mean() < 0.3
    W1, hist, ran = overlap_detector.continue_train(c['W'], img, labels, plan, 2, 4, weighted=True, patience=0,
                                                    device=ctx)
    cw = overlap_detector.cal_weighted_penalty(np.eye(2)[labels[tr]])
    out, h2, ran2 = ctx.od_finetune(C.pack(c['W']), img[tr], labels[tr], img[va], labels[va], cw,
                                    overlap_detector.cosine_lr(2), plan['perm'], plan['drop_mask'], 2, 4, 0)
    assert C.pack(W1).tobytes() == out.tobytes() and hist.tobytes() == h2.tobytes() and ran == ran2 == 2
