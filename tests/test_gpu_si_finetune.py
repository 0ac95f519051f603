"""GPU: speaker registration stage 2 -- mmla_si_loss_grad and mmla_si_finetune (si_bwd.hip) against the
torch-CPU restatement with autograd (tests/si_finetune_ref.py), then transfer_learning(fine_tune=True)
and Room.register(fine_tune=True) end to end.

The bounds are the two rules of tests/si_finetune_cases.py: every loss, gradient tensor and history
column within 16 x d32 of the helper's float64 run (d32 = the helper's own float32 deviation on the
same inputs, floor 16 x 2^-24 x max|ref|), and fitted weights compared as updates.  The inputs'
conditions (ReLU / pool margins of the gradient seed, the float32 helper inside the update cap) are
asserted on the CPU in tests/test_si_finetune_ref_cpu.py."""
import json
import os
import warnings

import numpy as np
import pytest

import cond_ref
import enrol_inputs
import si_finetune_cases as C
import si_finetune_ref as ref
from mmla_audio_amd import _lib, models, room, tfbundle, weights
from mmla_audio_amd import speaker_identification as si

pytestmark = pytest.mark.gpu

K = C.K
SPEC = weights.si_spec(K)
HEAD = 'layer_with_weights-42'


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _pack(W):
    return weights.pack(weights.SI, W, K)


# ---- 1. gradient ------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [2, 1])
def test_loss_and_gradient_vs_autograd(ctx, B):
    W, x, labels = C.grad_case(B)
    r = C.grad_ref(B)
    (d64, r64, g64), (d32, r32, g32) = r['f64'], r['f32']
    loss, grad = ctx.si_loss_grad(_pack(W), K, x, labels)
    C.check_d32('data term', loss[0], d64, d32)
    C.check_d32('R', loss[1], r64, r32)
    g = C.unpack(grad)
    for name, _, role in SPEC:
        if ref.is_frozen(role):
            assert not g[name].any(), f'{name}: the gradient slot of a moving statistic is not 0'
        else:
            C.check_d32(name, g[name], g64[name], g32[name])


# ---- 2. clip and L2 ---------------------------------------------------------------------------------

def test_clipped_samples_leave_only_the_penalty(ctx):
    W, x, _ = C.grad_case(2)
    W = dict(W)
    c = 1
    b = W[HEAD + '/bias'].copy()
    b[c] = -40.0                                   # s_c ~ e^-40: p_c far below the clip's 1e-7
    W[HEAD + '/bias'] = b
    loss, grad = ctx.si_loss_grad(_pack(W), K, x, np.full(2, c, np.int32))
    clipped = np.float32(-np.log(np.float64(np.float32(1e-7))))
    assert abs(float(loss[0]) - float(clipped)) <= float(np.spacing(clipped)), loss
    r64 = sum(lam * float((W[n].astype(np.float64) ** 2).sum()) for n, lam in ref.L2_NAMES.items())
    assert abs(float(loss[1]) - r64) <= 2.0 ** -23 * r64, (loss, r64)
    g = C.unpack(grad)
    for name, _, _ in SPEC:
        if name in ref.L2_NAMES:
            want = 2.0 * ref.L2_NAMES[name] * W[name].astype(np.float64)
            # one rounding of the product, plus that of the float32 constant 2 * lambda
            assert np.all(np.abs(g[name] - want) <= 2.0 ** -23 * np.abs(want)), name
            assert g[name].any()
        else:
            assert not g[name].any(), f'{name}: a gradient without a data term'


# ---- 3. fit -------------------------------------------------------------------------------------------

def _fit(ctx, c, epochs=None):
    epochs = C.FIT['epochs'] if epochs is None else epochs
    return ctx.si_finetune(_pack(c['W']), K, c['x'], c['labels'], c['val_x'], c['val_labels'],
                           c['perm'][:epochs], epochs, C.FIT['batch'], C.FIT['lr'])


@pytest.fixture(scope='module')
def fitted(ctx):
    out, hist = _fit(ctx, C.fit_case())
    out.setflags(write=False)
    hist.setflags(write=False)
    return out, hist


def test_fit_history_and_updates(ctx, fitted):
    c = C.fit_case()
    out, hist = fitted
    r = C.fit_ref()
    (W64, h64, _), (W32, h32, _) = r['f64'], r['f32']
    print('history', hist.tolist())
    assert hist.shape == (C.FIT['epochs'], 4) and np.isfinite(hist).all()
    for col, name in enumerate(('loss', 'acc', 'val_loss', 'val_acc')):
        C.check_d32(name, hist[:, col], h64[:, col], h32[:, col])
    got = C.unpack(out)
    C.check_updates(c['W'], got, W64, 'kernel')
    moved = 0
    for name, _, role in SPEC:
        if ref.is_frozen(role):
            assert got[name].tobytes() == c['W'][name].tobytes(), f'{name} moved'
        else:
            moved += int((got[name] != c['W'][name]).any())
    assert moved == sum(not ref.is_frozen(role) for _, _, role in SPEC), 'a trainable tensor did not move'


def test_fit_is_bit_reproducible_and_zero_epochs_is_the_identity(ctx, fitted):
    c = C.fit_case()
    out, hist = _fit(ctx, c)
    assert out.tobytes() == fitted[0].tobytes() and hist.tobytes() == fitted[1].tobytes()
    same, h0 = _fit(ctx, c, epochs=0)
    assert same.tobytes() == _pack(c['W']).tobytes() and h0.shape == (0, 4)


def test_fit_without_a_validation_set(ctx, fitted):
    c = C.fit_case()
    out, hist = ctx.si_finetune(_pack(c['W']), K, c['x'], c['labels'], None, None, c['perm'],
                                C.FIT['epochs'], C.FIT['batch'], C.FIT['lr'])
    assert out.tobytes() == fitted[0].tobytes()
    assert hist[:, :2].tobytes() == fitted[1][:, :2].tobytes() and np.isnan(hist[:, 2:]).all()


def test_device_pointers_match_the_host_calls(ctx, fitted):
    import torch
    c = C.fit_case()
    blob = _pack(c['W'])
    n, nv, ep = C.FIT['n_train'], C.FIT['n_val'], C.FIT['epochs']
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
           for k, v in dict(blob=blob, x=c['x'], labels=c['labels'], val_x=c['val_x'],
                            val_labels=c['val_labels'], perm=c['perm']).items()}
    out = torch.zeros(blob.size, dtype=torch.float32, device='cuda')
    hist = torch.zeros((ep, 4), dtype=torch.float32, device='cuda')
    loss = torch.zeros(2, dtype=torch.float32, device='cuda')
    grad = torch.ones(blob.size, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.si_finetune_dev(dev['blob'].data_ptr(), blob.size, K, dev['x'].data_ptr(), dev['labels'].data_ptr(), n,
                        dev['val_x'].data_ptr(), dev['val_labels'].data_ptr(), nv, ep, C.FIT['batch'],
                        C.FIT['lr'], dev['perm'].data_ptr(), out.data_ptr(), hist.data_ptr())
    ctx.si_loss_grad_dev(dev['blob'].data_ptr(), blob.size, K, dev['x'].data_ptr(), dev['labels'].data_ptr(), n,
                         loss.data_ptr(), grad.data_ptr())
    ctx.synchronize()
    assert out.cpu().numpy().tobytes() == fitted[0].tobytes()
    assert hist.cpu().numpy().tobytes() == fitted[1].tobytes()
    assert dev['blob'].cpu().numpy().tobytes() == blob.tobytes(), 'the input blob was written'
    want_loss, want_grad = ctx.si_loss_grad(blob, K, c['x'], c['labels'])
    assert loss.cpu().numpy().tobytes() == want_loss.tobytes()
    assert grad.cpu().numpy().tobytes() == want_grad.tobytes()


def test_invalid_arguments_are_rejected(ctx):
    c = C.fit_case()
    blob = _pack(c['W'])
    n, nv, ep = C.FIT['n_train'], C.FIT['n_val'], C.FIT['epochs']
    out = np.empty_like(blob)
    hist = np.empty((ep, 4), np.float32)
    loss = np.empty(2, np.float32)
    x, lab = np.ascontiguousarray(c['x']), np.ascontiguousarray(c['labels'])
    vx, vl = np.ascontiguousarray(c['val_x']), np.ascontiguousarray(c['val_labels'])
    perm = np.ascontiguousarray(c['perm'])
    p = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    good = dict(packed=blob, n_floats=blob.size, k=K, x=x, labels=lab, n=n, vx=vx, vl=vl, nv=nv, epochs=ep,
                batch=2, perm=perm, out=out, hist=hist)

    def fit_rc(**over):
        a = dict(good, **over)
        return ctx.lib.mmla_si_finetune(ctx.h, p(a['packed']), a['n_floats'], a['k'], p(a['x']), p(a['labels']),
                                        a['n'], p(a['vx']), p(a['vl']), a['nv'], a['epochs'], a['batch'], 1e-6,
                                        p(a['perm']), p(a['out']), p(a['hist']), 0)

    def grad_rc(**over):
        a = dict(good, **over)
        return ctx.lib.mmla_si_loss_grad(ctx.h, p(a['packed']), a['n_floats'], a['k'], p(a['x']), p(a['labels']),
                                         a['n'], p(loss), p(a['out']), 0)

    bad_label = lab.copy()
    bad_label[2] = K
    twice = perm.copy()
    twice[1, 0] = twice[1, 1]
    cases = [dict(k=0), dict(k=_lib.SI_TRAIN_MAX_CLASSES + 1), dict(n_floats=blob.size - 1),
             dict(n_floats=weights.n_params(weights.SI, K + 1)), dict(batch=0), dict(n=0), dict(nv=-1),
             dict(epochs=-1), dict(packed=None), dict(x=None), dict(labels=None), dict(out=None),
             dict(perm=None), dict(vx=None), dict(labels=bad_label), dict(perm=twice)]
    for over in cases:
        assert fit_rc(**over) == -1, over
    for over in (dict(k=0), dict(n_floats=blob.size + 1), dict(n=0), dict(packed=None), dict(x=None),
                 dict(labels=None), dict(out=None), dict(labels=bad_label)):
        assert grad_rc(**over) == -1, over
    assert fit_rc() == 0 and grad_rc() == 0          # the context still works, and the good call is good


# ---- 4. transfer_learning(fine_tune=True) ----------------------------------------------------------------

EPOCHS1 = 30


def _tl_inputs():
    rng = np.random.default_rng(404)
    x = (rng.standard_normal((12, 256, 39)) * 10).astype(np.float32)
    labels = np.repeat(np.arange(K, dtype=np.int32), 4)
    return x, labels, np.eye(K)[labels]


def test_transfer_learning_fine_tune(ctx, tmp_path):
    x, labels, y = _tl_inputs()
    base_dir = str(tmp_path / 'timit' / 'model')
    final, plain = str(tmp_path / 'tuned'), str(tmp_path / 'plain')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # synthetic base weights
        acc = si.transfer_learning(x, y, 1, 0, base_dir, final, epochs=EPOCHS1, allow_synthetic=True,
                                   device=ctx, fine_tune=True, fine_tune_epochs=2)
        acc0 = si.transfer_learning(x, y, 1, 0, base_dir, plain, epochs=EPOCHS1, allow_synthetic=True,
                                    device=ctx)
        base = models.load_model(base_dir, kind=weights.SI, allow_synthetic=True, device=ctx)
    # the composition: stage 1 as fit_registration runs it, then mmla_si_finetune on its plan
    fit = si.fit_registration(base.ctx.si_embed(x), labels, K, 1, 0, EPOCHS1, 1, ctx, 2)
    plan = fit.plan
    tr, va = plan['train'], plan['val']
    assert len(va) and plan['perm2'].shape == (2, len(tr))
    W1 = si.deployed_weights(base.W, fit.w, fit.b)
    out, hist = ctx.si_finetune(_pack(W1), K, x[tr], labels[tr], x[va], labels[va], plan['perm2'], 2)
    want = C.unpack(out)
    saved = tfbundle.load_bundle(final)
    deployed = models.load_model(final, device=ctx)
    assert (deployed.n_classes, deployed.head) == (K, _lib.HEAD_SIGMOID)
    changed = []
    for name, _, role in SPEC:
        assert deployed.W[name].tobytes() == want[name].tobytes(), name
        if ref.is_frozen(role):
            assert deployed.W[name].tobytes() == base.W[name].tobytes(), name
        elif not name.startswith(HEAD) and (deployed.W[name] != base.W[name]).any():
            changed.append(name)
    assert set(ref.L2_NAMES) <= set(changed), 'a regularised kernel equals the base\'s'
    assert acc == float(hist[-1, 3]) and acc0 == fit.accuracy
    assert len(saved) >= len(SPEC)
    # stage 1 inside a fine-tuned registration is the stage-1-only run, and without the flag the base
    # is saved as loaded
    off = models.load_model(plain, device=ctx)
    for name, _, _ in SPEC[:-2]:
        assert off.W[name].tobytes() == base.W[name].tobytes(), name
    for t in ('/kernel', '/bias'):
        assert off.W[HEAD + t].tobytes() == W1[HEAD + t].tobytes()


# ---- 5. Room.register(fine_tune=True) ----------------------------------------------------------------------

def test_room_register_fine_tune(tmp_path):
    n = 8 * 16000
    recs = [enrol_inputs.voiced(110.0, 80, n, [(30000, 50000)]),
            enrol_inputs.voiced(165.0, 81, n, [(64000, 90000)])]
    noises = [cond_ref.noise(0), cond_ref.noise(1)]
    base_dir = str(tmp_path / 'timit' / 'model')
    save_to = str(tmp_path / 'room_model')

    def make(si_dir=None):
        c = _lib.Context(0)
        od = models.OverlapDetectionModel(weights.synthetic(weights.OD, seed=81), device=c)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m = (models.load_model(base_dir, kind=weights.SI, allow_synthetic=True, device=c)
                 if si_dir is None else models.load_model(si_dir, device=c))
        return room.Room(od, m, noises)

    r, twin = make(), None
    try:
        base_W = r.si.W
        reg = r.register(recs, ['ft_anna', 'ft_bo'], mic=[0, 1], epochs=20, save_to=save_to, fine_tune=True,
                         fine_tune_epochs=1)
        print('n_windows', reg.n_windows.tolist(), 'accuracy', reg.accuracy, 'history', reg.fine_tune_history)
        assert reg.fine_tune_history.shape == (1, 4) and reg.history.shape == (1, 20, 4)
        assert reg.accuracy == float(reg.fine_tune_history[-1, 3])
        assert len(tuple(reg)) == 6 and reg[:2] == (reg.speaker_id_dict, reg.accuracy)
        assert (r.si.n_classes, r.si.head, r.ctx.si_classes) == (2, _lib.HEAD_SIGMOID, 2)
        assert json.load(open(os.path.join(save_to, 'speaker_id_dict.json'))) == {'0': 'ft_anna', '1': 'ft_bo'}
        name = 'layer_with_weights-37/kernel'
        assert (r.si.W[name] != base_W[name]).any()
        twin = make(save_to)
        assert twin.si.W[name].tobytes() == r.si.W[name].tobytes()
        x = cond_ref.clips()
        mic = np.array([0, 1, 0, 1, 0, 1], np.int32)
        got, want = r.tick(x, mic=mic), twin.tick(x, mic=mic)
        assert got.si_probs.shape == (6, 2)
        assert got.si_probs.tobytes() == want.si_probs.tobytes()
        assert got.si_argmax.tobytes() == want.si_argmax.tobytes()
    finally:
        r.ctx.close()
        if twin is not None:
            twin.ctx.close()
