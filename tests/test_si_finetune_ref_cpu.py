"""CPU: the stage-2 restatement (tests/si_finetune_ref.py) is tied to what is already pinned -- its forward
to oracle.nets, its gradient to central differences, its fit with a frozen base and no penalty to
tests/si_head_ref.py -- and the committed inputs of tests/test_gpu_si_finetune.py satisfy the conditions
their comparison rules need.  Also the Python plumbing that needs no device: the plan, unpack, the ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import si_finetune_cases as C
import si_finetune_ref as ref
import si_head_ref
from mmla_audio_amd import _lib, room, weights
from mmla_audio_amd import speaker_identification as si
from oracle import nets

K = C.K
SPEC = weights.si_spec(K)


def test_forward_equals_the_oracle():
    W, x, _ = C.grad_case(2)
    want = nets.si_forward(x.astype(np.float64), W, head='sigmoid', dtype=np.float64)
    got = ref.forward(W, x, torch.float64)
    assert got.shape == (2, K)
    assert np.max(np.abs(got - want)) <= 1e-10


def _loss64(W, x, labels):
    with torch.no_grad():
        net = ref._Net(W, torch.float64)
        loss, _, _ = ref._data_terms(net.sigmoids(x), labels, torch.float64)
        return float(loss.mean() + net.penalty())


def test_gradient_agrees_with_central_differences():
    W, x, labels = C.grad_case(2)
    _, _, g = C.grad_ref(2)['f64']
    W64 = {k: np.asarray(v, np.float64) for k, v in W.items()}
    rng = np.random.default_rng(9)
    picks = {           # one tensor of every role, the ones the issue names among them
        'layer_with_weights-0/kernel': 'stem kernel', 'layer_with_weights-0/bias': 'stem bias',
        'layer_with_weights-20/kernel': 'L2 kernel', 'layer_with_weights-37/kernel': 'L2 kernel',
        'layer_with_weights-21/gamma': 'BN gamma', 'layer_with_weights-21/beta': 'BN beta',
        'layer_with_weights-40/gamma': 'final BN gamma',
        'layer_with_weights-17/kernel': 'shortcut kernel', 'layer_with_weights-17/bias': 'shortcut bias',
        'layer_with_weights-41/forward/kernel': 'LSTM kernel',
        'layer_with_weights-41/forward/recurrent_kernel': 'LSTM recurrent',
        'layer_with_weights-41/backward/recurrent_kernel': 'LSTM recurrent',
        'layer_with_weights-41/backward/bias': 'LSTM bias',
        'layer_with_weights-42/kernel': 'head kernel', 'layer_with_weights-42/bias': 'head bias'}
    for name, what in picks.items():
        flat = g[name].ravel()
        # the largest-gradient entry and a random one
        for at in {int(np.argmax(np.abs(flat))), int(rng.integers(flat.size))}:
            # small enough that no ReLU or pool of the batch changes side (the seed's margins are ~1e-4)
            h = 1e-7 * max(1.0, abs(W64[name].ravel()[at]))
            vals = []
            for sgn in (1.0, -1.0):
                Wp = dict(W64)
                t = W64[name].copy()
                t.ravel()[at] += sgn * h
                Wp[name] = t
                vals.append(_loss64(Wp, x, labels))
            fd = (vals[0] - vals[1]) / (2 * h)
            # 5e-7: the rounding of a loss of ~130 (R dominates it) over a step of 2e-7
            tol = 1e-5 * max(abs(fd), float(np.max(np.abs(flat)))) + 5e-7
            assert abs(fd - flat[at]) <= tol, f'{what} {name}[{at}]: autograd {flat[at]:.9e}, differences {fd:.9e}'
    for name, _, role in SPEC:
        if ref.is_frozen(role):
            assert not g[name].any()


def test_frozen_base_without_penalty_is_stage_one():
    c = C.fit_case()
    W = c['W']
    kw = dict(epochs=3, batch=2, lr=1e-4)
    rng = np.random.default_rng(3)
    perm = np.stack([rng.permutation(5) for _ in range(3)])
    Wf, hist, _ = ref.fit(W, K, c['x'], c['labels'], c['val_x'], c['val_labels'], perm, dtype=torch.float64,
                          frozen_base=True, penalty=False, **kw)
    with torch.no_grad():
        net = ref._Net(W, torch.float64)
        emb, val_emb = net.embed(c['x']).numpy(), net.embed(c['val_x']).numpy()
    w, b, h, _ = si_head_ref.fit(emb, c['labels'], val_emb, c['val_labels'], W['layer_with_weights-42/kernel'],
                                 W['layer_with_weights-42/bias'], perm, dtype=np.float64, **kw)
    assert np.max(np.abs(Wf['layer_with_weights-42/kernel'] - w)) <= 1e-12
    assert np.max(np.abs(Wf['layer_with_weights-42/bias'] - b)) <= 1e-12
    assert np.max(np.abs(hist - h)) <= 1e-10
    for name, _, _ in SPEC[:-2]:
        assert np.array_equal(Wf[name], np.asarray(W[name], np.float64)), name


def test_committed_inputs_meet_their_conditions():
    for B in (2, 1):
        W, x, labels = C.grad_case(B)
        relu, pool, gap = ref.margins(W, K, x, labels)
        print(f'B = {B}: margins relu {relu:.3e}  pool {pool:.3e}  sigmoid gap {gap:.3e}')
        assert relu >= C.MARGIN and pool >= C.MARGIN and gap >= C.MARGIN
    c = C.fit_case()
    r = C.fit_ref()
    assert len(set(c['labels'].tolist())) > 1 and C.FIT['n_train'] % C.FIT['batch'] != 0   # a short last batch
    C.check_updates(c['W'], r['f32'][0], r['f64'][0], 'helper float32')
    assert r['f64'][2]['gap'] >= C.MARGIN                  # the accuracy columns cannot flip
    assert np.array_equal(r['f64'][1][:, [1, 3]], r['f32'][1][:, [1, 3]])
    for name, _, role in SPEC:
        if ref.is_frozen(role):
            assert np.array_equal(r['f64'][0][name], np.asarray(c['W'][name], np.float64))


def test_stage_two_plan_leaves_stage_one_draws():
    labels = np.repeat(np.arange(3), 5)
    for ratio in (0, 0.2):
        a = si._fit_plan(labels, 3, 7, ratio, 4, 2)
        b = si._fit_plan(labels, 3, 7, ratio, 4, 2, fine_tune_epochs=3)
        for key in ('train', 'val', 'test', 'w0', 'b0', 'perm'):
            assert a[key].tobytes() == b[key].tobytes(), key
        n = len(b['train'])
        assert a['perm2'].shape == (0, n) and b['perm2'].shape == (3, n) and b['perm2'].dtype == np.int32
        assert all(sorted(row) == list(range(n)) for row in b['perm2'].tolist())
        assert len({row.tobytes() for row in b['perm2']}) == 3
        # more epochs extend the orders, they do not redraw them
        assert si._fit_plan(labels, 3, 7, ratio, 4, 2, 5)['perm2'][:3].tobytes() == b['perm2'].tobytes()


def test_unpack_inverts_pack():
    W = C.synthetic(0)
    blob = weights.pack(weights.SI, W, K)
    back = weights.unpack(weights.SI, blob, K)
    assert sorted(back) == sorted(W)
    for name, shape, _ in SPEC:
        assert back[name].shape == tuple(shape) and back[name].tobytes() == W[name].tobytes()
    assert weights.pack(weights.SI, back, K).tobytes() == blob.tobytes()
    with pytest.raises(ValueError):
        weights.unpack(weights.SI, blob[:-1], K)


def test_abi_and_keywords():
    import inspect
    assert 'mmla_si_loss_grad' in _lib.SIGNATURES and 'mmla_si_finetune' in _lib.SIGNATURES
    for fn in (si.transfer_learning, room.Room.register):
        p = inspect.signature(fn).parameters
        assert p['fine_tune'].default is False and p['fine_tune_epochs'].default == 20
    assert room.Registration._fields[-1] == 'fine_tune_history'
    assert room.Registration({}, 1.0, None, None, None).fine_tune_history is None
    if not os.path.exists(_lib.LIB_PATH):       # not built: the keyword half above still stands
        return
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mmla_si_loss_grad', 'mmla_si_finetune'):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = _lib.SIGNATURES[name]
    assert lib.mmla_si_loss_grad(None, None, 0, 0, None, None, 0, None, None, 0) == -1
    assert lib.mmla_si_finetune(None, None, 0, 0, None, None, 0, None, None, 0, 0, 0, 0.0, None, None, None,
                                0) == -1
