"""CPU: the base-training restatement (tests/si_base_ref.py) is tied to what is already pinned -- its Philox
to a second, scalar restatement and the published known answer, its training-mode forward to
tests/si_finetune_ref.py -- and the committed inputs of tests/test_gpu_si_base.py satisfy the conditions their
comparison rules need.  Also the Python plumbing that needs no device: the initial state, the base-model
writer, the ABI."""
import ctypes
import os

import numpy as np
import torch

import si_base_cases as C
import si_base_ref as ref
import si_finetune_cases as FC
import si_finetune_ref as ft
from mmla_audio_amd import _lib, tfbundle, weights
from mmla_audio_amd import speaker_identification as si

HERE = os.path.dirname(os.path.abspath(__file__))


def _philox_scalar(counter, key):
    """Philox4x32-10 once more, with Python integers, written from the paper's round function: multiply
    the 1st and 3rd words by the two constants, swap the halves into place with the key xored in, bump the
    key by the Weyl constants between rounds"""
    x0, x1, x2, x3 = (int(v) for v in counter)
    k0, k1 = (int(v) for v in key)
    for rnd in range(10):
        if rnd:
            k0 = (k0 + 0x9E3779B9) % 2 ** 32
            k1 = (k1 + 0xBB67AE85) % 2 ** 32
        a = 0xD2511F53 * x0
        b = 0xCD9E8D57 * x2
        x0, x1, x2, x3 = (b // 2 ** 32) ^ x1 ^ k0, b % 2 ** 32, (a // 2 ** 32) ^ x3 ^ k1, a % 2 ** 32
    return [x0, x1, x2, x3]


def test_philox_two_restatements_and_the_known_answer():
    rng = np.random.default_rng(11)
    counters = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64).astype(np.uint32)
    keys = rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint64).astype(np.uint32)
    got = ref.philox4x32_10(counters, keys)
    for i in range(1000):
        assert got[i].tolist() == _philox_scalar(counters[i], keys[i]), i
    # Random123's known answer for the all-zero counter and key
    zero = ref.philox4x32_10(np.zeros((1, 4), np.uint32), np.zeros((1, 2), np.uint32))[0].tolist()
    assert zero == _philox_scalar([0] * 4, [0] * 2)
    assert zero == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def test_keep_rates():
    n = 2 ** 20
    a, _ = ref.drop_masks(C.DROP_SEED, 1, np.arange(n // ref.MAP))
    _, b = ref.drop_masks(C.DROP_SEED, 1, np.arange(n // ref.EMB))
    assert a.size == n and b.size == n
    assert abs(a.mean() - 0.75) <= 0.002 and abs(b.mean() - 0.8) <= 0.002
    # the sample id, the epoch and the site each change the bits; the slot in the batch does not
    a0, b0 = ref.drop_masks(C.DROP_SEED, 1, [3, 9])
    a1, b1 = ref.drop_masks(C.DROP_SEED, 1, [9, 3])
    assert (a0[0] == a1[1]).all() and (b0[1] == b1[0]).all() and (a0[0] != a0[1]).any()
    assert (ref.drop_masks(C.DROP_SEED, 2, [3])[0] != a0[0]).any()
    assert (ref.drop_words(C.DROP_SEED, 1, [3], 0, 512) != ref.drop_words(C.DROP_SEED, 1, [3], 1, 512)).any()


def test_training_mode_equals_the_pinned_forward_when_the_statistics_agree():
    W, x, _, _, _ = C.grad_case(2, 3)
    _, emb, stats = ref.train_forward(W, x)            # dropout off, BN on the batch's statistics
    W2 = dict(W)
    for k, (mean, var) in stats.items():                # the moving statistics := the batch's
        W2[f'layer_with_weights-{k}/moving_mean'] = mean
        W2[f'layer_with_weights-{k}/moving_variance'] = var
    assert len(stats) == 19
    with torch.no_grad():
        want = ft._Net(W2, torch.float64).embed(x).numpy()
    assert np.max(np.abs(emb - want)) <= 1e-9 * max(1.0, float(np.max(np.abs(want))))
    # and all-ones masks only scale: the map by float32(1 / 0.75) ahead of the LSTM, the embedding by 1 / 0.8
    ones = (np.ones((2, 32, 128), np.uint8), np.ones((2, 512), np.uint8))
    _, emb1, _ = ref.train_forward(W, x, ones)
    assert np.max(np.abs(emb1)) > 0 and not np.allclose(emb1, emb)


def test_gradient_cases_have_their_margins():
    for B in (1, 2, 3):
        W, x, _, _, masks = C.grad_case(B, 3)
        relu, pool = ref.margins(W, x, masks)
        print(f'B = {B}: smallest ReLU margin {relu:.3e}, pool margin {pool:.3e}')
        assert relu >= C.MARGIN and pool >= C.MARGIN


def test_gradient_agrees_with_central_differences():
    B, K = 2, 3
    W, x, labels, _, masks = C.grad_case(B, K)
    _, _, g, moved = C.grad_ref(B, K)['f64']
    W64 = {k: np.asarray(v, np.float64) for k, v in W.items()}

    def loss64(Wv):
        with torch.no_grad():
            net = ref._TrainNet(Wv, torch.float64)
            net.training, net.masks = True, masks
            loss, _ = ref._data_terms(net.logits(x), labels)
            return float(loss.mean() + net.penalty())

    for name in ('layer_with_weights-0/kernel', 'layer_with_weights-21/gamma', 'layer_with_weights-21/beta',
                 'layer_with_weights-20/kernel', 'layer_with_weights-40/gamma',
                 'layer_with_weights-41/forward/kernel', 'layer_with_weights-42/kernel',
                 'layer_with_weights-42/bias'):
        at = int(np.argmax(np.abs(g[name].ravel())))
        h = 1e-7 * max(1.0, abs(W64[name].ravel()[at]))
        vals = []
        for sgn in (1.0, -1.0):
            Wp = dict(W64)
            t = W64[name].copy()
            t.ravel()[at] += sgn * h
            Wp[name] = t
            vals.append(loss64(Wp))
        num = (vals[0] - vals[1]) / (2 * h)
        assert abs(num - g[name].ravel()[at]) <= 1e-4 * max(abs(num), 1e-3), (name, num, g[name].ravel()[at])
    # a Conv1D bias has no gradient at all (autograd's own float64 values are rounding noise next to the
    # other tensors' gradients), the helper reports it as exactly 0; moving statistics: zero slots, and every
    # one of them advanced
    raw = ref.loss_and_grad(W, K, x, labels, masks, torch.float64, raw=True)[2]
    scale = max(float(np.max(np.abs(v))) for v in raw.values())
    dead = [n for n, _, role in weights.si_spec(K) if ref.is_dead(n, role)]
    assert len(dead) == 22 and 'layer_with_weights-42/bias' not in dead
    for name in dead:
        assert np.max(np.abs(raw[name])) <= 1e-9 * scale and not g[name].any(), name
    assert np.max(np.abs(g['layer_with_weights-42/bias'])) > 0
    for name, _, role in weights.si_spec(K):
        if ft.is_frozen(role):
            assert not g[name].any() and (moved[name] != W64[name]).all(), name
        else:
            assert (moved[name] == W64[name]).all(), name


def test_fit_case_is_inside_the_update_cap_and_decides_clearly():
    f = C.fit_ref()
    c = C.fit_case()
    C.check_updates(c['W'], f['f32'][0], f['f64'][0], 'helper float32', C.fit_steps(), C.FIT['lr'])
    h64, h32 = f['f64'][1], f['f32'][1]
    assert np.isfinite(h64).all() and f['f64'][2]['epochs_run'] == C.FIT['epochs']
    # the checkpoint decision: one checkpoint epoch (2 of 3), taken whatever the accuracy is; with more, the
    # accuracies compared must be apart by more than the d32 bound
    ck = [e for e in range(C.FIT['epochs']) if (e + 1) % C.FIT['ckpt_period'] == 0]
    acc = h64[ck, 3]
    bound = FC.d32_bound(h64[:, 3], h32[:, 3])
    for i in range(len(ck)):
        for j in range(i):
            assert abs(acc[i] - acc[j]) > bound or acc[i] == acc[j]
    assert f['f64'][2]['best_epoch'] == f['f32'][2]['best_epoch'] == ck[0] + int(np.argmax(acc)) * C.FIT['ckpt_period']


def test_stop_case_decides_clearly():
    s = C.stop_ref()
    v64, v32 = s['f64'][1][:, 2], s['f32'][1][:, 2]
    run = ref.early_stop_epochs(v64, C.STOP['patience'])
    print('val_loss', v64, 'epochs run', run)
    assert 1 < run < C.STOP['epochs'], 'the case is meant to stop early'
    assert ref.early_stop_epochs(v32, C.STOP['patience']) == run
    bound = FC.d32_bound(v64, v32)
    best = np.inf
    for ep in range(run):                       # every comparison the rule makes
        if np.isfinite(best):
            assert abs(v64[ep] - best) > bound, (ep, v64[ep], best, bound)
        best = min(best, v64[ep])


def test_initial_state():
    K = 630
    W = weights.initial(weights.SI, seed=3, n_classes=K)
    weights.check(weights.SI, W, K)
    for name, shape, role in weights.si_spec(K):
        w = W[name].astype(np.float64)
        assert W[name].dtype == np.float32
        if role in ('bias', 'bn_beta', 'bn_mean'):
            assert not w.any(), name
        elif role in ('bn_gamma', 'bn_var'):
            assert (w == 1.0).all(), name
        elif role == 'lstm_bias':
            assert (w[256:512] == 1.0).all() and not w[:256].any() and not w[512:].any(), name
        elif role == 'lstm_rec':
            assert np.max(np.abs(w @ w.T - np.eye(256))) <= 1e-6, name
        else:
            rf = int(np.prod(shape[:-2]))
            lim = np.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
            assert np.max(np.abs(w)) <= lim * (1 + 1e-6) and np.std(w) > 0.5 * lim, name
    again = weights.initial(weights.SI, seed=3, n_classes=K)
    other = weights.initial(weights.SI, seed=4, n_classes=K)
    assert all((W[k] == again[k]).all() for k in W)
    assert (W['layer_with_weights-0/kernel'] != other['layer_with_weights-0/kernel']).any()
    try:
        weights.initial(weights.OD)
    except NotImplementedError:
        pass
    else:
        raise AssertionError('OD has no from-scratch initial state')


def test_base_layout_is_the_reference_index(tmp_path):
    K = 630
    W = weights.initial(weights.SI, seed=1, n_classes=K)
    tfbundle.save_speaker_base(str(tmp_path), W, K)
    want = tfbundle.variable_shapes(os.path.join(HERE, 'golden', 'si_timit_variables.index'))
    got = tfbundle.variable_shapes(str(tmp_path / 'variables' / 'variables.index'))
    assert set(got) == set(want)
    assert all(tuple(got[k]) == tuple(want[k]) for k in want)
    assert {f'trainable_variables/{i}' for i in range(82, 88)} <= set(got)
    back, (kind, k, head) = tfbundle.load_bundle(str(tmp_path), with_layout=True)
    assert (kind, k, head) == (weights.SI, K, _lib.HEAD_SOFTMAX)
    assert set(back) == set(W)
    for name in W:
        assert back[name].dtype == np.float32 and (back[name].view(np.uint32) == W[name].view(np.uint32)).all()


def test_abi_and_keywords():
    import inspect
    names = ('mmla_si_base_drop_mask', 'mmla_si_base_loss_grad', 'mmla_si_base_train')
    assert all(n in _lib.SIGNATURES for n in names)
    header = open(os.path.join(HERE, '..', 'include', 'mmla.h')).read()
    assert f'#define MMLA_SI_BASE_MAX_CLASSES {_lib.SI_BASE_MAX_CLASSES}' in header
    assert _lib.SI_BASE_MAX_CLASSES == 1024 and _lib.SI_TRAIN_MAX_CLASSES == 32
    p = inspect.signature(si.train).parameters
    assert [p[k].default for k in ('epochs', 'batch_size', 'lr', 'patience', 'checkpoint_period')] == \
        [200, 32, 1e-4, 10, 10]
    assert inspect.signature(si.res_model).parameters['n_classes'].default == 630
    h = si.History(np.arange(12, dtype=np.float32).reshape(3, 4), 2, -1)
    assert list(h.history) == list(si.HISTORY_KEYS) and h.history['val_loss'] == [2.0, 6.0]
    assert h.best_epoch is None and h.epochs_run == 2
    if not os.path.exists(_lib.LIB_PATH):       # not built: the half above still stands
        return
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = _lib.SIGNATURES[name]
    assert lib.mmla_si_base_drop_mask(None, 0, 0, None, 0, None, None, 0) == -1
    assert lib.mmla_si_base_loss_grad(None, None, 0, 0, None, None, 0, 0, 0, None, None, None, None, 0) == -1
    assert lib.mmla_si_base_train(None, None, 0, 0, None, None, 0, None, None, 0, 0, 0, 0.0, None, 0, 0, 0,
                                  None, None, None, None, None, 0) == -1
