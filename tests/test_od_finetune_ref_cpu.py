"""CPU: the restatement tests/od_finetune_ref.py is sound -- its inference-mode forward is Nets.od_forward,
its gradient agrees with central differences -- and the inputs of tests/test_gpu_od_finetune.py satisfy the
conditions their bounds rest on (tests/od_finetune_cases.py)."""
import numpy as np
import pytest
import torch

import od_finetune_cases as C
import od_finetune_ref as ref
from mmla_audio_amd import _lib, overlap_detector
from oracle.nets_torch import Nets


def test_inference_forward_is_od_forward():
    for (h, w, B) in ((20, 23, 3), (9, 8, 1)):
        W, img, _, _ = C.grad_case(h, w, B)
        got = ref.forward(W, img)
        want = Nets(W).od_forward(img.astype(np.float64))
        assert np.abs(got - want).max() <= 1e-10


# one tensor of every role: stem and block kernels, a bias in front of a pool (the only ones with a
# gradient: a bias in front of a BatchNorm on batch statistics has none), gamma, beta, the LSTM, the head
FD_TENSORS = ('layer_with_weights-0/kernel', 'layer_with_weights-2/kernel', 'layer_with_weights-4/bias',
              'layer_with_weights-5/kernel', 'layer_with_weights-3/gamma', 'layer_with_weights-3/beta',
              'layer_with_weights-17/kernel', 'layer_with_weights-40/forward/kernel',
              'layer_with_weights-40/forward/recurrent_kernel', 'layer_with_weights-40/backward/bias',
              'layer_with_weights-41/kernel', 'layer_with_weights-41/bias')


def test_gradient_matches_central_differences():
    h, w, B = 20, 23, 3
    W, img, labels, mask = C.grad_case(h, w, B)
    _, g, _, _ = C.grad_ref(h, w, B)['f64']
    rng = np.random.default_rng(11)
    for name in FD_TENSORS:
        base = W[name].astype(np.float64)
        scale = float(np.abs(g[name]).max())
        assert scale > 0, name
        for _ in range(2):
            at = tuple(int(rng.integers(0, s)) for s in base.shape)
            # small enough that no pool window or LeakyReLU of the case (margins >= 1e-5) changes sides
            step = 1e-6 * max(float(np.abs(base).max()), 1e-3)
            vals = []
            for sign in (1.0, -1.0):
                Wp = dict(W)
                t = base.copy()
                t[at] += sign * step
                Wp[name] = t
                vals.append(ref.loss_only(Wp, img, labels, C.CLASS_W, mask))
            fd = (vals[0] - vals[1]) / (2 * step)
            assert abs(fd - g[name][at]) <= 1e-4 * scale + 1e-7, (name, at, fd, g[name][at])


def test_moving_statistics_are_frozen_for_the_gradient_and_advance_one_step():
    W, img, labels, mask = C.grad_case(9, 8, 1)
    _, g, mv, _ = C.grad_ref(9, 8, 1)['f64']
    for name, _, role in C.SPEC:
        if ref.is_frozen(role):
            assert not g[name].any() and (mv[name] != W[name]).any()
        else:
            assert np.array_equal(mv[name], W[name].astype(np.float64))


@pytest.mark.parametrize('h,w,B', list(C.GRAD_CASES))
def test_gradient_cases_have_their_margins(h, w, B):
    m = C.grad_ref(h, w, B)['f64'][3]
    print(h, w, B, m)
    assert m['pool'] >= C.GRAD_MARGIN[(h, w, B)] and m['leaky'] >= C.MARGIN, m


def test_float32_restatement_is_inside_the_update_rule():
    c = C.fit_case()
    r = C.fit_ref()
    assert r['f64'][2] == r['f32'][2] == C.FIT['epochs']
    C.check_updates(c['W'], r['f32'][0], r['f64'][0], C.fit_lr_sum(c, C.FIT), 'float32 restatement')


def test_early_stop_is_decided_by_a_wide_gap():
    r = C.stop_ref()
    (_, h64, ran64, _), (_, h32, ran32, _) = r['f64'], r['f32']
    assert ran64 == ran32 and 1 < ran64 < C.STOP['epochs']
    assert np.isnan(h64[ran64:]).all()
    d32 = np.abs(h32[:ran64, 2] - h64[:ran64, 2]).max()
    gaps = np.abs(np.diff(h64[:ran64, 2]))
    print('val_loss', h64[:ran64, 2], 'd32', d32)
    assert gaps.min() > 100 * d32
    assert h64[ran64 - 1, 2] >= h64[:ran64 - 1, 2].min()      # the last epoch did not improve


def test_save_overlap_round_trip(tmp_path):
    from mmla_audio_amd import tfbundle, weights
    W = C.synthetic(2)
    tfbundle.save_overlap(str(tmp_path), W)
    got, (kind, k, head) = tfbundle.load_bundle(str(tmp_path), with_layout=True)
    assert (kind, k, head) == (weights.OD, 2, _lib.HEAD_SOFTMAX) and set(got) == set(W)
    for name in W:
        assert got[name].dtype == np.float32 and got[name].tobytes() == W[name].tobytes(), name
    bad = dict(W)
    del bad['layer_with_weights-41/bias']
    with pytest.raises(ValueError):
        tfbundle.save_overlap(str(tmp_path / 'x'), bad)


def test_python_helpers():
    import math
    assert overlap_detector.cosine_lr(2).tolist() == [1e-2, 1e-4 + (1e-2 - 1e-4) * (1 + math.cos(math.pi / 100)) / 2]
    assert overlap_detector.cal_weighted_penalty(np.eye(2)[[0, 1, 1, 1]]).tolist() == [0.75, 0.25]
    labels = np.array([0, 1] * 10)
    p, q = overlap_detector.fit_plan(labels, 4, 3), overlap_detector.fit_plan(labels, 4, 3)
    assert len(p['val']) == 4 and len(p['train']) == 16 and not set(p['train']) & set(p['val'])
    assert sorted(labels[p['val']]) == [0, 0, 1, 1]
    assert all(np.array_equal(p[k], q[k]) for k in p)
    assert all(sorted(row) == list(range(16)) for row in p['perm'])
    assert p['drop_mask'].shape == (3, 16, _lib.OD_DROP_UNITS) and p['drop_mask'].dtype == np.uint8
    # the first epochs of a longer plan are the shorter plan's
    assert np.array_equal(overlap_detector.fit_plan(labels, 4, 5)['perm'][:3], p['perm'])
    assert 'mmla_od_loss_grad' in _lib.SIGNATURES and 'mmla_od_finetune' in _lib.SIGNATURES
