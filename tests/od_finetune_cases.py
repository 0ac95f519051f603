"""TEST INFRASTRUCTURE: the inputs of the OD adaptation tests, the restatement's float64 and float32 runs on
them (computed once per process, shared, never modified) and the two comparison rules.

The rules (tests/test_gpu_od_finetune.py holds the kernels to them, tests/test_od_finetune_ref_cpu.py checks
that the inputs satisfy their conditions):
  d32 rule   per tensor (or scalar), d32 = max|restatement float32 - restatement float64|; the kernel must
             lie within FACTOR * d32 of the float64 run, with a floor of FACTOR * 2^-24 * max|ref64|.
             FACTOR = 16, the project's rule: other summation orders, hardware exp / log.
  update     weights after a fit are compared as updates D = out - in.  Adadelta's step is
             u = sqrt(d + eps) / sqrt(a + eps) g: the first is lr sqrt(eps / (1 - rho)) sign(g) = 1.414e-3 lr
             whatever |g| is (for g^2 >> eps / (1 - rho)), and with a steady gradient the later ones stay at
             that size.  Per tensor the share of entries with |D - D64| > 2 % of STEP * sum of the steps' lr
             is at most 1e-3, and none in a tensor of fewer than 1000 entries.
"""
import functools

import numpy as np
import torch

import od_finetune_ref as ref
from mmla_audio_amd import overlap_detector, weights

FACTOR = 16.0
MARGIN = 1e-5
CLASS_W = (0.3, 0.7)
# (h, w, B) -> seed, chosen on the CPU: pool and LeakyReLU margins >= the case's margin in the float64 run.
# At the room's size a batch of 2 has 1.7 million pool windows of O(1) values: the smallest gap of random
# inputs is ~1e-6 whatever the seed (five seeds gave 5e-7 .. 4.6e-6), so MARGIN is out of reach there and
# the case asserts what its seed has.  A window closer than float32 resolves moves one pixel's gradient to
# its neighbour in the float32 restatement as well: it is part of d32.
GRAD_CASES = {(20, 23, 3): 1, (9, 8, 1): 1, (128, 151, 2): 5}
GRAD_MARGIN = {(20, 23, 3): MARGIN, (9, 8, 1): MARGIN, (128, 151, 2): 4e-6}
FIT = dict(h=20, w=23, n_train=10, n_val=4, batch=4, epochs=3, seed=5)
# a constant lr of 2 makes the validation loss turn within three epochs (chosen on the CPU)
STOP = dict(h=20, w=23, n_train=6, n_val=4, batch=3, epochs=5, patience=1, seed=6, lr=2.0)
STEP = float(np.sqrt(1e-7 / 0.05))
SHARE, STEP_FRACTION, SMALL = 1e-3, 0.02, 1000
SPEC = ref.SPEC


def synthetic(seed):
    return weights.synthetic(weights.OD, seed=seed)


def images(seed, n, h, w):
    """random-noise images (flat ones make pool ties), labels, dropout keep-masks with a quarter dropped"""
    rng = np.random.default_rng([seed, 91])
    img = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    labels = rng.integers(0, 2, n).astype(np.int32)
    mask = (rng.random((n, 512)) >= 0.25).astype(np.uint8)
    return img, labels, mask


def grad_case(h, w, B):
    """-> (W, img [B,h,w,3] u8, labels [B], mask [B,512] u8)"""
    seed = GRAD_CASES[(h, w, B)]
    return (synthetic(seed),) + images(seed + 100 * h + w, B, h, w)


@functools.lru_cache(maxsize=None)
def grad_ref(h, w, B):
    """-> {dtype name: (loss, {name: grad}, {name: value after the moving update}, margins)}"""
    W, img, labels, mask = grad_case(h, w, B)
    return {'f64': ref.loss_and_grad(W, img, labels, CLASS_W, mask, torch.float64),
            'f32': ref.loss_and_grad(W, img, labels, CLASS_W, mask, torch.float32)}


def _fit_case(cfg, lr):
    n, nv, ep = cfg['n_train'], cfg['n_val'], cfg['epochs']
    img, labels, _ = images(cfg['seed'] + 1000, n + nv, cfg['h'], cfg['w'])
    labels[:2] = (0, 1)                                  # both classes in the training set
    rng = np.random.default_rng([cfg['seed'], 92])
    perm = np.stack([rng.permutation(n) for _ in range(ep)]).astype(np.int32)
    masks = (rng.random((ep, n, 512)) >= 0.25).astype(np.uint8)
    return dict(W=synthetic(cfg['seed']), img=img[:n], labels=labels[:n], val_img=img[n:], val_labels=labels[n:],
                perm=perm, masks=masks, lr=np.asarray(lr, np.float32))


def fit_case():
    return _fit_case(FIT, overlap_detector.cosine_lr(FIT['epochs']))


def stop_case():
    return _fit_case(STOP, np.full(STOP['epochs'], STOP['lr']))


def _fit_ref(c, cfg, patience):
    args = (c['W'], c['img'], c['labels'], c['val_img'], c['val_labels'], CLASS_W, c['lr'], c['perm'], c['masks'],
            cfg['epochs'], cfg['batch'], patience)
    return {'f64': ref.fit(*args, dtype=torch.float64), 'f32': ref.fit(*args, dtype=torch.float32)}


@functools.lru_cache(maxsize=None)
def fit_ref():
    """-> {dtype name: (W_out, history, epochs_run, margins)} of the restatement on fit_case()"""
    return _fit_ref(fit_case(), FIT, 0)


@functools.lru_cache(maxsize=None)
def stop_ref():
    return _fit_ref(stop_case(), STOP, STOP['patience'])


def fit_lr_sum(c, cfg):
    return float(np.sum(c['lr'].astype(np.float64)) * -(-cfg['n_train'] // cfg['batch']))


def d32_bound(r64, r32):
    r64, r32 = np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    d32 = float(np.max(np.abs(r32 - r64))) if r64.size else 0.0
    return FACTOR * max(d32, 2.0 ** -24 * float(np.max(np.abs(r64))) if r64.size else 0.0)


def check_d32(name, got, r64, r32, worst=None):
    """assert the d32 rule for one tensor; prints the figures first"""
    bound = d32_bound(r64, r32)
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(r64, np.float64))))
    ratio = FACTOR * err / bound if bound > 0 else 0.0
    print(f'{name}: |got - ref64| {err:.3e}  bound {bound:.3e}  ratio {ratio:.2f} of {FACTOR:.0f}  '
          f'(max|ref64| {np.max(np.abs(r64)):.3e})')
    if worst is not None:
        worst[name] = ratio
    assert err <= bound, f'{name}: {err:.3e} > {bound:.3e}'


def check_updates(W_in, W_out, W_out64, lr_sum, label):
    """the update rule over every trainable tensor; -> the worst share"""
    worst = 0.0
    for name, shape, role in SPEC:
        if ref.is_frozen(role):
            continue
        d = np.asarray(W_out[name], np.float64) - np.asarray(W_in[name], np.float64)
        d64 = np.asarray(W_out64[name], np.float64) - np.asarray(W_in[name], np.float64)
        share = float(np.mean(np.abs(d - d64) > STEP_FRACTION * STEP * lr_sum))
        worst = max(worst, share)
        cap = 0.0 if int(np.prod(shape)) < SMALL else SHARE
        assert share <= cap, f'{label} {name}: share {share:.2e} of updates off by > 2 % (cap {cap})'
    print(f'{label}: worst share of off updates {worst:.2e}')
    return worst


def unpack(blob):
    return weights.unpack(weights.OD, blob)


def pack(W):
    return weights.pack(weights.OD, W)
