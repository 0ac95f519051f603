"""TEST INFRASTRUCTURE: the committed inputs of the stage-2 (fine-tune) tests, the helper's float64 and
float32 runs on them (computed once per process, shared, never modified) and the two comparison rules.

The rules (tests/test_gpu_si_finetune.py holds the kernels to them, tests/test_si_finetune_ref_cpu.py
checks that the inputs satisfy their conditions):
  d32 rule   per tensor (or scalar), d32 = max|helper float32 - helper float64|; the kernel must lie
             within FACTOR * d32 of the float64 run, with a floor of FACTOR * 2^-24 * max|ref64| for a
             tensor whose d32 happens to be tiny.  FACTOR = 16 as in test_gpu_si_registration.py: other
             summation orders and hardware exp / log.
  update     weights after a fit are compared as updates D = out - in, because RMSprop's first step is
             +-3.16 lr whatever |g| is: per tensor the share of entries with |D - D64| > 2 % of
             steps * 3.17 * lr is at most 1e-3, and none in a tensor of fewer than 1000 entries.
"""
import functools

import numpy as np
import torch

import si_finetune_ref as ref
from mmla_audio_amd import weights

FACTOR = 16.0
K = 3
MARGIN = 1e-5
GRAD_SEED = 3          # chosen on the CPU: margins >= MARGIN at B = 2 and B = 1 (about one seed in ten)
FIT_SEED = 4          # the helper's float32 fit stays inside the update cap (asserted on the CPU)
FIT = dict(n_train=5, n_val=3, batch=2, epochs=2, lr=1e-6)
SHARE, STEP_FRACTION, SMALL = 1e-3, 0.02, 1000


def _windows(seed, n):
    rng = np.random.default_rng([seed, 77])
    x = (rng.standard_normal((n, 256, 39)) * 10).astype(np.float32)
    return x, rng.integers(0, K, n).astype(np.int32)


def synthetic(seed):
    return weights.synthetic(weights.SI, seed=seed, n_classes=K)


def grad_case(B):
    """-> (W, x [B,256,39] f32, labels [B])"""
    x, labels = _windows(GRAD_SEED, 2)
    return synthetic(GRAD_SEED), x[:B], labels[:B]


def fit_case():
    """-> dict(W, x, labels, val_x, val_labels, perm [epochs, n_train])"""
    n, nv = FIT['n_train'], FIT['n_val']
    x, labels = _windows(FIT_SEED + 1000, n + nv)
    rng = np.random.default_rng([FIT_SEED, 78])
    perm = np.stack([rng.permutation(n) for _ in range(FIT['epochs'])]).astype(np.int32)
    return dict(W=synthetic(FIT_SEED), x=x[:n], labels=labels[:n], val_x=x[n:], val_labels=labels[n:],
                perm=perm)


def fit_steps():
    return FIT['epochs'] * -(-FIT['n_train'] // FIT['batch'])


@functools.lru_cache(maxsize=None)
def grad_ref(B):
    """-> {dtype name: (data, R, {name: grad})} of the helper, and the float64 margins"""
    W, x, labels = grad_case(B)
    out = {'f64': ref.loss_and_grad(W, K, x, labels, torch.float64),
           'f32': ref.loss_and_grad(W, K, x, labels, torch.float32)}
    m = ref.margins(W, K, x, labels)
    assert m[0] >= MARGIN and m[1] >= MARGIN, f'GRAD_SEED no longer has its margins: {m}'
    return out


@functools.lru_cache(maxsize=None)
def fit_ref():
    """-> {dtype name: (W_out, history, margins)} of the helper on fit_case()"""
    c = fit_case()
    args = (c['W'], K, c['x'], c['labels'], c['val_x'], c['val_labels'], c['perm'], FIT['epochs'],
            FIT['batch'], FIT['lr'])
    return {'f64': ref.fit(*args, dtype=torch.float64), 'f32': ref.fit(*args, dtype=torch.float32)}


def d32_bound(r64, r32):
    r64, r32 = np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    d32 = float(np.max(np.abs(r32 - r64))) if r64.size else 0.0
    return FACTOR * max(d32, 2.0 ** -24 * float(np.max(np.abs(r64))) if r64.size else 0.0)


def check_d32(name, got, r64, r32):
    """assert the d32 rule for one tensor; prints the figures first"""
    bound = d32_bound(r64, r32)
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(r64, np.float64))))
    print(f'{name}: |got - ref64| {err:.3e}  bound {bound:.3e}  (max|ref64| {np.max(np.abs(r64)):.3e})')
    assert err <= bound, f'{name}: {err:.3e} > {bound:.3e}'


def update_share(w_in, w_out, w_out64, steps, lr):
    """share of entries whose update is off the float64 update by more than 2 % of the largest
    possible one"""
    d = np.asarray(w_out, np.float64) - np.asarray(w_in, np.float64)
    d64 = np.asarray(w_out64, np.float64) - np.asarray(w_in, np.float64)
    return float(np.mean(np.abs(d - d64) > STEP_FRACTION * steps * 3.17 * lr))


def check_updates(W_in, W_out, W_out64, label):
    """the update rule over every trainable tensor; -> the worst share"""
    worst = 0.0
    for name, shape, role in weights.si_spec(K):
        if ref.is_frozen(role):
            continue
        share = update_share(W_in[name], W_out[name], W_out64[name], fit_steps(), FIT['lr'])
        worst = max(worst, share)
        cap = 0.0 if int(np.prod(shape)) < SMALL else SHARE
        assert share <= cap, f'{label} {name}: share {share:.2e} of updates off by > 2 % (cap {cap})'
    print(f'{label}: worst share of off updates {worst:.2e}')
    return worst


def unpack(blob, n_classes=K):
    return weights.unpack(weights.SI, blob, n_classes)
