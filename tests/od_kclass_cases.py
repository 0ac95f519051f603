"""TEST INFRASTRUCTURE: the inputs of the K-class OD tests (tests/test_gpu_od_kclass.py), a numpy restatement of
the K-class AUC, and the restatement's float64 / float32 runs on the gradient and fit cases (computed once per
process, shared, never modified).  tests/test_od_kclass_cpu.py checks the conditions the GPU bounds rest on.

The head of a K-class test model: every tensor below it is ``weights.synthetic(OD, seed)``'s; the Dense kernel
is uniform in +-max|the two-class head kernel of the same synthetic W|, the bias normal(0, 0.1), both drawn from
``default_rng([77, K])``.  The bounds are those of tests/od_finetune_cases.py (the d32 rule, the update rule)
and of tests/test_gpu_od_train.py (AUC_TOL); none is new.
"""
import functools

import numpy as np
import torch

import od_finetune_cases as C
import od_finetune_ref as ref
import od_train_ref as tr
from mmla_audio_amd import overlap_detector, weights

KS = (3, 8)
HEAD = ref.HEAD
AUC_TOL = 1.2e-7            # tests/test_gpu_od_train.py
GRAD_SHAPES = ((20, 23, 3), (9, 8, 1))
FIT = C.FIT
FIT_K = 3
DROP_SEED = 0x5EED0D0D17
LABEL_STREAM = 94           # of the fit's labels and orders, chosen on the CPU (auc_margins; 93 puts a
                            # validation prob of epoch 2 within 5e-6 of a threshold)
CLIP_LO = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))


def with_head(W2, K):
    """the two-class weights W2 with the K-class test head"""
    rng = np.random.default_rng([77, K])
    lim = float(np.abs(W2[HEAD + '/kernel']).max())
    W = dict(W2)
    W[HEAD + '/kernel'] = rng.uniform(-lim, lim, (512, K)).astype(np.float32)
    W[HEAD + '/bias'] = rng.normal(0, 0.1, K).astype(np.float32)
    return W


def synthetic(seed, K):
    return with_head(weights.synthetic(weights.OD, seed=seed), K)


def pack(W):
    return weights.pack(weights.OD, W, weights.od_classes(W))


def unpack(blob, K):
    return weights.unpack(weights.OD, blob, K)


def spec(K):
    return weights.od_spec(K)


def class_w(K):
    return np.linspace(0.3, 0.9, K).astype(np.float32)


def labels_for(B, K):
    """arange(B) % K with the last one K - 1"""
    l = (np.arange(B) % K).astype(np.int32)
    l[-1] = K - 1
    return l


def forward_inputs():
    return np.random.default_rng(3).integers(0, 256, (5, 128, 151, 3)).astype(np.uint8)


# ---- AUC ------------------------------------------------------------------------------------------------

def auc(probs, labels):
    """Keras AUC() with multi_label=False on probs [n, K] against labels [n]: per threshold TP counts the
    true-class entry where p > thr, FP the K - 1 other entries where p > thr; recall = TP / n, fpr = FP /
    (n (K - 1)); the trapezoid sum over the 200 thresholds in double from the integer counts -> float32"""
    probs = np.asarray(probs, np.float32)
    n, K = probs.shape
    labels = np.asarray(labels).astype(np.int64)
    thr = tr.thresholds()
    true_p = probs[np.arange(n), labels]
    tp = np.array([int((true_p > t).sum()) for t in thr], np.int64)
    fp = np.array([int((probs > t).sum()) for t in thr], np.int64) - tp
    rec = tp.astype(np.float64) / float(n)
    fpr = fp.astype(np.float64) / float(n * (K - 1))
    total = 0.0
    for t in range(len(thr) - 1):
        total += (fpr[t] - fpr[t + 1]) * (rec[t] + rec[t + 1]) / 2.0
    return np.float32(total)


def auc_inputs(n, K):
    """informative predictions: the softmax of noise with the label's logit raised"""
    rng = np.random.default_rng([32, n, K])
    labels = rng.integers(0, K, n).astype(np.int32)
    z = rng.normal(0, 1, (n, K))
    z[np.arange(n), labels] += 1.0
    p = np.exp(z - z.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32), labels


# ---- gradient cases -------------------------------------------------------------------------------------

def grad_case(h, w, B, K):
    """-> (W, img [B,h,w,3] u8, labels [B], mask [B,512] u8): od_finetune_cases' inputs with the K-class head"""
    W2, img, _, mask = C.grad_case(h, w, B)
    return with_head(W2, K), img, labels_for(B, K), mask


@functools.lru_cache(maxsize=None)
def grad_ref(h, w, B, K):
    """-> {dtype name: (loss, {name: grad}, {name: value after the moving update}, margins)}"""
    W, img, labels, mask = grad_case(h, w, B, K)
    return {'f64': ref.loss_and_grad(W, img, labels, class_w(K), mask, torch.float64),
            'f32': ref.loss_and_grad(W, img, labels, class_w(K), mask, torch.float32)}


def q_true(W, img, labels, mask):
    """the float64 q_c of every sample of a training-mode batch"""
    with torch.no_grad():
        z = ref._Net(W, torch.float64).logits(img, mask, True)
        p = torch.softmax(z, 1)
        p = (p / p.sum(dim=1, keepdim=True)).numpy()
    return p[np.arange(len(labels)), np.asarray(labels)]


def clip_case():
    """grad_case(20, 23, 3) at K = 3 with bias (40, 0, 0) and every label 1: q_1 ~ e^-40, below the clip"""
    W, img, _, mask = grad_case(20, 23, 3, 3)
    W = dict(W)
    W[HEAD + '/bias'] = np.array([40.0, 0.0, 0.0], np.float32)
    return W, img, np.full(3, 1, np.int32), mask


# ---- the fit --------------------------------------------------------------------------------------------

def fit_case():
    """od_finetune_cases.FIT's sizes with labels in {0, 1, 2}, all present in train and validation; the
    keep-masks are those of mmla_od_train's DROP_SEED (tests/od_train_ref.drop_mask)"""
    n, nv, ep, K = FIT['n_train'], FIT['n_val'], FIT['epochs'], FIT_K
    img, _, _ = C.images(FIT['seed'] + 1000, n + nv, FIT['h'], FIT['w'])
    rng = np.random.default_rng([FIT['seed'], LABEL_STREAM])
    labels = rng.integers(0, K, n + nv).astype(np.int32)
    labels[:K] = np.arange(K)
    labels[n:n + K] = np.arange(K)
    perm = np.stack([rng.permutation(n) for _ in range(ep)]).astype(np.int32)
    masks = np.stack([tr.drop_mask(DROP_SEED, e, np.arange(n)) for e in range(ep)])
    return dict(W=synthetic(FIT['seed'], K), img=img[:n], labels=labels[:n], val_img=img[n:],
                val_labels=labels[n:], perm=perm, masks=masks,
                lr=overlap_detector.cosine_lr(ep).astype(np.float32), class_w=class_w(K))


@functools.lru_cache(maxsize=None)
def fit_ref():
    """-> {dtype name: (W_out, history, epochs_run, margins)} of the restatement on fit_case()"""
    c = fit_case()
    args = (c['W'], c['img'], c['labels'], c['val_img'], c['val_labels'], c['class_w'], c['lr'], c['perm'],
            c['masks'], FIT['epochs'], FIT['batch'], 0)
    return {'f64': ref.fit(*args, dtype=torch.float64), 'f32': ref.fit(*args, dtype=torch.float32)}


def threshold_margin(probs):
    """the smallest distance of a prob to an inner AUC threshold"""
    p = np.asarray(probs, np.float64).ravel()
    inner = tr.thresholds().astype(np.float64)[1:-1]
    return float(np.abs(p[:, None] - inner[None]).min())


def decided(probs, margin=1e-5):
    """no prob within `margin` of an inner AUC threshold"""
    p = np.asarray(probs, np.float64).ravel()
    return bool(((p >= 0) & (p <= 1)).all()) and threshold_margin(p) > margin


def train_probs(c):
    """the float64 training-mode softmax outputs of the fit's first epoch run as one batch"""
    order = c['perm'][0]
    with torch.no_grad():
        z = ref._Net(c['W'], torch.float64).logits(c['img'][order], c['masks'][0][order], True)
        return torch.softmax(z, 1).numpy()


def auc_margins():
    """-> (per epoch the threshold margin of the restatement's float64 validation probs after that many
    epochs, the margin of train_probs)"""
    c = fit_case()
    val = []
    for e in range(1, FIT['epochs'] + 1):
        W = ref.fit(c['W'], c['img'], c['labels'], c['val_img'], c['val_labels'], c['class_w'], c['lr'], c['perm'],
                    c['masks'], e, FIT['batch'], 0, dtype=torch.float64)[0]
        val.append(threshold_margin(ref.forward(W, c['val_img'])))
    return val, threshold_margin(train_probs(c))
