"""TEST INFRASTRUCTURE: numpy restatement of the sigmoid-head trainer (``mmla_si_head_fit``,
include/mmla.h), i.e. of what Keras 2.6 computes for ``Dense(K, sigmoid)`` under
``categorical_crossentropy`` and ``RMSprop(1e-4)`` (speaker_identification.py:409-432), stated from
Keras' published source -- TensorFlow is not available, parity with TF itself is unpinned.

  forward   z = e W + b, s = 1 / (1 + exp(-z))
  loss      p = s / sum_k s_k; -log(clip(p_c, 1e-7, 1 - 1e-7)); mean over the batch
  gradient  dz_k = s_k (1 - s_k) (1 / S - [k = c] / s_c) / B, zero where p_c is outside the clip range
  RMSprop   rms <- 0.9 rms + 0.1 g^2; v <- v - lr g / (sqrt(rms) + 1e-7)

Every function takes ``dtype`` (float64: the reference; float32: the arithmetic the kernel is held
to, with numpy's summation order and correctly rounded exp / log / sqrt).
"""
import numpy as np


def forward(w, b, e, dtype):
    z = e.astype(dtype) @ w.astype(dtype) + b.astype(dtype)
    return dtype(1) / (dtype(1) + np.exp(-z))


def sample_stats(s, labels, dtype):
    """-> (per-sample loss, hit, inside-the-clip mask, S, s_c, gap between the top two sigmoids)"""
    lo, hi = dtype(1e-7), dtype(1) - dtype(1e-7)
    n = len(labels)
    S = s.sum(axis=1, dtype=dtype)
    sc = s[np.arange(n), labels]
    p = sc / S
    inside = (p >= lo) & (p <= hi)
    loss = -np.log(np.clip(p, lo, hi))
    hit = s.argmax(axis=1) == labels          # first index wins a tie
    if s.shape[1] > 1:
        top = np.sort(s, axis=1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(n, np.inf)
    return loss.astype(dtype), hit, inside, S, sc, gap


def loss_and_grad(w, b, e, labels, dtype=np.float64):
    """mean batch loss and its gradient (gW [512,K], gb [K]) by the formula above"""
    s = forward(w, b, e, dtype)
    loss, _, inside, S, sc, _ = sample_stats(s, labels, dtype)
    n, K = s.shape
    onehot = np.zeros((n, K), dtype)
    onehot[np.arange(n), labels] = 1
    dz = s * (dtype(1) - s) * (dtype(1) / S[:, None] - onehot / sc[:, None]) / dtype(n)
    dz = np.where(inside[:, None], dz, dtype(0)).astype(dtype)
    return loss.mean(dtype=dtype), e.astype(dtype).T @ dz, dz.sum(axis=0, dtype=dtype)


def fit(emb, labels, val_emb, val_labels, w0, b0, perm, epochs, batch=16, lr=1e-4, dtype=np.float64):
    """One restart: w0 [512,K], b0 [K], perm [epochs,n].  -> (w, b, history [epochs,4] in dtype with
    acc columns = hits / n in float64, the smallest top-two sigmoid gap over every sample evaluated)"""
    w = np.array(w0, dtype=dtype)
    b = np.array(b0, dtype=dtype)
    labels = np.asarray(labels)
    lr = dtype(np.float32(lr))               # the kernel's lr argument is a float
    rho, rest, eps = dtype(0.9), dtype(0.1), dtype(1e-7)
    rw, rb = np.zeros_like(w), np.zeros_like(b)
    n = len(labels)
    nv = 0 if val_labels is None else len(val_labels)
    hist = np.full((epochs, 4), np.nan, np.float64)
    min_gap = np.inf
    for ep in range(epochs):
        tot, hits = dtype(0), 0
        for i0 in range(0, n, batch):
            idx = perm[ep, i0:i0 + batch]
            e, y = emb[idx], labels[idx]
            s = forward(w, b, e, dtype)
            loss, hit, _, _, _, gap = sample_stats(s, y, dtype)
            min_gap = min(min_gap, float(gap.min()))
            tot += loss.mean(dtype=dtype) * dtype(len(idx))
            hits += int(hit.sum())
            _, gw, gb = loss_and_grad(w, b, e, y, dtype)
            rw = rho * rw + rest * gw * gw
            rb = rho * rb + rest * gb * gb
            w = w - lr * gw / (np.sqrt(rw) + eps)
            b = b - lr * gb / (np.sqrt(rb) + eps)
        hist[ep, 0] = tot / dtype(n)
        hist[ep, 1] = hits / n
        if nv:
            s = forward(w, b, val_emb, dtype)
            loss, hit, _, _, _, gap = sample_stats(s, np.asarray(val_labels), dtype)
            min_gap = min(min_gap, float(gap.min()))
            hist[ep, 2] = loss.mean(dtype=dtype)
            hist[ep, 3] = int(hit.sum()) / nv
    return w, b, hist, min_gap
