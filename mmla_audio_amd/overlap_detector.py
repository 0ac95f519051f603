"""Adapting OD-NET to new labelled feature images on the GPU: the part of the reference's
``OverlapDetection/scripts/overlap_detector.py`` that fits a trained detector further
(``OverlapDetector.continue_train_model``, :480-509) -- Adadelta under the cosine learning-rate schedule,
the class-weighted cross-entropy, early stopping -- through ``mmla_od_finetune`` (include/mmla.h, which
states what is computed; parity with TensorFlow itself is unpinned).

Not here: training from scratch (``train_model``, the initialisers), the pyramid-blur ``augment_images``,
the xlsx / PNG dataset loaders, the ``AUC`` metric, ``restore_best_weights`` and the three-class variant of
``evaluation``.
"""
import math

import numpy as np

from . import _lib, weights
from .speaker_identification import _stratified_split


def cal_weighted_penalty(y):
    """The script's class weights (:124-140) of one-hot labels y [n, K]: 1 - count_i / total."""
    y = np.asarray(y)
    quantity = (y == 1).sum(axis=0).astype(np.float64)
    return 1.0 - quantity / quantity.sum()


def cosine_lr(epochs, T_max=100, eta_max=1e-2, eta_min=1e-4):
    """CosineAnnealingScheduler's learning rate of every epoch (cosine_annealing.py:20) -> float64 [epochs]"""
    return np.array([eta_min + (eta_max - eta_min) * (1 + math.cos(math.pi * e / T_max)) / 2
                     for e in range(int(epochs))], np.float64)


def fit_plan(labels, seed, epochs, val_ratio=0.2):
    """Everything random about one fit, drawn with numpy from `seed`: the stratified train / validation
    split (the project's ``_stratified_split``; sklearn's ``train_test_split(random_state=0)`` draw is not
    reproduced: the same data gives a different, equally distributed split), and from generators of their
    own the sample order of every epoch and the dropout keep-masks (rate 0.25), indexed by training sample.
    -> dict(train, val index arrays; perm [epochs, n_train] i32; drop_mask [epochs, n_train, 512] u8)"""
    labels = np.asarray(labels)
    idx = np.arange(len(labels))
    train, val = idx, np.zeros(0, np.int64)
    if val_ratio > 0:
        train, val = _stratified_split(np.random.default_rng([int(seed), 0]), idx, labels, val_ratio)
    n = len(train)
    rng_p, rng_m = np.random.default_rng([int(seed), 1]), np.random.default_rng([int(seed), 2])
    perm = np.stack([rng_p.permutation(n) for _ in range(epochs)]).astype(np.int32) if epochs else \
        np.zeros((0, n), np.int32)
    mask = (rng_m.random((epochs, n, _lib.OD_DROP_UNITS)) >= 0.25).astype(np.uint8)
    return dict(train=train, val=val, perm=perm, drop_mask=mask)


def continue_train(W, images, labels, plan, epochs, batch_size, weighted=True, patience=10, device=None):
    """``continue_train_model`` on the device: W {name: array} (weights.od_spec), images uint8 [n,h,w,3],
    labels [n] in {0, 1}, plan = fit_plan(labels, seed, epochs).  weighted: the loss's class weights are
    cal_weighted_penalty of the training labels, else [1, 1].
    -> (W' {name: float32 array}, history [epochs_total, 5] = loss, acc, val_loss, val_acc, lr, epochs_run)"""
    ctx = device if isinstance(device, _lib.Context) else _lib.default_context(device)
    images = np.asarray(images, np.uint8)
    labels = np.asarray(labels, np.int32)
    tr, va = plan['train'], plan['val']
    cw = cal_weighted_penalty(np.eye(2)[labels[tr]]) if weighted else np.ones(2)
    out, hist, ran = ctx.od_finetune(weights.pack(weights.OD, W), images[tr], labels[tr],
                                     images[va] if len(va) else None, labels[va] if len(va) else None, cw,
                                     cosine_lr(epochs), plan['perm'], plan['drop_mask'], epochs, batch_size,
                                     patience)
    return weights.unpack(weights.OD, out), hist, ran
