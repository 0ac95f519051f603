"""Training OD-NET on labelled feature images on the GPU: the fits of the reference's
``OverlapDetection/scripts/overlap_detector.py``.  ``OverlapDetector.continue_train_model`` (:480-509) fits a
trained detector further -- Adadelta under the cosine learning-rate schedule, the class-weighted
cross-entropy, early stopping -- through ``mmla_od_finetune``; ``train_model`` (:392-451) trains one from the
Keras initial state through ``mmla_od_train``, which adds keep-bits generated on the device, ModelCheckpoint
and the AUC metric, after the pyramid-blur class balancing of ``augment_images`` (:143-220,
``mmla_od_augment``).  include/mmla.h states what is computed; parity with TensorFlow and OpenCV themselves
is unpinned.

The detector has K classes, 2 <= K <= ``weights.OD_MAX_CLASSES``: two for the deployed model, three (``Overlap``
column values 0, 1, 2; class 2 = overlapped) for the reference's research models.  ``train_model`` takes K from
the labels, ``continue_train`` from the weights, and ``evaluation`` (:513-543) scores the last class.

Not here: the xlsx / PNG dataset loaders, ``StratifiedKFold``, ``restore_best_weights`` (the reference never
sets it) and multi-GPU training.
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
    """``continue_train_model`` on the device: W {name: array} (weights.od_spec(K), K from its head), images
    uint8 [n,h,w,C] with C the channels of W's stem (3, or 1 for an imagetype='gray' model), labels [n] in
    [0, K), plan = fit_plan(labels, seed, epochs).  weighted: the loss's class weights are
    cal_weighted_penalty of the training labels, else ones.
    -> (W' {name: float32 array}, history [epochs_total, 5] = loss, acc, val_loss, val_acc, lr, epochs_run)"""
    ctx = device if isinstance(device, _lib.Context) else _lib.default_context(device)
    images = np.asarray(images, np.uint8)
    labels = np.asarray(labels, np.int32)
    tr, va = plan['train'], plan['val']
    K, ch = weights.od_classes(W), weights.od_channels(W)
    cw = cal_weighted_penalty(np.eye(K)[labels[tr]]) if weighted else np.ones(K)
    out, hist, ran = ctx.od_finetune(weights.pack(weights.OD, W, K, ch), images[tr], labels[tr],
                                     images[va] if len(va) else None, labels[va] if len(va) else None, cw,
                                     cosine_lr(epochs), plan['perm'], plan['drop_mask'], epochs, batch_size,
                                     patience)
    return weights.unpack(weights.OD, out, K, ch), hist, ran


# ---- training from scratch: augment_images (:143-220), train_model (:392-451) -----------------------------

HISTORY_KEYS = ('loss', 'categorical_accuracy', 'val_loss', 'val_categorical_accuracy', 'lr', 'auc', 'val_auc')


class History:
    """What ``model.fit`` returns, as far as the reference reads it: ``history`` is a dict of the Keras keys
    (``HISTORY_KEYS``), one value per epoch run.  ``epochs_run`` and ``best_epoch`` (0-based, None if no
    checkpoint was taken) say what the two callbacks did."""

    def __init__(self, rows, epochs_run, best_epoch):
        rows = np.asarray(rows, np.float32)[:epochs_run]
        self.history = {k: [float(v) for v in rows[:, i]] for i, k in enumerate(HISTORY_KEYS)}
        self.epoch = list(range(epochs_run))
        self.epochs_run = int(epochs_run)
        self.best_epoch = None if best_epoch < 0 else int(best_epoch)


def _class_labels(y, what):
    """labels [n] of integers, or one-hot rows [n, K] as ``labels_loader`` returns them -> int32 [n]"""
    y = np.asarray(y)
    if y.ndim == 2:
        if not 2 <= y.shape[1] <= weights.OD_MAX_CLASSES or \
                not (((y == 0) | (y == 1)).all() and (y.sum(axis=1) == 1).all()):
            raise ValueError(f'{what} {y.shape}: expected one-hot rows of 2..{weights.OD_MAX_CLASSES} classes')
        return y.argmax(axis=1).astype(np.int32)
    if y.ndim != 1 or not np.issubdtype(y.dtype, np.integer):
        raise ValueError(f'{what} {y.shape} {y.dtype}: expected integer labels [n] or one-hot rows [n,K]')
    return y.astype(np.int32)


def _n_classes(n_classes, *ys):
    """K of a fit: the given one, else the one-hot width of the first two-dimensional y, else max label + 1;
    never below 2"""
    if n_classes is not None:
        return int(n_classes)
    for y in ys:
        if y is not None and np.ndim(y) == 2:
            return max(2, int(np.shape(y)[1]))
    top = max([int(np.max(y)) for y in ys if y is not None and np.size(y)], default=1)
    return max(2, top + 1)


def augment_plan(labels, n_classes=None):
    """The class balancing of ``augment_images`` (:158-166, :199-204) as indices: count[k] images per class,
    base = max(count), ratio[k] = base / count[k] - 1, and for i in range(round(ratio[k])) -- Python's round,
    half to even -- every image of class k gets a copy blurred i + 1 times.  -> (src, levels, new_labels),
    int32 each: the originals in input order at level 0, then the copies by class, by i, by image.  n_classes
    None: max(labels) + 1."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer) or (labels.size and labels.min() < 0):
        raise ValueError(f'labels {labels.shape} {labels.dtype}: expected non-negative integers [n]')
    K = int(labels.max()) + 1 if n_classes is None and labels.size else int(n_classes or 0)
    if labels.size and labels.max() >= K:
        raise ValueError(f'label {int(labels.max())} outside the {K} classes')
    count = [int((labels == k).sum()) for k in range(K)]
    for k in range(K):
        if count[k] == 0:
            raise ValueError(f'class {k} has no images: its ratio base / count is undefined')
    base = max(count) if K else 0
    src, levels = [np.arange(len(labels))], [np.zeros(len(labels), np.int64)]
    for k in range(K):
        copies = round(base / count[k] - 1)
        if copies > _lib.OD_AUG_MAX_LEVELS:
            raise ValueError(f'class {k}: {copies} copies per image, more than the {_lib.OD_AUG_MAX_LEVELS} '
                             f'levels built')
        members = np.flatnonzero(labels == k)
        for i in range(copies):
            src.append(members)
            levels.append(np.full(len(members), i + 1))
    src = np.concatenate(src).astype(np.int32)
    return src, np.concatenate(levels).astype(np.int32), labels[src].astype(np.int32)


def _augment(ctx, images, src, levels):
    """``mmla_od_augment`` on [n,h,w,3], or on one-channel images [n,h,w,1]: widened to three equal channels
    (what ``cv.imread`` gives the reference for a gray PNG), blurred on the same kernel, channel 0 returned --
    the blur is per channel, so this is exact"""
    if images.shape[3] == 1:
        return np.ascontiguousarray(ctx.od_augment(np.repeat(images, 3, axis=3), src, levels)[..., :1])
    return ctx.od_augment(images, src, levels)


def augment_images(images, labels, ctx=None):
    """``augment_images`` on arrays: images uint8 [n,h,w,C] (C = 3 or 1), labels [n] -> (images_aug [m,h,w,C],
    labels_aug [m]) in ``augment_plan``'s order, the blurred copies through ``mmla_od_augment``."""
    ctx = ctx if isinstance(ctx, _lib.Context) else _lib.default_context(ctx)
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] not in weights.OD_CHANNELS or \
            images.shape[0] != len(labels):
        raise ValueError(f'images {images.shape} {images.dtype}: expected uint8 [n,h,w,3] or [n,h,w,1], one per label')
    src, levels, new_labels = augment_plan(labels)
    return _augment(ctx, images, src, levels), new_labels


def train_model(x_train, y_train, x_val, y_val, *, epochs, batch_size, weighted=False, augmented=False, seed=0,
                patience=10, checkpoint_path=None, save_path=None, device=None, n_classes=None):
    """``OverlapDetector.train_model`` on the device (``mmla_od_train``): ``__ResBLSTM`` from its Keras initial
    state (``weights.initial_od(seed)``) under Adadelta with the cosine schedule, EarlyStopping(val_loss,
    patience) and ModelCheckpoint(val_categorical_accuracy, save_best_only, 'max', period=1).  Images uint8
    [n,h,w,3], or [n,h,w,1] for the one-channel network of ``OverlapDetector(imagetype='gray')`` (:84-90: the
    stem is Conv2D(16, 1) on one channel; the model returned then has ``channels == 1``); labels integers or
    one-hot rows.  augmented: the training set is balanced first
    (``augment_images``); weighted: the loss's class weights are ``cal_weighted_penalty`` of the (possibly
    augmented) training labels, else ones.  n_classes (the script's ``class_dim = y_train.shape[1]``, :394):
    None = the width of one-hot labels, or the largest label + 1, never below 2.  x_val None or empty: no
    validation set, no callbacks.
    -> (OverlapDetectionModel, History): the model holds the LAST epoch's weights (no restore_best_weights)
    and is installed on the device.  The best checkpoint's weights go to checkpoint_path when one was taken,
    the final model to save_path (``tfbundle.save_overlap``).  Everything random comes from `seed` through
    numpy: the initial state, the order of every epoch (``fit_plan``'s generator) and the dropout seed;
    TensorFlow's streams are not reproduced."""
    import os

    from . import models, tfbundle
    ctx = device if isinstance(device, _lib.Context) else _lib.default_context(device)
    x_train = np.asarray(x_train)
    labels = _class_labels(y_train, 'y_train')
    if x_train.dtype != np.uint8 or x_train.ndim != 4 or x_train.shape[3] not in weights.OD_CHANNELS or \
            len(x_train) != len(labels):
        raise ValueError(f'x_train {x_train.shape} {x_train.dtype}: expected uint8 [n,h,w,3] or [n,h,w,1], one '
                         'per label')
    ch = int(x_train.shape[3])
    nv = 0 if x_val is None else len(x_val)
    vx = vl = None
    if nv:
        vx, vl = np.asarray(x_val), _class_labels(y_val, 'y_val')
        if vx.dtype != np.uint8 or vx.shape[1:] != x_train.shape[1:] or len(vl) != nv:
            raise ValueError(f'x_val {vx.shape} {vx.dtype}: expected uint8 [n,{x_train.shape[1]},'
                             f'{x_train.shape[2]},{ch}], one per label')
    epochs = int(epochs)
    if epochs < 0 or batch_size < 1:
        raise ValueError('epochs must be >= 0 and batch_size >= 1')
    K = _n_classes(n_classes, y_train, y_val if nv else None)
    if not 2 <= K <= weights.OD_MAX_CLASSES:
        raise ValueError(f'n_classes {K} outside [2, {weights.OD_MAX_CLASSES}]')
    for what, l in (('y_train', labels), ('y_val', vl)):
        if l is not None and len(l) and (l.min() < 0 or l.max() >= K):
            raise ValueError(f'{what}: a label outside the {K} classes')
    if augmented:
        src, levels, labels = augment_plan(labels, K)
        x_train = _augment(ctx, x_train, src, levels)
    cw = cal_weighted_penalty(np.eye(K)[labels]) if weighted else np.ones(K)
    n = len(labels)
    rng_p = np.random.default_rng([int(seed), 1])       # fit_plan's generator of the epochs' orders
    perm = np.stack([rng_p.permutation(n) for _ in range(epochs)]).astype(np.int32) if epochs else \
        np.zeros((0, n), np.int32)
    drop_seed = int(np.random.default_rng([int(seed), 2]).integers(0, 2 ** 63))
    W0 = weights.initial_od(seed, K, ch)
    out, best, hist, ran, best_ep = ctx.od_train(weights.pack(weights.OD, W0, K, ch), x_train, labels, vx, vl, cw,
                                                 cosine_lr(epochs), perm, epochs, batch_size, drop_seed, patience,
                                                 1)
    model = models.OverlapDetectionModel(weights.unpack(weights.OD, out, K, ch), device=ctx)
    if checkpoint_path is not None and best is not None:
        os.makedirs(checkpoint_path, exist_ok=True)
        tfbundle.save_overlap(checkpoint_path, weights.unpack(weights.OD, best, K, ch))
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
        tfbundle.save_overlap(save_path, model.W)
    return model, History(hist, ran, best_ep)


def evaluation(model, x_eval, y_eval):
    """``OverlapDetector.evaluation`` (:513-543) for a K-class model: the argmax of ``model.predict(x_eval)``
    against y_eval (integers [n] or one-hot rows [n, K]) -> (confusion [K, K] float64, rows = ground truth,
    columns = predicted; recall and precision of class K - 1, the script's 'overlapped' class: NaN where the
    script divides 0 by 0).  Printed as the script prints them."""
    K = int(model.n_classes)
    truth = _class_labels(y_eval, 'y_eval')
    if len(truth) and (truth.min() < 0 or truth.max() >= K):
        raise ValueError(f'y_eval: a label outside the {K} classes')
    predicted = np.argmax(model.predict(x_eval), axis=1)
    if len(predicted) != len(truth):
        raise ValueError(f'x_eval / y_eval: {len(predicted)} predictions for {len(truth)} labels')
    confusion_matrix = np.zeros((K, K))
    np.add.at(confusion_matrix, (truth, predicted), 1)
    tp = confusion_matrix[K - 1, K - 1]
    fn = confusion_matrix[K - 1, :K - 1].sum()
    fp = confusion_matrix[:K - 1, K - 1].sum()
    with np.errstate(invalid='ignore', divide='ignore'):
        recall = np.float64(tp) / (tp + fn)
        precision = np.float64(tp) / (tp + fp)
    # rows = ground truth; cols = predicted
    print(confusion_matrix)
    print('Overlapped recall: ', recall, " precision: ", precision)
    return confusion_matrix, float(recall), float(precision)
