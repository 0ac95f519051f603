"""TEST INFRASTRUCTURE: numpy restatements for ``mmla_od_train`` (include/mmla.h): the AUC metric
(``tf.keras.metrics.AUC()`` at its defaults, overlap_detector.py:403, stated from Keras 2.6's published source;
TensorFlow is not available, parity with TF itself is unpinned) and OD's dropout keep-bits (site 2 of the
Philox stream tests/si_base_ref.py restates).
"""
import numpy as np

import si_base_ref

N_THR = 200
DROP_SITE, DROP_RATE, DROP_UNITS = 2, 0x40000000, 512


def thresholds():
    """float32 [200]: float32(0 - 1e-7), float32((i + 1) / 199.0) with the quotient in double, float32(1 + 1e-7)"""
    mid = [np.float32((i + 1) / 199.0) for i in range(N_THR - 2)]
    return np.array([np.float32(0.0 - 1e-7)] + mid + [np.float32(1.0 + 1e-7)], np.float32)


def auc_binary(pred, truth):
    """pred float32 [k] against truth bool [k]: integer TP / FP / TN / FN per threshold (positive iff
    pred > thr), recall and fpr with 0 for an empty denominator, the trapezoid sum in double -> float32"""
    pred = np.asarray(pred, np.float32).ravel()
    truth = np.asarray(truth).astype(bool).ravel()
    thr = thresholds()
    above = pred[None, :] > thr[:, None]                      # float32 against float32
    tp = (above & truth[None]).sum(axis=1).astype(np.int64)
    fp = (above & ~truth[None]).sum(axis=1).astype(np.int64)
    fn = int(truth.sum()) - tp
    tn = int((~truth).sum()) - fp
    rec = np.array([t / (t + f) if t + f else 0.0 for t, f in zip(tp.tolist(), fn.tolist())], np.float64)
    fpr = np.array([p / (p + t) if p + t else 0.0 for p, t in zip(fp.tolist(), tn.tolist())], np.float64)
    total = 0.0
    for t in range(N_THR - 1):
        total += (fpr[t] - fpr[t + 1]) * (rec[t] + rec[t + 1]) / 2.0
    return np.float32(total)


def auc(probs, labels):
    """multi_label=False: all 2 n entries of probs [n, 2] against the entries of the one-hot label rows"""
    probs = np.asarray(probs, np.float32).reshape(-1, 2)
    onehot = np.eye(2, dtype=bool)[np.asarray(labels).astype(np.int64) & 1]
    return auc_binary(probs.ravel(), onehot.ravel())


def threshold_margin(probs):
    """the smallest distance of any prob to any threshold"""
    p = np.asarray(probs, np.float64).ravel()
    return float(np.abs(p[:, None] - thresholds().astype(np.float64)[None]).min())


def on_threshold_case():
    """one sample of class 0 whose positive entry is exactly float32(50 / 199) and whose negative entry lies
    between thresholds 49 and 50 -> (probs [1, 2], the same with the positive entry one ulp higher)"""
    t50 = np.float32(50 / 199.0)
    on = np.array([[t50, np.float32(49.5 / 199.0)]], np.float32)
    nudged = on.copy()
    nudged[0, 0] = np.nextafter(t50, np.float32(1))
    return on, nudged


def drop_mask(seed, epoch, sample_ids):
    """-> uint8 [n, 512]; 1 = kept"""
    words = si_base_ref.drop_words(seed, epoch, sample_ids, DROP_SITE, DROP_UNITS)
    return (words >= np.uint32(DROP_RATE)).astype(np.uint8)
