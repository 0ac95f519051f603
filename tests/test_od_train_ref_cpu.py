"""CPU: the restatements behind the OD from-scratch trainer (tests/pyr_ref.py, tests/od_train_ref.py) hold
their own known answers, and the Python pieces that need no device -- ``augment_plan``, ``weights.initial_od``,
the ABI table -- do what include/mmla.h and the reference script state."""
import ctypes
import os

import numpy as np
import pytest

import od_train_ref as tr
import pyr_ref
from mmla_audio_amd import _lib, overlap_detector, weights

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((8, 9), (16, 21), (128, 151))
LEVELS = (1, 2, 3, 8)


def _image(seed, h, w):
    return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w), dtype=np.uint8)


# ---- the pyramid -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('h,w', SIZES)
def test_separable_and_direct_pyramids_agree_bit_for_bit(h, w):
    img = _image(1, h, w)
    for level in LEVELS:
        a, b = pyr_ref.blur(img, level, 'sep'), pyr_ref.blur(img, level, 'direct')
        assert a.shape == (h, w) and a.dtype == np.uint8
        assert a.tobytes() == b.tobytes(), (h, w, level)
    assert pyr_ref.blur(img, 0).tobytes() == img.tobytes()
    assert (pyr_ref.blur(img, 1) != img).any()


@pytest.mark.parametrize('impl', ['sep', 'direct'])
def test_constant_and_ramp_images_are_fixed_points(impl):
    for v in (0, 1, 127, 255):
        img = np.full((16, 21), v, np.uint8)
        for level in LEVELS:
            assert (pyr_ref.blur(img, level, impl) == v).all(), (v, level)
    h, w = 128, 151
    ramp_x = np.broadcast_to(np.arange(w, dtype=np.uint8)[None], (h, w))
    assert (pyr_ref.blur(ramp_x, 1, impl)[:, 4:147] == ramp_x[:, 4:147]).all()
    ramp_y = np.broadcast_to(np.arange(h, dtype=np.uint8)[:, None], (h, w))
    assert (pyr_ref.blur(ramp_y, 1, impl)[4:124] == ramp_y[4:124]).all()


@pytest.mark.parametrize('impl', ['sep', 'direct'])
@pytest.mark.parametrize('y0,x0', [(8, 10), (9, 11), (8, 11)])
def test_pyr_down_of_one_bright_pixel(impl, y0, x0):
    s = np.zeros((16, 21), np.uint8)
    s[y0, x0] = 255
    d = pyr_ref.pyr_down(s, impl)
    want = np.zeros((8, 11), np.int64)
    for y in range(8):
        for x in range(11):
            i, j = y0 - 2 * y, x0 - 2 * x
            if abs(i) <= 2 and abs(j) <= 2:
                want[y, x] = (pyr_ref.K5[i + 2] * pyr_ref.K5[j + 2] * 255 + 128) >> 8
    assert want.any() and (d == want).all()


def test_the_extra_column_is_cropped_once():
    h, w = 128, 151
    img = _image(2, h, w)
    once = pyr_ref.blur(img, 2)
    twice = pyr_ref.blur(pyr_ref.blur(img, 1), 1)            # cropped after level 1, then level 1 again
    assert (once[:, :w - 4] == twice[:, :w - 4]).all()       # the lost column reaches columns >= w - 3 only
    assert (once[:, w - 4:] != twice[:, w - 4:]).any()


def test_against_opencv_where_it_is_installed():
    cv2 = pytest.importorskip('cv2')
    for h, w in SIZES:
        img = np.random.default_rng([3, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)
        for level in LEVELS:
            src = img
            for _ in range(level):
                src = cv2.pyrUp(cv2.pyrDown(src))
            assert pyr_ref.blur(img, level).tobytes() == np.ascontiguousarray(src[:, :-1]).tobytes(), (h, w, level)


# ---- augment_plan -----------------------------------------------------------------------------------------

def test_augment_plan_balances_like_the_script():
    # counts (9, 3, 1): ratios 0, 2, 8 -> class 1 gets copies at levels {1, 2}, class 2 at levels 1..8
    labels = np.array([0] * 9 + [1] * 3 + [2], np.int64)
    labels = labels[np.random.default_rng(4).permutation(len(labels))]
    src, levels, new = overlap_detector.augment_plan(labels)
    n = len(labels)
    assert src.dtype == levels.dtype == new.dtype == np.int32
    assert src[:n].tolist() == list(range(n)) and not levels[:n].any()      # the originals, in input order
    c1, c2 = np.flatnonzero(labels == 1).tolist(), int(np.flatnonzero(labels == 2)[0])
    assert src[n:n + 6].tolist() == c1 + c1 and levels[n:n + 6].tolist() == [1] * 3 + [2] * 3   # by i, by image
    assert src[n + 6:].tolist() == [c2] * 8 and levels[n + 6:].tolist() == list(range(1, 9))
    assert (new == labels[src]).all() and new[n:].tolist() == [1] * 6 + [2] * 8
    # counts (10, 3, 1): class 1 still gets levels {1, 2} (round(2.33) = 2); class 2's ratio is 10 / 1 - 1 = 9,
    # range(9) is levels 1..9, one more than the MMLA_OD_AUG_MAX_LEVELS = 8 built
    assert round(10 / 3 - 1) == 2 and round(10 / 1 - 1) == 9
    with pytest.raises(ValueError, match='class 2'):
        overlap_detector.augment_plan(np.array([0] * 10 + [1] * 3 + [2]))


def test_augment_plan_rounds_half_to_even():
    assert round(0.5) == 0 and round(1.5) == 2 and round(8.5) == 8
    src, levels, _ = overlap_detector.augment_plan(np.array([0, 0, 0, 1, 1]))     # ratio 0.5 -> no copy
    assert len(src) == 5 and not levels.any()
    src, levels, _ = overlap_detector.augment_plan(np.array([0] * 5 + [1] * 2))   # ratio 1.5 -> two copies
    assert src[7:].tolist() == [5, 6, 5, 6] and levels[7:].tolist() == [1, 1, 2, 2]
    _, levels, _ = overlap_detector.augment_plan(np.array([0] * 19 + [1] * 2))    # ratio 8.5 -> eight
    assert levels.max() == 8


def test_augment_plan_rejects_what_it_cannot_balance():
    with pytest.raises(ValueError, match='class 1'):
        overlap_detector.augment_plan(np.array([0, 0, 2]))
    with pytest.raises(ValueError, match='class 2'):
        overlap_detector.augment_plan(np.array([0, 1, 1]), n_classes=3)
    with pytest.raises(ValueError, match='9 copies'):
        overlap_detector.augment_plan(np.array([0] * 10 + [1]))
    with pytest.raises(ValueError):
        overlap_detector.augment_plan(np.array([0.0, 1.0]))
    with pytest.raises(ValueError):
        overlap_detector.augment_plan(np.array([0, -1]))


# ---- AUC ----------------------------------------------------------------------------------------------------

def test_auc_thresholds_and_known_answers():
    thr = tr.thresholds()
    assert thr.dtype == np.float32 and thr.shape == (200,)
    assert thr[0] < 0 and thr[-1] > 1 and (np.diff(thr) > 0).all()
    assert thr[50] == np.float32(50 / 199.0)
    # a perfect separator
    labels = np.array([0, 1, 1, 0, 1])
    probs = np.where(np.eye(2)[labels] == 1, 0.9, 0.1).astype(np.float32)
    assert tr.auc(probs, labels) == np.float32(1.0)
    # all-equal predictions
    assert tr.auc(np.full((6, 2), 0.5, np.float32), np.array([0, 1, 0, 0, 1, 1])) == np.float32(0.5)
    # a single class among the binary entries: no negatives (or no positives) gives 0
    assert tr.auc_binary(np.array([0.2, 0.7, 0.9], np.float32), np.array([1, 1, 1])) == 0.0
    assert tr.auc_binary(np.array([0.2, 0.7, 0.9], np.float32), np.array([0, 0, 0])) == 0.0
    # strictly above: a prob equal to a threshold is not positive at it
    t50 = np.float32(50 / 199.0)
    on, nudged = tr.on_threshold_case()
    above = on.ravel()[None] > thr[:, None]
    assert on[0, 0] == t50 and above[49, 0] and not above[50, 0]
    assert (nudged.ravel()[None] > thr[:, None])[50, 0]
    # the negative entry lies between thresholds 49 and 50: on the threshold both entries flip together
    # (the chord, 0.5); one ulp above it the positive entry outlasts the negative (1)
    assert tr.auc(on, [0]) == np.float32(0.5) and tr.auc(nudged, [0]) == np.float32(1.0)


def test_od_drop_mask_restatement_rate():
    m = tr.drop_mask(1234567, 3, np.arange(64))
    assert m.shape == (64, 512) and m.dtype == np.uint8
    n = m.size
    assert abs(m.mean() - 0.75) <= 4 * np.sqrt(0.75 * 0.25 / n)
    assert (tr.drop_mask(1234567, 4, np.arange(64)) != m).any()


# ---- the initial state --------------------------------------------------------------------------------------

def test_initial_od_state():
    W = weights.initial_od(seed=3)
    weights.check(weights.OD, W)
    for name, shape, role in weights.od_spec():
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
    again, other = weights.initial_od(seed=3), weights.initial_od(seed=4)
    assert all((W[k] == again[k]).all() for k in W)
    assert (W['layer_with_weights-0/kernel'] != other['layer_with_weights-0/kernel']).any()
    with pytest.raises(NotImplementedError):
        weights.initial(weights.OD)
    # the SI state keeps its draws: the shared body is seeded as before
    si = weights.initial(weights.SI, seed=3, n_classes=4)
    rng = np.random.default_rng(np.random.PCG64(0x696E6974 + 7919 * 3))
    lim = np.sqrt(6.0 / (4 * 39 + 4 * 32))
    assert (si['layer_with_weights-0/kernel'] == rng.uniform(-lim, lim, (4, 39, 32)).astype(np.float32)).all()


# ---- ABI ----------------------------------------------------------------------------------------------------

def test_abi_and_keywords():
    import inspect
    names = ('mmla_od_augment', 'mmla_od_auc', 'mmla_od_drop_mask', 'mmla_od_train')
    assert all(n in _lib.SIGNATURES for n in names)
    header = open(os.path.join(HERE, '..', 'include', 'mmla.h')).read()
    assert f'#define MMLA_OD_AUG_MAX_LEVELS {_lib.OD_AUG_MAX_LEVELS}' in header
    assert 'parity with OpenCV unpinned' in header
    p = inspect.signature(overlap_detector.train_model).parameters
    assert [p[k].default for k in ('weighted', 'augmented', 'seed', 'patience')] == [False, False, 0, 10]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('epochs', 'batch_size', 'save_path'))
    h = overlap_detector.History(np.arange(21, dtype=np.float32).reshape(3, 7), 2, 1)
    assert list(h.history) == list(overlap_detector.HISTORY_KEYS) and h.history['val_auc'] == [6.0, 13.0]
    assert h.best_epoch == 1 and h.epochs_run == 2
    for fn in ('od_train', 'od_drop_mask', 'od_augment', 'od_auc'):
        assert hasattr(_lib.Context, fn) and hasattr(_lib.Context, fn + '_dev')
    if not os.path.exists(_lib.LIB_PATH):       # not built: the half above still stands
        return
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = _lib.SIGNATURES[name]
    assert lib.mmla_od_augment(None, None, 0, 0, 0, None, None, 0, None, 0) == -1
    assert lib.mmla_od_auc(None, None, None, 0, None, 0) == -1
    assert lib.mmla_od_drop_mask(None, 0, 0, None, 0, None, 0) == -1
    assert lib.mmla_od_train(None, None, 0, None, None, 0, None, None, 0, 0, 0, None, 0, 0, None, None, 0, 0, 0,
                             None, None, None, None, None, 0) == -1
