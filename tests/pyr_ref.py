"""TEST INFRASTRUCTURE: numpy restatement of what ``mmla_od_augment`` (include/mmla.h) computes -- the pyramid
blur of ``OverlapDetector.augment_images`` (overlap_detector.py:198-220): ``cv.pyrDown`` then ``cv.pyrUp``,
level times, cropped once with ``src[:, :-1]``.  Stated from OpenCV's published uint8 pyramid code; OpenCV is
not available here: parity with OpenCV itself is unpinned (tests/test_od_train_ref_cpu.py compares where cv2
happens to be installed).

Written twice, independently, and the two must agree bit for bit:

  separable   a row pass into a uint16 intermediate, then a column pass (``impl='sep'``)
  direct      the 5 x 5 (pyrDown) / 3 x 3 (pyrUp) 2-D weighted sum in one step, int64 (``impl='direct'``)

Each channel alone; all arithmetic exact in integers.
"""
import numpy as np

K5 = (1, 4, 6, 4, 1)


def _r101(i, n):
    """BORDER_REFLECT_101: -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3"""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


# ---- separable ------------------------------------------------------------------------------------------------

def _down_sep(s):
    H, W = s.shape
    ho, wo = (H + 1) // 2, (W + 1) // 2
    s16 = s.astype(np.uint16)
    t = np.zeros((H, wo), np.uint16)
    for j in range(-2, 3):
        t += np.uint16(K5[j + 2]) * s16[:, _r101(2 * np.arange(wo) + j, W)]
    acc = np.zeros((ho, wo), np.uint32)
    for i in range(-2, 3):
        acc += np.uint32(K5[i + 2]) * t[_r101(2 * np.arange(ho) + i, H)].astype(np.uint32)
    return ((acc + 128) >> 8).astype(np.uint8)


def _up_rows16(s16):
    """the pyrUp rule along axis 1: [H, N] -> [H, 2 N]; s[-1] = s[1], s[N] = s[N-1]"""
    N = s16.shape[1]
    before = s16[:, [1] + list(range(N - 1))]
    after = s16[:, list(range(1, N)) + [N - 1]]
    e = np.empty((s16.shape[0], 2 * N), s16.dtype)
    e[:, 0::2] = before + 6 * s16 + after
    e[:, 1::2] = 4 * (s16 + after)
    return e


def _up_sep(s):
    e = _up_rows16(s.astype(np.uint16))                     # uint16 intermediate, at most 8 * 255
    v = _up_rows16(e.T.astype(np.uint32)).T
    return ((v + 32) >> 6).astype(np.uint8)


# ---- direct -------------------------------------------------------------------------------------------------

def _down_direct(s):
    H, W = s.shape
    ho, wo = (H + 1) // 2, (W + 1) // 2
    s64 = s.astype(np.int64)
    acc = np.zeros((ho, wo), np.int64)
    for i in range(-2, 3):
        rows = _r101(2 * np.arange(ho) + i, H)
        for j in range(-2, 3):
            cols = _r101(2 * np.arange(wo) + j, W)
            acc += K5[i + 2] * K5[j + 2] * s64[np.ix_(rows, cols)]
    return ((acc + 128) >> 8).astype(np.uint8)


def _up_taps(N):
    """per output index o < 2 N: three (source index, weight) taps of the 1-D pyrUp rule"""
    idx = np.zeros((2 * N, 3), np.int64)
    wt = np.zeros((2 * N, 3), np.int64)
    for x in range(N):
        nxt = x + 1 if x + 1 < N else N - 1             # replicate behind
        prv = x - 1 if x > 0 else 1                     # reflect before
        idx[2 * x] = (prv, x, nxt)
        wt[2 * x] = (1, 6, 1)
        idx[2 * x + 1] = (x, nxt, x)
        wt[2 * x + 1] = (4, 4, 0)
    return idx, wt


def _up_direct(s):
    H, W = s.shape
    s64 = s.astype(np.int64)
    iy, wy = _up_taps(H)
    ix, wx = _up_taps(W)
    v = np.zeros((2 * H, 2 * W), np.int64)
    for a in range(3):
        for b in range(3):
            v += wy[:, a, None] * wx[None, :, b] * s64[np.ix_(iy[:, a], ix[:, b])]
    return ((v + 32) >> 6).astype(np.uint8)


_IMPL = {'sep': (_down_sep, _up_sep), 'direct': (_down_direct, _up_direct)}


def pyr_down(plane, impl='sep'):
    """uint8 [H, W] -> [(H+1)/2, (W+1)/2]"""
    return _IMPL[impl][0](np.asarray(plane, np.uint8))


def pyr_up(plane, impl='sep'):
    """uint8 [H, W] -> [2 H, 2 W]"""
    return _IMPL[impl][1](np.asarray(plane, np.uint8))


def blur(img, level, impl='sep'):
    """img uint8 [h, w] or [h, w, c] -> the same shape: `level` rounds of pyrDown + pyrUp on every channel,
    the extra column kept through the levels and cropped once at the end; level 0 is a copy.  h even, w odd."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 3:
        return np.stack([blur(img[..., c], level, impl) for c in range(img.shape[2])], axis=-1)
    h, w = img.shape
    assert h % 2 == 0 and w % 2 == 1, (h, w)
    cur = img
    for _ in range(level):
        cur = pyr_up(pyr_down(cur, impl), impl)
    return cur[:, :w].copy()


def augment(images, src, levels, impl='sep'):
    """the arguments of mmla_od_augment -> uint8 [m, h, w, 3]"""
    images = np.asarray(images, np.uint8)
    out = np.empty((len(src),) + images.shape[1:], np.uint8)
    for k, (s, lv) in enumerate(zip(src, levels)):
        out[k] = blur(images[s], int(lv), impl)
    return out
