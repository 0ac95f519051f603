"""GPU: mmla_od_augment (od_aug.hip), the pyramid blur of augment_images, bit for bit against the numpy
restatement tests/pyr_ref.py (whose two independent versions tests/test_od_train_ref_cpu.py holds together),
with host and device pointers, and every MMLA_E_INVALID case of include/mmla.h."""
import numpy as np
import pytest

import pyr_ref
from mmla_audio_amd import _lib, overlap_detector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _images(seed, n, h, w):
    return np.random.default_rng([seed, n, h, w]).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# 8 x 9: every tap of every row and column touches a border; 16 x 21: w + 1 is no multiple of 4;
# 128 x 151 with three images: the LDS sizing.  Levels 0, 1, 2, 3, 8 mixed; src repeats and is out of order.
CASES = [(8, 9, 2, [1, 0, 1, 1, 0, 0], [8, 0, 1, 3, 2, 1]),
         (16, 21, 3, [2, 2, 0, 1, 0, 2, 1], [1, 2, 0, 8, 3, 3, 0]),
         (128, 151, 3, [2, 0, 1, 0, 2], [3, 1, 8, 0, 2])]


@pytest.mark.parametrize('h,w,n,src,levels', CASES)
def test_augment_equals_the_restatement_bit_for_bit(ctx, h, w, n, src, levels):
    img = _images(7, n, h, w)
    want = pyr_ref.augment(img, src, levels)
    got = ctx.od_augment(img, src, levels)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert not len(bad), (len(bad), bad[:5].tolist())
    for k, lv in enumerate(levels):
        if lv == 0:
            assert got[k].tobytes() == img[src[k]].tobytes()


def test_device_pointers_and_an_empty_call(ctx):
    import torch
    h, w, n, src, levels = CASES[1]
    img = _images(7, n, h, w)
    want = pyr_ref.augment(img, src, levels)
    d_img = torch.from_numpy(img).cuda()
    d_src = torch.tensor(src, dtype=torch.int32, device='cuda')
    d_lv = torch.tensor(levels, dtype=torch.int32, device='cuda')
    out = torch.zeros((len(src), h, w, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.od_augment_dev(d_img.data_ptr(), n, h, w, d_src.data_ptr(), d_lv.data_ptr(), len(src), out.data_ptr())
    ctx.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert d_img.cpu().numpy().tobytes() == img.tobytes(), 'the input was written'
    # a broken contract on device pointers: src and levels are clamped into range
    d_src2 = torch.tensor([-5, n + 3, 1], dtype=torch.int32, device='cuda')
    d_lv2 = torch.tensor([-1, 1, 99], dtype=torch.int32, device='cuda')
    out2 = torch.zeros((3, h, w, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.od_augment_dev(d_img.data_ptr(), n, h, w, d_src2.data_ptr(), d_lv2.data_ptr(), 3, out2.data_ptr())
    ctx.synchronize()
    assert out2.cpu().numpy().tobytes() == pyr_ref.augment(img, [0, n - 1, 1], [0, 1, 8]).tobytes()
    # m = 0
    empty = ctx.od_augment(img, [], [])
    assert empty.shape == (0, h, w, 3)
    ctx.od_augment_dev(d_img.data_ptr(), n, h, w, 0, 0, 0, 0)


def test_invalid_arguments_name_the_argument(ctx):
    h, w, n = 16, 21, 2
    img = _images(9, n, h, w)
    src = np.array([0, 1], np.int32)
    lv = np.array([1, 2], np.int32)
    out = np.empty((2, h, w, 3), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    good = dict(img=img, n=n, h=h, w=w, src=src, lv=lv, m=2, out=out)

    def rc(**over):
        a = dict(good, **over)
        r = ctx.lib.mmla_od_augment(ctx.h, p(a['img']), a['n'], a['h'], a['w'], p(a['src']), p(a['lv']), a['m'],
                                    p(a['out']), 0)
        return r, ctx.lib.mmla_last_error(ctx.h).decode()

    cases = [(dict(h=6), 'h 6'), (dict(h=130), 'h 130'), (dict(h=17), 'h 17'), (dict(w=7), 'w 7'),
             (dict(w=153), 'w 153'), (dict(w=20), 'w 20'), (dict(n=0), 'n 0'), (dict(m=-1), 'm -1'),
             (dict(img=None), 'null pointer'), (dict(src=None), 'null pointer'), (dict(lv=None), 'null pointer'),
             (dict(out=None), 'null pointer'), (dict(src=np.array([0, 2], np.int32)), 'src[1] = 2'),
             (dict(src=np.array([-1, 0], np.int32)), 'src[0] = -1'),
             (dict(lv=np.array([0, 9], np.int32)), 'levels[1] = 9'),
             (dict(lv=np.array([-1, 0], np.int32)), 'levels[0] = -1')]
    for over, word in cases:
        r, msg = rc(**over)
        assert r == -1 and 'od_augment' in msg and word in msg, (over, r, msg)
    assert rc()[0] == 0
    assert out.tobytes() == pyr_ref.augment(img, src, lv).tobytes()


def test_augment_images_is_the_plan_through_the_kernel(ctx):
    h, w = 16, 17
    labels = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.int32)            # 9 : 3
    img = _images(11, len(labels), h, w)
    out, new = overlap_detector.augment_images(img, labels, ctx)
    src, levels, want_labels = overlap_detector.augment_plan(labels)
    assert len(out) == 9 + 3 + 6 and levels[12:].tolist() == [1] * 3 + [2] * 3
    assert (new == want_labels).all() and out.tobytes() == pyr_ref.augment(img, src, levels).tobytes()
