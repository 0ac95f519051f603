"""CPU: the gray / viridis image rule and the one-channel OD network's layouts (tests/od_imgtype_cases.py).

The colour maps are pinned three ways: the fixture tests/golden/cmap_lut.npz, the tables compiled into the
library (mmla_debug_od_image_lut) and, where matplotlib is installed, matplotlib's own.  The rule the GPU tests hold
the front-end to is checked against ``plt.imsave`` itself, on every float32 value at and next to a bin edge."""
import io

import numpy as np
import pytest

import od_finetune_cases as C
import od_imgtype_cases as T
import pyr_ref
from mmla_audio_amd import _lib, overlap_detector, tfbundle, weights

OD = weights.OD


# ---- 1. the colour maps -----------------------------------------------------------------------------------------

def test_fixture_library_and_matplotlib_hold_the_same_tables():
    luts = T.luts()
    for name in T.TYPES:
        assert np.array_equal(_lib.od_image_lut(name), luts[name]), f'{name}: library != fixture'
    gray = luts['gray']
    assert (gray[:, 0] == gray[:, 1]).all() and (gray[:, 1] == gray[:, 2]).all()
    assert gray[0, 0] == 0 and gray[255, 0] == 255 and (np.diff(gray[:, 0].astype(int)) >= 0).all()
    with pytest.raises(ValueError):
        _lib.od_image_lut('zcr')
    try:
        import matplotlib
    except ImportError:
        return                                     # only the comparison with matplotlib itself is left out
    for name in T.TYPES:
        want = matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3]
        assert np.array_equal(luts[name], want), f'{name}: fixture != matplotlib {matplotlib.__version__}'


# ---- 2. the rule is plt.imsave ----------------------------------------------------------------------------------

def _imsave_rgba(norm, name):
    import matplotlib.pyplot as plt
    buf = io.BytesIO()
    plt.imsave(buf, norm, origin='lower', cmap=name, format='png')
    buf.seek(0)
    rgba = plt.imread(buf, format='png')            # float32 in [0, 1]: k / 255 of the stored bytes
    return np.rint(rgba * 255.0).astype(np.uint8)


def _edge_values():
    """float32 [128, 151]: 0, 1, every k / 256 and its two float32 neighbours, the rest random in [0, 1)"""
    k = (np.arange(1, 256) / 256.0).astype(np.float32)
    vals = np.concatenate([[0.0, 1.0], k, np.nextafter(k, np.float32(0)), np.nextafter(k, np.float32(1)),
                           [np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(0), np.float32(1))]])
    rng = np.random.default_rng(5)
    a = rng.random(128 * 151).astype(np.float32)
    a[:vals.size] = vals.astype(np.float32)
    return rng.permutation(a).reshape(128, 151)


@pytest.mark.parametrize('name', T.TYPES)
def test_rule_equals_imsave_on_every_bin_edge_and_on_nan(name):
    pytest.importorskip('matplotlib')
    a = _edge_values()
    assert a.min() == 0.0 and a.max() == 1.0         # imsave's autoscale is then the identity
    got = _imsave_rgba(a, name)
    assert np.array_equal(got[..., :3], T.rule(a, name))
    assert (got[..., 3] == 255).all()
    idx = T.index(a)
    assert idx.min() == 0 and idx.max() == 255 and len(np.unique(idx)) == 256
    silent = _imsave_rgba(np.full((128, 151), np.nan, np.float32), name)
    assert not silent.any()                          # RGBA (0, 0, 0, 0)
    assert not T.rule(np.full((128, 151), np.nan, np.float32), name).any()
    # (normalize_matrix gives a clip all NaN or none: 0 / 0 of a constant matrix)


# ---- 3. layouts -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', (2, 3, 8))
@pytest.mark.parametrize('ch', (1, 3))
def test_spec_pack_unpack_and_layout_of(K, ch):
    spec = weights.od_spec(K, ch)
    assert spec[0][1] == (1, 1, ch, 16) and spec[-2][1] == (512, K)
    assert [s[0] for s in spec] == [s[0] for s in weights.od_spec(K)]
    assert [s[1] for s in spec[1:]] == [s[1] for s in weights.od_spec(K)[1:]]
    n = weights.n_params(OD, K, ch)
    assert n == weights.n_params(OD, K) - (32 if ch == 1 else 0)
    assert weights.od_layout_of(n) == (K, ch)
    W = weights.synthetic(OD, seed=4, n_classes=K, channels=ch)
    assert weights.od_channels(W) == ch and weights.od_classes(W) == K
    blob = weights.pack(OD, W, K, ch)
    assert blob.size == n and blob.dtype == np.float32
    back = weights.unpack(OD, blob, K, ch)
    assert all(back[k].tobytes() == W[k].tobytes() and back[k].shape == W[k].shape for k in W)
    with pytest.raises(ValueError):
        weights.pack(OD, W, K, 4 - ch)               # the other layout's check refuses the stem
    W0 = weights.initial_od(3, K, ch)
    assert W0['layer_with_weights-0/kernel'].shape == (1, 1, ch, 16)
    if ch == 3:
        assert weights.od_classes_of(n) == K


def test_no_two_layouts_share_a_size():
    sizes = {}
    for K in range(2, weights.OD_MAX_CLASSES + 1):
        for ch in weights.OD_CHANNELS:
            sizes.setdefault(weights.n_params(OD, K, ch), []).append((K, ch))
    assert all(len(v) == 1 for v in sizes.values()), sizes
    for n, ((K, ch),) in sizes.items():
        assert weights.od_layout_of(n) == (K, ch)
    for bad in (min(sizes) - 1, max(sizes) + 1, min(sizes) + 32 + 1):
        with pytest.raises(ValueError):
            weights.od_layout_of(bad)
    with pytest.raises(ValueError):
        weights.od_spec(2, 2)


# ---- 4. the bundle ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', (2, 3))
def test_one_channel_model_round_trips_through_the_bundle(tmp_path, K):
    W = T.synthetic1(6, K)
    tfbundle.save_overlap(str(tmp_path), W)
    shapes = tfbundle.variable_shapes(str(tmp_path / 'variables' / 'variables.index'))
    assert tuple(shapes['layer_with_weights-0/kernel']) == (1, 1, 1, 16)
    kind, k, head, _ = tfbundle.layout(shapes)
    assert (kind, k, head) == (OD, K, _lib.HEAD_SOFTMAX)
    back, (bkind, bk, _) = tfbundle.load_bundle(str(tmp_path), with_layout=True)
    assert (bkind, bk) == (OD, K) and set(back) == set(W)
    assert all(back[n].tobytes() == W[n].tobytes() and back[n].shape == W[n].shape for n in W)
    assert weights.od_channels(back) == 1


# ---- 5. augmentation --------------------------------------------------------------------------------------------

class _HostAugment(_lib.Context):
    """a context whose od_augment is the numpy restatement: what overlap_detector does around the kernel"""

    def __init__(self):
        self.h = None
        self.calls = []

    def od_augment(self, img, src, levels):
        self.calls.append(np.asarray(img).shape)
        return pyr_ref.augment(img, src, levels)


def test_augment_images_on_one_channel_is_channel_0_of_three():
    rng = np.random.default_rng(8)
    img1 = rng.integers(0, 256, (7, 20, 23, 1)).astype(np.uint8)
    labels = np.array([0, 0, 0, 0, 0, 1, 1], np.int32)          # class 1 gets round(5 / 2 - 1) = 2 copies
    ctx = _HostAugment()
    got, new_labels = overlap_detector.augment_images(img1, labels, ctx)
    assert ctx.calls == [(7, 20, 23, 3)]                          # widened for the three-channel kernel
    src, levels, want_labels = overlap_detector.augment_plan(labels)
    assert got.shape == (len(src), 20, 23, 1) and got.dtype == np.uint8 and levels.max() == 2
    assert np.array_equal(new_labels, want_labels)
    img3 = np.repeat(img1, 3, axis=3)
    got3, _ = overlap_detector.augment_images(img3, labels, _HostAugment())
    assert np.array_equal(got[..., 0], got3[..., 0])
    assert (got3[..., 0] == got3[..., 1]).all() and (got3[..., 1] == got3[..., 2]).all()
    for k in range(len(src)):                                     # the plane itself against the restatement
        assert np.array_equal(got[k, :, :, 0], pyr_ref.blur(img1[src[k], :, :, 0], int(levels[k]), 'direct'))
    with pytest.raises(ValueError):
        overlap_detector.augment_images(np.zeros((7, 20, 23, 2), np.uint8), labels, ctx)


# ---- 6. the gradient cases' conditions --------------------------------------------------------------------------

@pytest.mark.parametrize('h,w,B', list(T.GRAD_CASES))
def test_one_channel_gradient_cases_have_their_margins(h, w, B):
    W, img, _, _ = T.grad_case(h, w, B)
    assert img.shape == (B, h, w, 1) and W['layer_with_weights-0/kernel'].shape == (1, 1, 1, 16)
    r = T.grad_ref(h, w, B)['f64']
    m = r[3]
    print(h, w, B, m)
    assert m['pool'] >= C.MARGIN and m['leaky'] >= C.MARGIN, m
    g = r[1]['layer_with_weights-0/kernel']
    assert g.shape == (1, 1, 1, 16) and np.abs(g).max() > 0
