"""GPU: the batched SSIM kernel (mmla_ssim_u8, csrc/ssim.hip) against the float64 restatement of
scikit-image's structural_similarity (tests/ssim_ref.py), and the drop-ins on top of it.

Tolerance 2e-6: the kernel forms the window sums as exact integers and does the rest in float32 --
about six roundings of 2^-24 on |S| <= 1 per window plus the float32 summation; the same arithmetic
on the CPU stays within 1.3e-7 of float64 on 40 adversarial pairs, so 2e-6 leaves ~15 x margin.
Shapes beyond the OD geometry: a single window, sizes that are no multiple of anything, 4 channels,
and rows wider than one workgroup's 512 elements (the kernel then walks column chunks)."""
import numpy as np
import pytest

import ssim_ref
from mmla_audio_amd import _lib
from oracle import synth

pytestmark = pytest.mark.gpu

TOL = 2e-6


@pytest.fixture(scope='module')
def ctx():
    return _lib.Context(0)


@pytest.fixture(scope='module')
def od_pairs(ctx):
    """six pairs [6,128,151,3]: random vs random, an image vs itself, vs itself +-3, column-constant
    vs perturbed, all-0 vs all-255, two front-end images; shared read-only"""
    rng = np.random.default_rng(41)
    shape = (128, 151, 3)
    r0 = rng.integers(0, 256, shape, dtype=np.uint8)
    r1 = rng.integers(0, 256, shape, dtype=np.uint8)
    near = np.clip(r0.astype(int) + rng.integers(-3, 4, shape), 0, 255).astype(np.uint8)
    col = np.broadcast_to(rng.integers(0, 256, (1, 151, 3), dtype=np.uint8), shape).copy()
    colp = np.clip(col.astype(int) + rng.integers(-1, 2, shape), 0, 255).astype(np.uint8)
    fe = ctx.od_features(synth.batch(0, 2, 24000), db=False, norm=False, zcr=False)['img']
    a = np.stack([r0, r0, r0, col, np.zeros(shape, np.uint8), fe[0]])
    b = np.stack([r1, r0, near, colp, np.full(shape, 255, np.uint8), fe[1]])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _ref(a, b):
    return np.array([ssim_ref.ssim(x, y) for x, y in zip(a, b)])


def test_od_geometry_matches_reference(ctx, od_pairs):
    a, b = od_pairs
    got = ctx.ssim_u8(a, b)
    want = _ref(a, b)
    err = np.abs(got.astype(np.float64) - want)
    print('ssim', got, 'max err', err.max())
    assert got.dtype == np.float32 and got.shape == (6,)
    assert got[1] == 1.0                      # an image against itself: exactly 1
    assert err.max() <= TOL, (got, want)


@pytest.mark.parametrize('shape', [(1, 7, 7, 1), (2, 8, 9, 3), (3, 16, 40, 4), (1, 10, 600, 1),
                                   (2, 9, 200, 3), (2, 9, 140, 4)])
def test_other_shapes_match_reference(ctx, shape):
    rng = np.random.default_rng(42 + shape[2])
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-40, 41, shape), 0, 255).astype(np.uint8)
    b[-1] = rng.integers(0, 256, shape[1:], dtype=np.uint8)
    got = ctx.ssim_u8(a, b)
    err = np.abs(got.astype(np.float64) - _ref(a, b))
    print(shape, got, 'max err', err.max())
    assert err.max() <= TOL
    assert np.array_equal(ctx.ssim_u8(a, a), np.ones(shape[0], np.float32))


def test_bit_reproducible_across_batch_size_and_position(ctx, od_pairs):
    a, b = od_pairs
    whole = ctx.ssim_u8(a, b)
    for k in range(6):
        assert ctx.ssim_u8(a[k:k + 1], b[k:k + 1])[0].tobytes() == whole[k].tobytes()
        assert np.float32(ctx.ssim_u8(a[k], b[k])).tobytes() == whole[k].tobytes()
    perm = np.array([4, 2, 5, 0, 3, 1])
    assert ctx.ssim_u8(a[perm], b[perm]).tobytes() == whole[perm].tobytes()


def test_device_pointers_equal_host_pointers(ctx, od_pairs):
    import torch
    a, b = od_pairs
    ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    out = torch.zeros(6, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.ssim_u8_dev(ta.data_ptr(), tb.data_ptr(), 6, 128, 151, 3, out.data_ptr())
    ctx.synchronize()
    assert out.cpu().numpy().tobytes() == ctx.ssim_u8(a, b).tobytes()


def test_edge_cases(ctx):
    e = np.zeros((0, 16, 16, 3), np.uint8)
    assert ctx.ssim_u8(e, e).shape == (0,)
    with pytest.raises(_lib.MmlaError):
        ctx.ssim_u8(np.zeros((1, 6, 16, 3), np.uint8), np.zeros((1, 6, 16, 3), np.uint8))
    with pytest.raises(_lib.MmlaError):
        ctx.ssim_u8(np.zeros((1, 16, 6, 3), np.uint8), np.zeros((1, 16, 6, 3), np.uint8))
    with pytest.raises(_lib.MmlaError):
        ctx.ssim_u8(np.zeros((1, 16, 16, 2), np.uint8), np.zeros((1, 16, 16, 2), np.uint8))


def test_structural_similarity_dropin(od_pairs):
    from mmla_audio_amd.metrics import structural_similarity
    a, b = od_pairs
    s3 = structural_similarity(a[2], b[2], multichannel=True)
    assert abs(s3 - ssim_ref.ssim(a[2], b[2])) <= TOL
    assert abs(structural_similarity(a[5], b[5], channel_axis=-1, win_size=7, data_range=255) -
               ssim_ref.ssim(a[5], b[5])) <= TOL
    s2 = structural_similarity(a[0][..., 0], b[0][..., 0])
    assert abs(s2 - ssim_ref.ssim(a[0][..., 0], b[0][..., 0])) <= TOL


def test_compare_images_dropin(tmp_path, capsys, od_pairs):
    from mmla_audio_amd.metrics import compare_images
    from mmla_audio_amd.overlap_features_generator import write_png_rgba
    a, b = od_pairs
    p = [str(tmp_path / f'{k}.png') for k in range(3)]
    write_png_rgba(p[0], a[0])
    write_png_rgba(p[1], b[0])     # random vs random: similarity ~0.01
    write_png_rgba(p[2], b[2])     # the first image +-3: similarity 0.9996
    assert compare_images(p[0], p[1]) is True
    assert 'The similarity is too low' in capsys.readouterr().out
    assert compare_images(p[0], p[2]) is False
    assert capsys.readouterr().out == ''
    assert compare_images(p[0], p[2], threshold=0.9999) is True
    assert compare_images(p[0], p[0], threshold=1.0) is False     # exactly 1 is not below 1
