"""CPU: the float64 SSIM restatement the GPU tests compare against (tests/ssim_ref.py) is itself
checked against the definition, the kernel's integer form against the restatement, and the drop-in
``mmla_audio_amd.metrics.structural_similarity`` refuses what is not built before it touches the
library."""
import numpy as np
import pytest

import ssim_ref


def _pairs():
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, (9, 10, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (9, 10, 3), dtype=np.uint8)
    near = np.clip(a.astype(int) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
    col = np.broadcast_to(rng.integers(0, 256, (1, 10, 3), dtype=np.uint8), a.shape).copy()
    return a, b, near, col


def test_restatement_matches_brute_force():
    a, b, near, col = _pairs()
    for x, y in ((a, b), (a, near), (col, near), (a[..., 0], b[..., 0])):
        assert abs(ssim_ref.ssim(x, y) - ssim_ref.ssim_brute(x, y)) < 1e-12


def test_identical_images_give_one():
    a, _, _, col = _pairs()
    assert ssim_ref.ssim(a, a) == 1.0
    assert ssim_ref.ssim(col, col) == 1.0
    z = np.zeros((12, 8, 3), np.uint8)
    assert ssim_ref.ssim(z, z) == 1.0


def test_symmetric():
    a, b, near, _ = _pairs()
    assert abs(ssim_ref.ssim(a, b) - ssim_ref.ssim(b, a)) < 1e-15
    assert abs(ssim_ref.ssim(a, near) - ssim_ref.ssim(near, a)) < 1e-15


def test_integer_form_equals_restatement():
    rng = np.random.default_rng(32)
    a, b, near, col = _pairs()
    big = rng.integers(0, 256, (40, 33, 4), dtype=np.uint8)
    big2 = rng.integers(0, 256, (40, 33, 4), dtype=np.uint8)
    lo, hi = np.zeros((16, 16, 1), np.uint8), np.full((16, 16, 1), 255, np.uint8)
    for x, y in ((a, b), (a, near), (col, near), (a, a), (big, big2), (lo, hi), (hi, hi)):
        assert abs(ssim_ref.ssim_integer_form(x, y) - ssim_ref.ssim(x, y)) < 1e-12


def test_dropin_rejects_what_is_not_built(monkeypatch):
    from mmla_audio_amd import _lib, metrics

    def no_library(*a, **k):
        raise AssertionError('the library was loaded')

    monkeypatch.setattr(_lib, 'load_library', no_library)
    monkeypatch.setattr(_lib, 'default_context', no_library)
    u2 = np.zeros((16, 16), np.uint8)
    u3 = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        metrics.structural_similarity(u2.astype(np.float32), u2.astype(np.float32))
    with pytest.raises(NotImplementedError):
        metrics.structural_similarity(u2, u2, gaussian_weights=True)
    with pytest.raises(NotImplementedError):
        metrics.structural_similarity(u2, u2, win_size=11)
    with pytest.raises(NotImplementedError):
        metrics.structural_similarity(u3, u3)
    with pytest.raises(NotImplementedError):
        metrics.structural_similarity(u3, u3, multichannel=True, full=True)
    with pytest.raises(NotImplementedError):
        metrics.structural_similarity(u2, u2, data_range=1.0)
