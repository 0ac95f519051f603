"""GPU: the stationary gate's noise thresholds (nr.hip nr_noise_db_kernel + nr_noise_thresh_kernel), read back
with mmla_debug_nr_thresh, against tests/nr_ref.py thresholds64 -- oracle noise_threshold with every step in
float64 on the float32 samples.

Rule (the project's d32 rule, FACTOR 16): |got - th64| <= 16 x max(d32, 2^-24 max|th64|) on
every bin, d32 = max|noise_threshold - thresholds64| being the float32 restatement's own distance from the
float64 definition; all values finite.  The kernels follow the float32 definition with another summation
order, log10f and hypotf, so they may be as far from float64 as it is, times a margin.

Clips: white noise of 16 000 samples and of 2, 300, 513, 1 025 and 12 345 (below 513 samples the frame load
reflects more than once); a click (46 % of its dB cells raised by the top_db clamp), a half-muted clip
(35 %), a muted one (every cell is 10 log10 of the float32 subnormal next to 1e-40); the clips of the gate
cases.  Alone, and as one bank of mixed lengths, whose rows must be the single profiles bit for bit.

Each case prints ratio = max|got - th64| / max(d32, 2^-24 max|th64|) (bound: 16).  Measured on an MI355X:
white 2.06, white[:2] 0.62, [:300] 1.35, [:513] 1.12, [:1025] 1.36, [:12345] 1.58, click 1.59, half-muted 3.17
(the worst), muted 1.00 (-400.00003, the float32 restatement's value, on every bin), floored 1.84, base 1.86,
long 1.85; the bank's rows are the same bits.  |got - th64| itself is 1.3e-6 .. 1.0e-5 dB (muted: 3.1e-5).
"""
import ctypes

import numpy as np
import pytest

import nr_ref as R
from mmla_audio_amd import _lib

pytestmark = pytest.mark.gpu

FACTOR = 16.0


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def clips():
    x = R.noise_clips()
    for a in x.values():
        a.setflags(write=False)
    return x


def _check(got, clip, what):
    bound, th64 = R.thresh_bound(clip, FACTOR)
    assert got.dtype == np.float32 and got.shape == (R.NB,), (what, got.dtype, got.shape)
    err = float(np.abs(got.astype(np.float64) - th64).max())
    print(f'{what}: |got - th64| {err:.3e}  bound {bound:.3e}  ratio {err / (bound / FACTOR):.2f}')
    assert np.isfinite(got).all(), what
    assert err <= bound, f'{what}: {err:.3e} > {bound:.3e}'


@pytest.mark.parametrize('name', R.THRESH_CLIPS)
def test_single_profile(ctx, clips, name):
    ctx.nr_set_noise(clips[name])
    got = ctx.debug_nr_thresh()
    assert got.shape == (1, R.NB)
    _check(got[0], clips[name], name)


def test_mixed_length_bank(ctx, clips):
    ctx.nr_set_noise_bank([clips[name] for name in R.THRESH_CLIPS])
    got = ctx.debug_nr_thresh()
    assert got.shape == (len(R.THRESH_CLIPS), R.NB)
    for p, name in enumerate(R.THRESH_CLIPS):
        _check(got[p], clips[name], f'bank[{p}] {name}')
    for p, name in enumerate(R.THRESH_CLIPS):       # a profile does not depend on its neighbours
        ctx.nr_set_noise(clips[name])
        assert ctx.debug_nr_thresh()[0].tobytes() == got[p].tobytes(), name


def test_read_back_arguments(clips):
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.MmlaError) as e:               # no bank yet
            c.debug_nr_thresh()
        assert e.value.code == -1, e.value
        c.nr_set_noise_bank([clips['white'], clips['white[:300]']])
        n = ctypes.c_int64(0)
        buf = np.full(2 * R.NB + 1, 7.0, np.float32)
        assert c.lib.mmla_debug_nr_thresh(c.h, buf.ctypes.data, 2 * R.NB - 1, ctypes.byref(n)) == -1
        assert n.value == 2 and (buf == 7.0).all()             # too small: the size is reported, nothing written
        assert c.lib.mmla_debug_nr_thresh(c.h, None, 2 * R.NB, None) == -1
        assert c.lib.mmla_debug_nr_thresh(c.h, buf.ctypes.data, 2 * R.NB, None) == 0
        assert buf[-1] == 7.0 and buf[:-1].reshape(2, R.NB).tobytes() == c.debug_nr_thresh().tobytes()
    finally:
        c.close()
