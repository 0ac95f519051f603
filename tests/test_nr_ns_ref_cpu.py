"""CPU: the non-stationary gate's restatement (tests/nr_ns_ref.py) is consistent with itself -- the
explicit recurrence the GPU kernel walks is scipy's filtfilt, the coefficient is the published one,
and the one deviation from the library (mask 0 where the smoothed floor is 0) fires only for all-zero
buffers."""
import numpy as np
import pytest

import nr_ns_ref as ref


@pytest.fixture(scope='module')
def planes():
    """(A, smooth) of every buffer of every parity input, computed once"""
    return {name: [ref.chunk_smooth(buf) for _, _, buf in ref.buffers(y)]
            for name, y in ref.named_inputs().items()}


def test_coefficient_at_16k():
    assert ref.coefficient(2.0, 16000) == 0.007968063999744002


def test_recurrence_is_filtfilt(planes):
    b = ref.coefficient()
    for name in ('tone', 'speech', 'noise', 'speech[:700]', 'stale0', 'stale2'):
        for A, smooth in planes[name]:
            err = np.abs(ref.smooth_recurrence(A, b) - smooth).max() / smooth.max()
            assert err <= 1e-13, (name, err)
    A = planes['speech'][0][0]
    b2 = ref.coefficient(0.5)
    err = np.abs(ref.smooth_recurrence(A, b2) - ref.smooth_filtfilt(A, b2)).max()
    assert err <= 1e-13 * ref.smooth_filtfilt(A, b2).max()


def test_all_zero_signal_gives_zeros():
    for n in (1, 4000, 40000):
        out = ref.reduce_noise(np.zeros(n, np.float32))
        assert out.dtype == np.float32 and np.array_equal(out, np.zeros(n, np.float32))


def test_floor_is_positive_on_every_other_input(planes):
    """so the smooth == 0 rule is inert on the parity inputs"""
    for name, bufs in planes.items():
        for _, smooth in bufs:
            assert smooth.min() > 0, (name, smooth.min())


def test_mask_is_a_sigmoid_in_0_1(planes):
    A, smooth = planes['speech'][0]
    m = ref.mask_of(A, smooth)
    assert np.isfinite(m).all() and m.min() >= 0 and m.max() <= 1
    x = (A - smooth) / smooth
    assert x.min() >= -1.0
