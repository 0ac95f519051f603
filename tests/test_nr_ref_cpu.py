"""CPU: the conditions the stationary gate's GPU tests (test_gpu_noisereduce.py, test_gpu_nr_thresh.py) rest
on, asserted on the reference alone with the reference's own float32 thresholds (tests/nr_ref.py).

  decided      every gate input keeps every (bin, frame) cell, and every bin's top_db floor, at least GAP =
               1e-9 dB from its threshold: two float64 evaluations of a dB value agree to ~1e-12 dB, so the
               kernel and the reference take the same decisions and |got - want| <= 1e-6 max|want| can be
               asked of every sample.  (The GPU tests assert the same on the thresholds the device holds.)
  floored      on the floored pair the signal's top_db floor lies above 64..449 of the 513 thresholds, each by
               at least 1e-4 dB: the (max - 80 > thresh) term of nr_rows_kernel decides those bins.  No other
               input has such a bin.
  click        10..90 % of the click profile's dB cells are raised by the noise side's top_db clamp
               (nr_noise_thresh_kernel's fmaxf(db, gm - 80)); the clips the gate was tested with before have none.
  sensitivity  reference against reference: a gate that reads only 1 280 samples around a chunk breaks the new
               bar on the long signal and passes the old rule (99.9 % within 1e-5, all within 2e-2); a gate
               without the top_db clamp breaks the new bar on the floored pair.
"""
import numpy as np
import pytest

import nr_ref as R
from oracle import noisereduce as onr


@pytest.fixture(scope='module')
def clips():
    return R.noise_clips()


@pytest.fixture(scope='module')
def thresh(clips):
    """the reference's own float32 thresholds of every noise clip"""
    return {name: onr.noise_threshold(c) for name, c in clips.items()}


@pytest.fixture(scope='module')
def signals():
    return {**R.signals(), **R.long_signals()}


def test_reduce_on_the_reference_thresholds_is_reduce_noise(clips, thresh, signals):
    for name in ('speech', 'speech[:257]', 'zero-run', 'long1'):
        y, nz = signals[name]
        assert np.array_equal(R.reduce(y, thresh[nz]), onr.reduce_noise(y, 16000, clips[nz])), name


@pytest.mark.parametrize('name', R.THRESH_CLIPS)
def test_thresholds64_is_noise_threshold_in_float64(clips, thresh, name):
    bound, th64 = R.thresh_bound(clips[name])
    d32 = np.abs(thresh[name].astype(np.float64) - th64).max()
    print(f'{name}: d32 {d32:.3e}  bound {bound:.3e}  clamped share {R.clamped_share(clips[name]):.3f}')
    assert th64.shape == (R.NB,) and np.isfinite(th64).all()
    assert d32 <= 1e-4 and d32 <= bound        # float32 dB of magnitude <= 400: a few ulp (2.4e-5 at 400)


def test_muted_profile_rests_on_a_float32_subnormal(clips, thresh):
    """float32 max(1e-40, 0) is the subnormal nearest 1e-40, whose log10 is not -40: -400.00003 on every bin;
    the float64 definition gives -400 exactly"""
    assert (thresh['muted'] == np.float32(-400.00003)).all() and thresh['muted'][0] != np.float32(-400.0)
    assert (R.thresholds64(clips['muted']) == -400.0).all()


def test_decided(thresh, signals):
    for name, (y, nz) in signals.items():
        g = R.gaps(y, thresh[nz])
        print(f'{name}: (cell gap, floor gap) per chunk {g}')
        assert min(min(c) for c in g) >= R.GAP, f'input not decided: {name} {g}'
    assert len(R.gaps(signals['long1'][0], thresh['long'])) == 2


def test_floored(thresh, signals):
    y, nz = signals['floored']
    fb = R.floored_bins(y, thresh[nz])
    n = int((fb > 0).sum())
    print(f'floored pair: {n} of {R.NB} bins with floor > thresh, nearest bin {np.abs(fb).min():.3e} dB')
    assert 64 <= n <= 449 and fb[fb > 0].min() >= 1e-4
    for name in ('tone', 'speech', 'noise', 'zero-run'):        # the inputs the gate was tested on before
        y, nz = signals[name]
        assert not (R.floored_bins(y, thresh[nz]) > 0).any(), name


def test_click(clips):
    share = R.clamped_share(clips['click'])
    print(f'click: {share:.3f} of the dB cells clamped; half-muted {R.clamped_share(clips["half-muted"]):.3f}')
    assert 0.1 <= share <= 0.9
    assert R.clamped_share(clips['half-muted']) > 0.1
    for name in ('base', 'long'):                  # the clips the gate was tested with before: no cell
        assert R.clamped_share(clips[name]) == 0.0, name


def test_sensitivity_seam_context(thresh, signals):
    y, nz = signals['long']
    want = R.reduce(y, thresh[nz])
    got = R.reduce(y, thresh[nz], context=1280)
    err = R.rel_err(got, want)
    print(f'context 1280: {int((err > R.BAR).sum())} samples over the bar, max {err.max():.3e}')
    assert err.max() > R.BAR                   # the new bar sees it
    assert R.old_rule(got, want)               # the old rule did not: the gap the new bar closes


def test_sensitivity_top_db(thresh, signals):
    y, nz = signals['floored']
    want = R.reduce(y, thresh[nz])
    got = R.reduce(y, thresh[nz], top_db=False)
    err = R.rel_err(got, want)
    print(f'top_db off: {int((err > R.BAR).sum())} samples over the bar, max {err.max():.3e}')
    assert err.max() > R.BAR
    y, nz = signals['speech']                  # ... and only there: no floored bin, nothing changes
    assert np.array_equal(R.reduce(y, thresh[nz]), R.reduce(y, thresh[nz], top_db=False))
