"""GPU stationary noise gate (nr.hip) against the oracle restatement of noisereduce 2.0.x
(oracle/noisereduce.py; parity with the real library is unpinned: it is not installed).

Rule: the reference runs on the thresholds the device holds, want = nr_ref.reduce(y, ctx.debug_nr_thresh()[p])
(the thresholds themselves meet their reference in test_gpu_nr_thresh.py).  Every case first asserts that the
input is decided -- every (bin, frame) cell and every bin's top_db floor at least GAP = 1e-9 dB from its
threshold, where two float64 evaluations of a dB value agree to ~1e-12 dB; a failure there reads "input not
decided" and means another seed, never an excuse -- and then
    |got - want| <= 1e-6 x max|want|  at EVERY sample,
the non-stationary gate's bar and derivation: float64 internals on both sides, one float32 cast of the output
(2^-24 of a sample), a factor 16.  Digital silence is bit-equal.  No case excuses any share of its samples.

Cases: the three 40 000-sample signals, prefixes of 1 .. 5 000 samples (255, 256, 257: around one hop), a signal
with runs of zeros after a call that filled the scratch, silence, the 620 000-sample signal and a 600 001-sample
one whose second chunk keeps one sample, the floored pair (249 of 513 bins set by the signal's top_db floor;
with runs of zeros and as a 700-sample prefix too, where all-zero windows get a non-zero mask), a batch mixing
floored and unfloored signals over a two-profile bank, batches against their signals alone.

Each case prints its maximum error.  Measured on an MI355X:
the maximum error is 0 on every case (the float32 outputs are equal, both long signals and the floored cases
included); the device's thresholds leave the smallest gap at 2.1e-5 dB (long), 1.0e-4 .. 4.1e-4 dB on the
40 000-sample signals, 1.6e-2 dB on the floored ones.
"""
import numpy as np
import pytest

import nr_ref as R
from mmla_audio_amd import _lib

pytestmark = pytest.mark.gpu

BANK = ('base', 'long', 'floored')          # the module context's bank: a signal's profile is its clip's index


@pytest.fixture(scope='module')
def clips():
    x = R.noise_clips()
    for a in x.values():
        a.setflags(write=False)
    return x


@pytest.fixture(scope='module')
def signals():
    x = {**R.signals(), **R.long_signals()}
    for y, _ in x.values():
        y.setflags(write=False)
    return x


@pytest.fixture(scope='module')
def ctx(clips):
    c = _lib.Context(0)
    c.nr_set_noise_bank([clips[name] for name in BANK])
    yield c
    c.close()


@pytest.fixture(scope='module')
def thresh(ctx):
    """the thresholds the device holds, by noise clip"""
    th = ctx.debug_nr_thresh()
    th.setflags(write=False)
    return {name: th[p] for p, name in enumerate(BANK)}


@pytest.fixture(scope='module')
def want(signals, thresh):
    """name -> the reference on the device's thresholds, computed on first use and shared read-only"""
    cache = {}

    def get(name):
        if name not in cache:
            y, nz = signals[name]
            cache[name] = R.reduce(y, thresh[nz])
            cache[name].setflags(write=False)
        return cache[name]
    return get


def _check(got, name, signals, thresh, want, held=None):
    """`held`: the thresholds of the context that made `got`, when it is not the module's: the same bits"""
    y, nz = signals[name]
    if held is not None:
        assert held.tobytes() == thresh[nz].tobytes(), f'{name}: the thresholds of {nz} differ between contexts'
    return R.check_gate(got, y, thresh[nz], name, want(name))


def _gate(ctx, name, signals):
    y, nz = signals[name]
    return ctx.nr_reduce_bank(y, BANK.index(nz))


def test_reduce_noise_matches_oracle(clips, signals, thresh, want):
    from mmla_audio_amd import noisereduce as nr
    for name in ('tone', 'speech', 'noise'):
        y, nz = signals[name]
        got = nr.reduce_noise(y=y, sr=16000, y_noise=clips[nz], stationary=True)
        _check(got, name, signals, thresh, want, held=_lib.default_context(0).debug_nr_thresh()[0])


def test_batched_equals_single(ctx, signals, thresh, want):
    names = ('tone', 'speech', 'noise', 'silence', 'zero-run')
    ys = np.stack([signals[n][0] for n in names])
    single = [ctx.nr_reduce_bank(y, 0) for y in ys]
    for n in (1, 3, 5):
        batch = ctx.nr_reduce_bank(ys[:n], 0)
        for i in range(n):
            assert batch[i].tobytes() == single[i].tobytes(), (n, names[i])
    back = ctx.nr_reduce_bank(ys[::-1].copy(), 0)          # a signal's result does not depend on its row
    for i, name in enumerate(names):
        assert back[len(names) - 1 - i].tobytes() == single[i].tobytes(), name
        _check(single[i], name, signals, thresh, want)


def test_long_signal_is_chunked_like_get_traces(ctx, signals, thresh, want):
    _check(_gate(ctx, 'long', signals), 'long', signals, thresh, want)


def test_long_signal_whose_second_chunk_keeps_one_sample(ctx, signals, thresh, want):
    _check(_gate(ctx, 'long1', signals), 'long1', signals, thresh, want)


def test_unsupported_modes_raise():
    from mmla_audio_amd import noisereduce as nr
    y = np.zeros(1000, np.float32)
    with pytest.raises(NotImplementedError):
        nr.reduce_noise(y=y, sr=16000, stationary=False)
    with pytest.raises(NotImplementedError):
        nr.reduce_noise(y=y, sr=16000, stationary=True, prop_decrease=0.5)


@pytest.mark.parametrize('n', R.PREFIXES)
def test_short_signals(ctx, signals, thresh, want, n):
    """Signals shorter than one frame / a few frames: every window reaches the buffer's reflect
    edges' zero padding, and the launched frame range (nr_frame_range) is small."""
    name = f'speech[:{n}]'
    _check(_gate(ctx, name, signals), name, signals, thresh, want)


def test_silent_signal(clips, signals, thresh, want):
    """All-zero input: every frame is the -400 dB floor (the top_db reference of the chunk)."""
    from mmla_audio_amd import noisereduce as nr
    y, nz = signals['silence']
    got = nr.reduce_noise(y=y, sr=16000, y_noise=clips[nz], stationary=True)
    _check(got, 'silence', signals, thresh, want, held=_lib.default_context(0).debug_nr_thresh()[0])
    assert np.array_equal(got, want('silence')) and not want('silence').any()


def test_zero_run_inside_signal_after_other_calls(clips, signals, thresh, want):
    """A run of >= 1024 zero samples inside a voiced signal: its all-zero windows still reach the
    kept interior, so their spectra (0) are read by the gate; the scratch holding the previous
    call's spectra must not leak in (regression: the first call on a fresh context passed)."""
    c = _lib.Context(0)
    try:
        c.nr_set_noise(clips['base'])
        c.nr_reduce(np.stack([signals['tone'][0], signals['speech'][0]]))   # fill the scratch with nonzero spectra
        got = c.nr_reduce(signals['zero-run'][0])
        _check(got, 'zero-run', signals, thresh, want, held=c.debug_nr_thresh()[0])
    finally:
        c.close()


@pytest.mark.parametrize('name', ['floored', 'floored zero-run', 'floored[:700]'])
def test_floored_pair(ctx, signals, thresh, want, name):
    """The signal's top_db floor (its maximum - 80 dB) lies above about half of the quiet clip's thresholds:
    nr_rows_kernel's (gmax - 80 > thresh) sets those bins' mask in every frame, all-zero windows included."""
    y, nz = signals[name]
    fb = R.floored_bins(y, thresh[nz])
    n = int((fb > 0).sum())
    print(f'{name}: {n} of {R.NB} bins floored, the nearest {np.abs(fb).min():.3e} dB from its threshold')
    assert 64 <= n <= 449
    ctx.nr_reduce_bank(np.stack([signals['tone'][0], signals['speech'][0]]), 0)   # nonzero spectra in the scratch
    _check(_gate(ctx, name, signals), name, signals, thresh, want)


def test_mixed_batch_over_a_two_profile_bank(clips, signals, thresh, want):
    """floored and unfloored signals in one launch, each against its own profile"""
    names = ('speech', 'floored', 'zero-run', 'floored zero-run', 'tone')
    bank = ('base', 'floored')
    c = _lib.Context(0)
    try:
        c.nr_set_noise_bank([clips[name] for name in bank])
        held = c.debug_nr_thresh()
        prof = np.array([bank.index(signals[n][1]) for n in names], np.int32)
        ys = np.stack([signals[n][0] for n in names])
        got = c.nr_reduce_bank(ys, prof)
        for i, name in enumerate(names):
            _check(got[i], name, signals, thresh, want, held=held[prof[i]])
            assert got[i].tobytes() == c.nr_reduce_bank(ys[i], int(prof[i])).tobytes(), name
        swapped = c.nr_reduce_bank(ys[:2], np.array([1, 0], np.int32))      # the profile matters
        assert not np.array_equal(swapped[0], got[0]) and not np.array_equal(swapped[1], got[1])
    finally:
        c.close()
