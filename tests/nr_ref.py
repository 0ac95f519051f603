"""Stationary noise-gate reference with the thresholds supplied -- TEST INFRASTRUCTURE ONLY, never product code.

Built on ``oracle/noisereduce.py`` (the restatement of noisereduce 2.0.x ``SpectralGateStationary``).  The gate
is a threshold decision per (bin, frame): ``dB > thresh``.  The device computes the noise thresholds in
float32 with another summation order than numpy, so the last bit of a threshold may differ, and a gate
compared against the reference's *own* thresholds may flip a cell that sits between the two.  Here the two
halves are held to a reference separately:

  thresholds  ``thresholds64`` is ``noise_threshold`` with every step in float64 on the float32 samples; the
              device's thresholds (``Context.debug_nr_thresh``) are held to it by the d32 rule, d32 being the
              float32 restatement's own distance from the float64 one;
  gate        ``reduce(y, thresh)`` is ``reduce_noise`` on the thresholds the device holds.  With the same
              thresholds on both sides every decision is the same as long as no cell lies within float64
              rounding of its threshold, which ``gaps`` measures; the outputs then differ by float64 rounding
              and the one float32 cast.

The named inputs at the end are shared by tests/test_nr_ref_cpu.py (which asserts the conditions the GPU
tests rest on) and the GPU tests.
"""
import numpy as np
from scipy.signal import fftconvolve

from oracle import noisereduce as onr
from oracle import synth

N_FFT, HOP, CHUNK, PADDING, NB = onr.N_FFT, onr.HOP, onr.CHUNK, onr.PADDING, onr.N_FFT // 2 + 1
SR = 16000
AMIN2 = 1e-40            # amplitude_to_db's amin ** 2
TOP_DB = 80.0

# two float64 evaluations of one dB value (numpy's FFT / the kernel's, |X|^2 / re^2 + im^2) agree to ~1e-12 dB;
# a cell at least GAP from its threshold is decided the same way by both
GAP = 1e-9
# |got - want| <= BAR x max|want| at every sample: 16 x 2^-24 for the one float32 cast of the output
BAR = 1e-6


# ---- thresholds --------------------------------------------------------------------------------------------

def noise_db64(noise):
    """dB cells [513, frames] of the noise clip before the top_db clamp, in float64 on the float32 samples"""
    yn = np.asarray(noise, dtype=np.float32)[:CHUNK].astype(np.float64)
    power = np.square(np.abs(onr.stft(yn, N_FFT, HOP)))
    return 10.0 * np.log10(np.maximum(AMIN2, power))


def thresholds64(noise):
    """oracle noise_threshold (mean + 1.5 std over frames of the clamped dB) in float64 -> float64 [513]"""
    db = noise_db64(noise)
    db = np.maximum(db, db.max() - TOP_DB)
    return np.mean(db, axis=1) + np.std(db, axis=1) * onr.N_STD


def clamped_share(noise):
    """share of the noise clip's dB cells that the top_db clamp raises"""
    db = noise_db64(noise)
    return float(np.mean(db < db.max() - TOP_DB))


def thresh_bound(noise, factor=16.0):
    """the d32 rule's bound on |device threshold - thresholds64| -> (bound, th64)"""
    th64 = thresholds64(noise)
    d32 = float(np.abs(onr.noise_threshold(noise).astype(np.float64) - th64).max())
    return factor * max(d32, 2.0 ** -24 * float(np.abs(th64).max())), th64


# ---- the gate on supplied thresholds -----------------------------------------------------------------------

def buffers(y, context=PADDING):
    """the float64 buffers SpectralGate._read_chunk builds for a mono signal: (start, end, buffer).  Every
    buffer has PADDING samples on both sides of its chunk; `context` (<= PADDING) of them are read from the
    signal, the rest are zeros (PADDING: the library; less: a gate that reads too little around a seam)."""
    y = np.asarray(y)
    n = len(y)
    spans = [(0, n)] if n <= CHUNK else [(i * CHUNK, (i + 1) * CHUNK) for i in range(int((n - 1) / CHUNK) + 1)]
    for start, end in spans:
        i1, i2 = start - PADDING, end + PADDING
        buf = np.zeros(i2 - i1)
        a, b = max(start - context, 0), min(end + context, n)
        buf[a - i1:b - i1] = y[a:b]
        yield start, end, buf


def _gate_chunk_unclamped(chunk, thresh):
    """oracle gate_chunk without amplitude_to_db's top_db clamp (the sensitivity check only)"""
    S = onr.stft(chunk, N_FFT, HOP)
    db = 10.0 * np.log10(np.maximum(AMIN2, np.square(np.abs(S))))
    mask = (db > thresh[:, None]) * 1.0
    mask = fftconvolve(mask, onr.smoothing_filter(*onr.grads(SR, N_FFT, HOP)), mode='same')
    y = onr.istft(S * mask, N_FFT, HOP)
    out = np.zeros(chunk.shape)
    out[:len(y)] = y
    return out


def reduce(y, thresh, context=PADDING, top_db=True):
    """oracle reduce_noise(y, 16000, .) with the per-bin thresholds [513] supplied: the same chunking and
    gate_chunk.  context / top_db are for the sensitivity checks: how much real signal surrounds a chunk,
    and whether the signal's dB are clamped at max - 80."""
    y = np.asarray(y)
    thresh = np.asarray(thresh)
    assert thresh.shape == (NB,), thresh.shape
    n = len(y)
    out = np.zeros(n)
    for start, end, buf in buffers(y, context):
        g = onr.gate_chunk(buf, thresh, SR, N_FFT, HOP) if top_db else _gate_chunk_unclamped(buf, thresh)
        e = min(end, n)
        out[start:e] = g[PADDING:PADDING + (end - start)][:e - start]
    return out.astype(y.dtype)


def chunk_db(buf):
    """(dB cells [513, T] after the top_db clamp, the clamp's floor) of one float64 buffer"""
    db = 10.0 * np.log10(np.maximum(AMIN2, np.square(np.abs(onr.stft(buf, N_FFT, HOP)))))
    floor = db.max() - TOP_DB
    return np.maximum(db, floor), floor


def gaps(y, thresh):
    """per chunk buffer (cell_gap, floor_gap): the smallest |dB - thresh| over all T x 513 cells after the
    top_db floor, and the smallest |floor - thresh| over the bins.  Both far above float64 rounding: every
    decision of the gate is the same in any float64 evaluation."""
    th = np.asarray(thresh, dtype=np.float64)
    out = []
    for _, _, buf in buffers(y):
        db, floor = chunk_db(buf)
        out.append((float(np.abs(db - th[:, None]).min()), float(np.abs(floor - th).min())))
    return out


def min_gap(y, thresh):
    return min(min(g) for g in gaps(y, thresh))


def floored_bins(y, thresh):
    """floor - thresh [513] of the signal's (only) buffer: > 0 where the top_db floor alone sets the mask"""
    (_, _, buf), = buffers(y)
    return chunk_db(buf)[1] - np.asarray(thresh, dtype=np.float64)


def rel_err(got, want):
    """|got - want| / max|want| per sample, float64"""
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / np.abs(want).max()


def check_gate(got, y, thresh, what, want=None):
    """the gate's bar for one signal: `thresh` are the thresholds the device holds for it (float32 [513]);
    `want` = reduce(y, thresh) when the caller has it already.  -> the maximum error (printed first)"""
    g = min_gap(y, thresh)
    assert g >= GAP, f'input not decided: {what}: a cell {g:.3e} dB from its threshold; change the seed'
    if want is None:
        want = reduce(y, thresh)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    peak = np.abs(want).max()
    if peak == 0.0:                                   # digital silence stays bit-equal
        print(f'{what}: want is all zeros')
        assert np.array_equal(got, want), what
        return 0.0
    err = float(rel_err(got, want).max())
    print(f'{what}: max |got - want| / max |want| = {err:.3e}  (smallest gap {g:.3e} dB)')
    assert np.isfinite(got).all() and err <= BAR, (what, err)
    return err


def old_rule(got, want):
    """the rule the gate's tests used before: all but one sample in a thousand within 1e-5 of the peak, all
    within 2e-2.  No test asserts it of the gate any more; the sensitivity check shows what it let through."""
    err = np.abs(np.asarray(got, np.float64) - want) / (np.abs(want).max() + 1e-12)
    return bool(np.quantile(err, 1.0 - 1e-3) <= 1e-5 and err.max() <= 2e-2)


# ---- named inputs, fixed seeds -----------------------------------------------------------------------------

PREFIXES = (1, 10, 255, 256, 257, 700, 1025, 5000)
SHORT_NOISE = (2, 300, 513, 1025, 12345)
LONG = 620000
LONG1 = CHUNK + 1         # the second chunk keeps one sample


def _base():
    rng = np.random.default_rng(5)
    noise = (0.01 * rng.standard_normal(48000)).astype(np.float32)
    t = np.arange(40000) / 16000
    tone = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.01 * rng.standard_normal(40000)).astype(np.float32)
    speech = (synth.clip(91, 40000).astype(np.float32) / 32768.0).astype(np.float32)
    pure = (0.01 * rng.standard_normal(40000)).astype(np.float32)
    return noise, tone, speech, pure


def _long():
    rng = np.random.default_rng(6)
    noise = (0.02 * rng.standard_normal(20000)).astype(np.float32)
    y = np.concatenate([synth.clip(100 + k, 40000) for k in range(16)]).astype(np.float32) / 32768
    return noise, (y[:LONG] + 0.02 * rng.standard_normal(LONG)).astype(np.float32)


def noise_clips():
    """name -> float32 noise clip.  'base' and 'long' are the clips the gate cases always used; 'floored' is
    so quiet against its signal that the signal's top_db floor lies above about half of its thresholds;
    'click', 'half-muted' and 'muted' put the noise side's top_db clamp to work."""
    base = _base()[0]
    out = {'base': base, 'long': _long()[0]}
    out['white'] = (0.01 * np.random.default_rng(8).standard_normal(16000)).astype(np.float32)
    for m in SHORT_NOISE:
        out[f'white[:{m}]'] = out['white'][:m].copy()
    out['floored'] = np.convolve(1.5e-4 * np.random.default_rng(7).standard_normal(16000),
                                 [1.0, 0.9])[:16000].astype(np.float32)
    # one loud sample on a frame centre over noise 104 dB below it: the click's four frames set the maximum,
    # and max - 80 dB falls inside the spread of the quiet frames' cells
    click = (1e-6 * np.random.default_rng(9).standard_normal(16000)).astype(np.float32)
    click[8192] = 0.16
    out['click'] = click
    half = out['white'].copy()
    half[:6000] = 0.0
    out['half-muted'] = half
    out['muted'] = np.zeros(16000, np.float32)
    return out


THRESH_CLIPS = ('white',) + tuple(f'white[:{m}]' for m in SHORT_NOISE) + ('click', 'half-muted', 'muted',
                                                                          'floored', 'base', 'long')


def floored_signal():
    y = synth.clip(91, 40000).astype(np.float64)
    return (0.9 * y / np.abs(y).max()).astype(np.float32)


def zero_run_signal():
    y = _base()[2].copy()
    y[9000:13800] = 0.0
    y[30000:31100] = 0.0
    return y


def signals():
    """name -> (float32 signal, the name of its noise clip): every 40 000-sample and shorter gate input"""
    _, tone, speech, pure = _base()
    out = {'tone': (tone, 'base'), 'speech': (speech, 'base'), 'noise': (pure, 'base')}
    for n in PREFIXES:
        out[f'speech[:{n}]'] = (speech[:n].copy(), 'base')
    out['zero-run'] = (zero_run_signal(), 'base')
    out['silence'] = (np.zeros(40000, np.float32), 'base')
    fl = floored_signal()
    out['floored'] = (fl, 'floored')
    # floored bins meet all-zero windows: the windows' own bits are 0, the floor sets their mask to 1
    holes = fl.copy()
    holes[9000:13800] = 0.0
    holes[30000:31100] = 0.0
    out['floored zero-run'] = (holes, 'floored')
    out['floored[:700]'] = (fl[:700].copy(), 'floored')
    return out


def long_signals():
    """name -> (float32 signal, 'long'): two chunks each, the second keeping 20 000 samples and one sample"""
    y = _long()[1]
    return {'long': (y, 'long'), 'long1': (y[:LONG1].copy(), 'long')}
