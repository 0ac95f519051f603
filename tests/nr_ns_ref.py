"""Non-stationary noise-gate restatement (numpy / scipy) -- TEST INFRASTRUCTURE ONLY, never product code.

noisereduce 2.0.x ``reduce_noise(y=y, sr=sr)`` in its default mode (``stationary=False``,
``SpectralGateNonStationary``), restated from its published source on the librosa-0.8 ``stft`` /
``istft`` that ``oracle/noisereduce.py`` restates for the stationary gate.  The reference's scripts never
call this mode and neither library is installed here: parity with the library is *unpinned*, this file
is the definition the GPU gate (nr.hip, the nr_ns_* kernels) is held to.

Per chunk buffer (float64, ``padding`` samples of context on both sides, zeros outside the signal):
  S = stft(buffer);  A = |S|
  b = (sqrt(1 + 4 t^2) - 1) / (2 t^2),  t = time_constant_s * sr / hop
  smooth = scipy.signal.filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)
  mask = sigmoid((A - smooth) / smooth, -thresh_n_mult, sigmoid_slope)
  mask = fftconvolve(mask, smoothing_filter, 'same');  y = istft(S * mask)
One deliberate deviation from the library: where smooth == 0 the mask is 0 (the library computes 0 / 0
there and returns NaN for the whole signal).  smooth is 0 only for a buffer of nothing but zeros.
"""
import numpy as np
from scipy.signal import fftconvolve, filtfilt

from oracle import noisereduce as onr

N_FFT, HOP, CHUNK, PADDING = onr.N_FFT, onr.HOP, onr.CHUNK, onr.PADDING


def coefficient(time_constant_s=2.0, sr=16000, hop=HOP):
    """b of get_time_smoothed_representation: the one-pole coefficient of a time constant in frames."""
    t_frames = time_constant_s * sr / hop
    return (np.sqrt(1 + 4 * t_frames ** 2) - 1) / (2 * t_frames ** 2)


def smooth_filtfilt(A, b):
    """the library's call: forward-backward one-pole filter along time, no edge padding"""
    return filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)


def smooth_recurrence(A, b):
    """filtfilt([b], [1, b - 1], A, axis=-1, padtype=None) as the explicit recurrence, per bin, in
    scipy's direct-form-II-transposed operation order (what nr_ns_smooth_kernel walks)."""
    A = np.asarray(A, dtype=np.float64)
    omb = -(b - 1.0)
    T = A.shape[-1]
    f = np.empty_like(A)
    z = omb * A[..., 0]
    for t in range(T):
        f[..., t] = b * A[..., t] + z
        z = omb * f[..., t]
    g = np.empty_like(A)
    z = omb * f[..., T - 1]
    for t in range(T - 1, -1, -1):
        g[..., t] = b * f[..., t] + z
        z = omb * g[..., t]
    return g


def mask_of(A, smooth, thresh_n_mult=2.0, sigmoid_slope=10.0):
    """sigmoid((A - smooth) / smooth, -thresh_n_mult, sigmoid_slope); 0 where smooth == 0"""
    ok = smooth != 0
    x = np.zeros_like(A)
    x[ok] = (A[ok] - smooth[ok]) / smooth[ok]
    mask = 1.0 / (1.0 + np.exp(-(x + -thresh_n_mult) * sigmoid_slope))
    mask[~ok] = 0.0
    return mask


def chunk_smooth(chunk, sr=16000, time_constant_s=2.0):
    """(A, smooth) of one float64 buffer: what the mask is made of"""
    A = np.abs(onr.stft(chunk, N_FFT, HOP))
    return A, smooth_filtfilt(A, coefficient(time_constant_s, sr))


def gate_chunk(chunk, sr, time_constant_s=2.0, thresh_n_mult=2.0, sigmoid_slope=10.0):
    """spectral_gating_nonstationary on one float64 buffer (prop_decrease 1.0)"""
    S = onr.stft(chunk, N_FFT, HOP)
    A = np.abs(S)
    smooth = smooth_filtfilt(A, coefficient(time_constant_s, sr))
    mask = mask_of(A, smooth, thresh_n_mult, sigmoid_slope)
    mask = fftconvolve(mask, onr.smoothing_filter(*onr.grads(sr, N_FFT, HOP)), mode='same')
    y = onr.istft(S * mask, N_FFT, HOP)
    out = np.zeros(chunk.shape)
    out[:len(y)] = y
    return out


def buffers(y, chunk_size=CHUNK, padding=PADDING):
    """the float64 buffers SpectralGate._read_chunk builds for a mono signal: (start, end, buffer)"""
    y = np.asarray(y)
    n = len(y)
    spans = [(0, n)] if n <= chunk_size else [(i * chunk_size, (i + 1) * chunk_size)
                                              for i in range(int((n - 1) / chunk_size) + 1)]
    for start, end in spans:
        i1, i2 = start - padding, end + padding
        buf = np.zeros(i2 - i1)
        a, b = max(i1, 0), min(i2, n)
        buf[a - i1:b - i1] = y[a:b]
        yield start, end, buf


def reduce_noise(y, sr=16000, time_constant_s=2.0, thresh_n_mult=2.0, sigmoid_slope=10.0):
    """reduce_noise(y=y, sr=sr, stationary=False, ...) for a mono y; the dtype is preserved"""
    y = np.asarray(y)
    n = len(y)
    out = np.zeros(n)
    for start, end, buf in buffers(y):
        g = gate_chunk(buf, sr, time_constant_s, thresh_n_mult, sigmoid_slope)
        e = min(end, n)
        out[start:e] = g[PADDING:PADDING + (end - start)][:e - start]
    return out.astype(y.dtype)


# ---- the inputs the CPU and GPU tests share -------------------------------------------------------

def signals():
    """the three 40 000-sample signals of tests/test_gpu_noisereduce.py: tone + noise, speech, noise"""
    from oracle import synth
    rng = np.random.default_rng(5)
    rng.standard_normal(48000)                       # that file's noise clip comes first
    t = np.arange(40000) / 16000
    tone = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.01 * rng.standard_normal(40000)).astype(np.float32)
    speech = (synth.clip(91, 40000).astype(np.float32) / 32768.0).astype(np.float32)
    pure = (0.01 * rng.standard_normal(40000)).astype(np.float32)
    return np.stack([tone, speech, pure])


def long_signal():
    """620 000 samples: two chunks (tests/test_gpu_noisereduce.py's)"""
    from oracle import synth
    rng = np.random.default_rng(6)
    rng.standard_normal(20000)
    y = np.concatenate([synth.clip(100 + k, 40000) for k in range(16)]).astype(np.float32) / 32768
    return (y[:620000] + 0.02 * rng.standard_normal(620000)).astype(np.float32)


def stale_scratch_signals():
    """40 000-sample signals that leave most frames all-zero windows: two that are nonzero only in
    [0, 700), and the speech clip with two runs of zeros inside"""
    ys = signals()
    head = np.zeros((2, 40000), np.float32)
    head[0, :700] = ys[1][:700]
    head[1, :700] = ys[0][:700]
    holes = ys[1].copy()
    holes[9000:13800] = 0.0
    holes[30000:31100] = 0.0
    return np.concatenate([head, holes[None]])


PREFIXES = (1, 10, 700, 1025, 5000)


def named_inputs():
    """every nonzero input of tests/test_gpu_nr_nonstationary.py's parity cases, by name"""
    ys = signals()
    out = {'tone': ys[0], 'speech': ys[1], 'noise': ys[2], 'long': long_signal()}
    for n in PREFIXES:
        out[f'speech[:{n}]'] = ys[1][:n].copy()
    for i, y in enumerate(stale_scratch_signals()):
        out[f'stale{i}'] = y
    return out
