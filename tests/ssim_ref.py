"""Float64 restatement of ``skimage.metrics.structural_similarity`` for uint8 images -- TEST
INFRASTRUCTURE ONLY.

Written from scikit-image's published source (``skimage/metrics/_structural_similarity.py``, 0.19) with
the same ``scipy.ndimage.uniform_filter`` calls it makes, for the defaults the reference's call
``structural_similarity(image1, image2, multichannel=True)`` (record_on_pi.py:44) takes on uint8
input: win_size 7, uniform window, K1 0.01, K2 0.03, data_range 255, sample covariance.  scikit-image
itself is not installed here, so parity with the real library is unpinned.

Also the recipe of the clips the silence-gate tests share (``gate_clips``) and the CPU oracle of the
whole gate (``oracle_gate``).
"""
import numpy as np
from scipy.ndimage import uniform_filter

WIN = 7
K1, K2, R = 0.01, 0.03, 255.0
C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2


def _ssim_2d(x, y):
    """one channel [h, w] -> mean SSIM (float64)"""
    x = x.astype(np.float64)
    y = y.astype(np.float64)
    NP = WIN ** x.ndim
    cov_norm = NP / (NP - 1)          # sample covariance
    ux = uniform_filter(x, size=WIN)
    uy = uniform_filter(y, size=WIN)
    uxx = uniform_filter(x * x, size=WIN)
    uyy = uniform_filter(y * y, size=WIN)
    uxy = uniform_filter(x * y, size=WIN)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
    B1, B2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (WIN - 1) // 2               # crop(S, pad): the filter's border mode never enters
    return S[pad:-pad, pad:-pad].mean(dtype=np.float64)


def ssim(a, b):
    """structural_similarity(a, b) for uint8 [h, w], or (multichannel=True) [h, w, c]: the mean over
    channels of the per-channel mean."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape
    if a.ndim == 2:
        return _ssim_2d(a, b)
    return np.mean([_ssim_2d(a[..., k], b[..., k]) for k in range(a.shape[2])], dtype=np.float64)


def ssim_brute(a, b):
    """the definition with plain loops over window positions (slow; small images only)"""
    a = np.asarray(a, np.float64).reshape(a.shape[0], a.shape[1], -1)
    b = np.asarray(b, np.float64).reshape(a.shape)
    h, w, c = a.shape
    per = []
    for k in range(c):
        vals = []
        for i in range(h - WIN + 1):
            for j in range(w - WIN + 1):
                x = a[i:i + WIN, j:j + WIN, k].ravel()
                y = b[i:i + WIN, j:j + WIN, k].ravel()
                ux, uy = x.mean(), y.mean()
                vx, vy = x.var(ddof=1), y.var(ddof=1)
                vxy = ((x - ux) * (y - uy)).sum() / (x.size - 1)
                vals.append(((2 * ux * uy + C1) * (2 * vxy + C2)) /
                            ((ux * ux + uy * uy + C1) * (vx + vy + C2)))
        per.append(np.mean(vals))
    return float(np.mean(per))


def ssim_integer_form(a, b):
    """the kernel's form (csrc/ssim.hip): exact integer 7 x 7 sums, then
    S = (2 sx sy + 49^2 C1)(2 (49 sxy - sx sy) + 49 48 C2) /
        ((sx^2 + sy^2 + 49^2 C1)((49 sxx - sx^2) + (49 syy - sy^2) + 49 48 C2)), in float64"""
    a = np.asarray(a, np.int64).reshape(a.shape[0], a.shape[1], -1)
    b = np.asarray(b, np.int64).reshape(a.shape)

    def box(v):
        cs = np.cumsum(np.cumsum(np.pad(v, ((1, 0), (1, 0), (0, 0))), axis=0), axis=1)
        return cs[WIN:, WIN:] - cs[:-WIN, WIN:] - cs[WIN:, :-WIN] + cs[:-WIN, :-WIN]

    NP = WIN * WIN
    sx, sy, sxx, syy, sxy = box(a), box(b), box(a * a), box(b * b), box(a * b)
    parts = (2 * sx * sy, sx * sx + sy * sy, 2 * (NP * sxy - sx * sy),
             (NP * sxx - sx * sx) + (NP * syy - sy * sy))
    assert max(int(np.abs(p).max()) for p in parts) <= 312250050   # int32 is enough
    A1 = parts[0] + NP * NP * C1
    B1 = parts[1] + NP * NP * C1
    A2 = parts[2] + NP * (NP - 1) * C2
    B2 = parts[3] + NP * (NP - 1) * C2
    S = (A1 * A2) / (B1 * B2)
    return float(S.mean(axis=(0, 1)).mean())


# ---- the clips of the silence-gate tests ------------------------------------------------------------

NOISE_LEVEL = 0.01 / 3.0   # white noise at -40 dBFS / 3 sigma, librosa.load scale
GATE_CLIP = 24000


def gate_noise():
    """the noise profile: 1 s of white noise, float32"""
    rng = np.random.default_rng(4101)
    return (NOISE_LEVEL * rng.standard_normal(16000)).astype(np.float32)


def gate_clips():
    """int16 [12, 24000]: oracle.synth.clip(i, 24000), i = 0..10, the voiced classes (i % 5 in {0, 1})
    halved and mixed with fresh noise of the profile's level; clip 11 is fresh noise alone"""
    from oracle import synth
    rng = np.random.default_rng(4102)
    out = np.zeros((12, GATE_CLIP), np.int16)
    for i in range(11):
        x = synth.clip(i, GATE_CLIP).astype(np.float64)
        if i % 5 in (0, 1):
            x = x / 2 + 32767.0 * NOISE_LEVEL * rng.standard_normal(GATE_CLIP)
        out[i] = np.clip(np.round(x), -32768, 32767).astype(np.int16)
    out[11] = np.round(32767.0 * NOISE_LEVEL * rng.standard_normal(GATE_CLIP)).astype(np.int16)
    return out


def pcm16(y):
    """soundfile's PCM_16 write of float32 audio (libsndfile: lrintf(y * 0x7FFF) into a short)"""
    return np.rint(np.float32(32767.0) * np.asarray(y, np.float32)).astype(np.int32).astype(np.int16)


def oracle_gate(pcm, noise, passes=4, length=None):
    """the gate of record_on_pi.py:103-124 on one int16 clip with the CPU oracles: -> (ssim of the raw
    clip's image against the `passes` x denoised clip's image, the denoised int16 clip).  `length`: the
    clip's true length (the clip is zero past it and stays so after every pass)."""
    from oracle import noisereduce as onr
    from oracle import od_fe
    pcm = np.asarray(pcm, np.int16)
    q = pcm.copy()
    for _ in range(passes):
        y = (q.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        q = pcm16(onr.reduce_noise(y, 16000, noise))
        if length is not None:
            q[length:] = 0
    a = od_fe.od_features(pcm if length is None else pcm[:length])['png_rgb']
    b = od_fe.od_features(q if length is None else q[:length])['png_rgb']
    return ssim(a, b), q
