"""numpy restatement of the streaming capture conversion (mmla_capture_convert; include/mmla.h) -- TEST
INFRASTRUCTURE ONLY.

A capture format is (rate, channels, channel): channel k >= 0 picks channel k of every interleaved frame,
MEAN (-1, stereo only) is audioop.tomono(data, 2, 0.5, 0.5).  The mono signal then goes through
audioop.ratecv(fragment, 2, 1, rate, 16000, state) with the state (d, prev) carried per stream.  Both the
sequential loop of CPython's audioop (``ratecv_loop``) and the closed form the kernels evaluate
(``ratecv_closed``) are here; tests/test_capture_ref_cpu.py pins both against stdlib audioop.
"""
from math import gcd

import numpy as np

MEAN = -1
OUT_RATE = 16000


def reduced(rate):
    """(ir, or): the capture rate and 16000 over their gcd"""
    g = gcd(int(rate), OUT_RATE)
    return int(rate) // g, OUT_RATE // g


def fresh(rate):
    return -reduced(rate)[1], 0


def mono(frames, channels, channel):
    """interleaved int16 [n * channels] -> the mono int16 [n] the converter reads"""
    x = np.asarray(frames, np.int16).reshape(-1, channels)
    if channel >= 0:
        return x[:, channel].copy()
    assert channels == 2
    v = 0.5 * x[:, 0].astype(np.float64) + 0.5 * x[:, 1].astype(np.float64)
    return np.floor(v).astype(np.int16)


def out_clip_len(clip_frames, rate):
    ir, orr = reduced(rate)
    return (clip_frames * orr - 1) // ir + 1


def _sample(p, c, d, orr):
    """audioop's interpolation of two samples already shifted to 32 bits, phase d in [0, or)"""
    v = (float(p) * float(d) + float(c) * float(orr - d)) / float(orr)
    return int(v) >> 16          # the C cast truncates, the shift floors


def ratecv_loop(x, rate, state):
    """CPython's audioop.ratecv loop on mono int16 x with state (d, prev) -> (int16 out, new state)"""
    ir, orr = reduced(rate)
    d, prev = state
    prev_i = prev * 65536
    cur_i = prev_i
    out = []
    k = 0
    n = len(x)
    while True:
        while d < 0:
            if k == n:
                return np.array(out, np.int16), (d, cur_i >> 16 if n else prev)
            prev_i = cur_i
            cur_i = int(x[k]) * 65536
            k += 1
            d += orr
        while d >= 0:
            out.append(_sample(prev_i, cur_i, d, orr))
            d -= ir


def ratecv_closed(x, rate, state):
    """the closed form: every output from (j, d0, prev) alone -> (int16 out, new state)"""
    ir, orr = reduced(rate)
    d0, prev = state
    n = len(x)
    t = n * orr + d0
    m = t // ir + 1 if t >= 0 else 0
    out = np.zeros(m, np.int16)
    for j in range(m):
        k = -((-(j * ir - d0)) // orr) - 1          # ceil((j ir - d0) / or) - 1
        assert 0 <= k <= n - 1
        d = d0 + (k + 1) * orr - j * ir
        assert 0 <= d < orr
        p = (int(x[k - 1]) if k > 0 else prev) * 65536
        out[j] = _sample(p, int(x[k]) * 65536, d, orr)
    return out, (d0 + n * orr - m * ir, int(x[n - 1]) if n > 0 else prev)


def ratecv_fast(x, rate, state):
    """ratecv_closed vectorised (the GPU tests' inputs are 122 880 frames per clip)"""
    ir, orr = reduced(rate)
    d0, prev = state
    x = np.asarray(x, np.int16)
    n = len(x)
    t = n * orr + d0
    m = t // ir + 1 if t >= 0 else 0
    if m == 0:
        return np.zeros(0, np.int16), (t, int(x[n - 1]) if n > 0 else prev)
    j = np.arange(m, dtype=np.int64)
    k = -((-(j * ir - d0)) // orr) - 1
    d = d0 + (k + 1) * orr - j * ir
    xp = np.concatenate([[prev], x.astype(np.int64)])
    p = (xp[k] * 65536).astype(np.float64)
    c = (xp[k + 1] * 65536).astype(np.float64)
    v = (p * d.astype(np.float64) + c * (orr - d).astype(np.float64)) / float(orr)
    out = (np.trunc(v).astype(np.int64) >> 16).astype(np.int16)
    return out, (t - m * ir, int(x[n - 1]))


class Converter:
    """the converters of a room: n_streams states in one format"""

    def __init__(self, n_streams, rate, channels=1, channel=0):
        self.rate, self.channels, self.channel = int(rate), int(channels), int(channel)
        self.states = [fresh(rate) for _ in range(n_streams)]

    def state_arrays(self):
        return (np.array([s[0] for s in self.states], np.int32),
                np.array([s[1] for s in self.states], np.int32))

    def convert(self, pcm, frames=None, items_per_stream=1, fn=ratecv_fast):
        """interleaved int16 [n, >= clip_frames * channels] with frames[c] valid frames -> (out int16
        [n, out_clip_len] with zeros behind out_lens, out_lens int32 [n]); the states advance"""
        pcm = np.asarray(pcm, np.int16)
        n = pcm.shape[0]
        clip_frames = pcm.shape[1] // self.channels
        frames = np.full(n, clip_frames, np.int32) if frames is None else np.asarray(frames, np.int32)
        ocl = out_clip_len(clip_frames, self.rate)
        out = np.zeros((n, ocl), np.int16)
        lens = np.zeros(n, np.int32)
        for c in range(n):
            s = c // items_per_stream
            x = mono(pcm[c, :frames[c] * self.channels], self.channels, self.channel)
            y, self.states[s] = fn(x, self.rate, self.states[s])
            out[c, :len(y)] = y
            lens[c] = len(y)
        return out, lens
