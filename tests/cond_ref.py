"""The inputs the conditioning tests share (mmla_condition, mmla_{od,si}_pipeline_conditioned) and the
composition of the public calls the fused calls must equal -- TEST INFRASTRUCTURE ONLY.

Three noise profiles (microphones) of rising level and six clips of the PC loop's 2.56 s: the levels are
such that, per profile, the batched save_wave_file keeps one clip nearly whole, shortens one and empties
one, and the three profiles keep different lengths (tests/test_conditioning_inputs_cpu.py asserts it
with the CPU oracles).
"""
import numpy as np

import ssim_ref

L = 40960                      # record_on_pc.py: 2.56 s at 16 kHz
LV = ssim_ref.NOISE_LEVEL
N_PROFILES = 3

# kept lengths of the six clips: one oracle gate pass against profile p (None: no gate), ssim_ref.pcm16,
# one webrtc_vad.Vad(3) carried over the six clips in order (a record: see the CPU test)
KEPT = {
    0: (40800, 26400, 10080, 0, 0, 30720),
    1: (40800, 24960, 9600, 0, 0, 30720),
    2: (14880, 21120, 0, 0, 0, 23040),
    None: (40800, 26880, 10080, 0, 0, 30720),
}


def noise(p):
    """noise profile p in {0, 1, 2}: 1 s of white noise of level 4**p * LV, float32"""
    return (4 ** p * LV * np.random.default_rng(5200 + p).standard_normal(16000)).astype(np.float32)


def clips():
    """int16 [6, L]: voiced, voiced with a noise-only gap, a 0.2 s burst in noise, noise alone,
    digital zeros, voiced with a noise-only tail"""
    from oracle import synth
    rng = np.random.default_rng(5210)

    def nz(n):
        return 32767.0 * LV * rng.standard_normal(n)

    def v(i):
        return synth.clip(i, L).astype(np.float64) / 2

    x = np.zeros((6, L), np.float64)
    x[0] = v(0) + nz(L)
    x[1] = v(1) + nz(L)
    x[1, 8000:28000] = nz(20000)
    x[2] = nz(L)
    x[2, 16000:19200] += v(5)[16000:19200]
    x[3] = nz(L)
    x[5] = v(5) + nz(L)
    x[5, 24000:] = nz(L - 24000)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def oracle_kept(x, p):
    """kept lengths of the clips x by the CPU oracles, gated against profile p (None: no gate)"""
    from oracle import noisereduce as onr
    from oracle import vad as ovad
    from oracle import webrtc_vad
    det = webrtc_vad.Vad(3)
    kept = []
    for c in x:
        q = c
        if p is not None:
            y = (c.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
            q = ssim_ref.pcm16(onr.reduce_noise(y, 16000, noise(p)))
        kept.append(len(ovad.remove_silence(q, det.is_speech)[0]))
    return tuple(kept)


def zero_tails(q, lens):
    if lens is not None:
        for i, m in enumerate(lens):
            q[i, m:] = 0
    return q


def composed_condition(ctx, pcm, noises, profile, lens=None, passes=1, silence_remove=True,
                       items_per_stream=1, reset=True):
    """mmla_condition from the public calls: per profile nr_set_noise + nr_reduce on its clips -> pcm16 ->
    tail zeroing, `passes` times; then vad_remove_silence on (by default freshly reset) detectors.
    -> (int16 [n, L] with zeros behind the kept samples, kept_len [n]).  Leaves the context's noise
    profile replaced."""
    pcm = np.asarray(pcm, np.int16)
    n, width = pcm.shape
    q = zero_tails(pcm.copy(), lens)
    profile = np.zeros(n, np.int32) if profile is None else np.asarray(profile)
    for _ in range(passes):
        y = q.astype(np.float32) / np.float32(32768.0)
        for p in sorted(set(profile.tolist())):
            idx = np.flatnonzero(profile == p)
            ctx.nr_set_noise(noises[p])
            q[idx] = ctx.pcm16(ctx.nr_reduce(y[idx]))
        q = zero_tails(q, lens)
    if not silence_remove:
        kept = np.full(n, width, np.int32) if lens is None else np.asarray(lens, np.int32).copy()
        return q, kept
    if reset:
        ctx.vad_reset(n // items_per_stream, 3)
    voiced, _ = ctx.vad_remove_silence(q, lens=lens, items_per_stream=items_per_stream)
    out = np.zeros_like(q)
    kept = np.zeros(n, np.int32)
    for i, o in enumerate(voiced):
        out[i, :len(o)] = o
        kept[i] = len(o)
    return out, kept
