"""The inputs the enrolment tests share (mmla_si_enrol_embed, Room.register) -- TEST INFRASTRUCTURE ONLY.

Registration recordings are voiced synthetic audio in the style of test_gpu_si_registration._voiced_wav (a
harmonic series under a slow amplitude modulation) with a stretch of low noise inside, so that the silence
removal has something to take out and something to keep (tests/test_enrol_cpu.py asserts both with the CPU
oracles before a GPU run is spent on it)."""
import numpy as np

import cond_ref

SR = 16000
CLIP = 48000                                   # test (a): 3 s recordings, w_max = 2
LENS = np.array([48000, 30000, 0], np.int32)
PROFILE = np.array([1, 0, 1], np.int32)        # two noise profiles of cond_ref
LONG = 610000                                  # test (b): crosses the gate chunk, no multiple of 480


def frames(n):
    """psf's frame count T(n), n >= 1"""
    return 1 if n <= 400 else 1 + -(-(n - 400) // 160)


def windows(n):
    """256-frame windows of n samples (0 for none)"""
    return -(-frames(n) // 256) if n > 0 else 0


def voiced(f0, seed, n, quiet=()):
    """int16 [n]: 20 harmonics of f0 under a 3 Hz amplitude modulation at half scale, plus a noise floor of
    cond_ref's level; inside every (a, b) of `quiet` the noise floor alone"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    k = np.arange(1, 21)[:, None]
    x = np.sum(np.sin(2 * np.pi * k * f0 * t[None] + rng.uniform(0, 2 * np.pi, (20, 1))) / k, axis=0)
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
    x = 0.5 * x / np.abs(x).max()
    for a, b in quiet:
        x[a:b] = 0.0
    x = x + cond_ref.LV * rng.standard_normal(n)
    return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)


def recordings():
    """int16 [3, CLIP] for test (a): two voiced recordings with a quiet second inside, one unused row"""
    x = np.stack([voiced(110.0, 60, CLIP, [(16000, 32000)]),
                  voiced(165.0, 61, CLIP, [(8000, 20000)]),
                  voiced(230.0, 62, CLIP)])
    x.setflags(write=False)
    return x


def noises():
    return [cond_ref.noise(0), cond_ref.noise(1)]


def long_recording():
    """int16 [LONG] for test (b): voiced with quiet stretches, one of them across the gate chunk's end"""
    x = voiced(140.0, 63, LONG, [(100000, 180000), (590000, 605000)])
    x.setflags(write=False)
    return x


def oracle_kept(x, lens, profile, noise_clips):
    """kept lengths by the CPU oracles: one gate pass against the recording's profile, the PCM_16 write,
    silence removal on a fresh webrtc_vad.Vad(3) per recording"""
    import ssim_ref
    from oracle import noisereduce as onr
    from oracle import vad as ovad
    from oracle import webrtc_vad
    kept = []
    for c, m, p in zip(x, lens, profile):
        y = np.zeros(len(c), np.float32)
        y[:m] = c[:m].astype(np.float32) / np.float32(32768.0)
        q = ssim_ref.pcm16(onr.reduce_noise(y, 16000, noise_clips[p]))
        q[m:] = 0
        kept.append(len(ovad.remove_silence(q[:m], webrtc_vad.Vad(3).is_speech)[0]))
    return kept
