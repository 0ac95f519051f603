"""The capture audio the GPU capture tests tick on (tests/test_gpu_capture.py) and the CPU oracles' verdict
on it (tests/test_capture_inputs_cpu.py) -- TEST INFRASTRUCTURE ONLY.

Two ticks of 6 clips = 3 streams x 2 of tests/cond_ref.py's clips (voiced, gapped, burst, noise, digital
zeros, voiced with a noise tail), brought to a capture format:
  48 kHz stereo  channel 0 holds every 16 kHz sample three times, channel 1 another signal.  audioop's
                 ratecv of a thrice-held signal from a fresh state returns the signal (phase d = 0 at every
                 output), so the restatement's converted clips are cond_ref's clips themselves
  44.1 kHz mono  the clips linearly interpolated to 112 896 frames, with ragged frame counts
"""
import numpy as np

import capture_ref
import cond_ref

STREAMS, IPS = 3, 2
N = STREAMS * IPS
ORDER = ((0, 1, 2, 3, 4, 5), (5, 0, 2, 1, 3, 4))          # the two ticks' clips
FRAMES_48K = 3 * cond_ref.L                                 # 122 880
FRAMES_441 = cond_ref.L * 441 // 160                        # 112 896: 2.56 s
# 44.1 kHz: ragged frame counts; 11 000 frames are 3 991 samples at 16 kHz: below the silent rule's 4 000
RAGGED = np.array([FRAMES_441, 60000, FRAMES_441, 11000, FRAMES_441, 82688], np.int32)


def ticks16k():
    x = cond_ref.clips()
    return [np.ascontiguousarray(x[list(o)]) for o in ORDER]


def capture_48k_stereo(x):
    """int16 [n, L] at 16 kHz -> interleaved [n, 2 * 3 L]: channel 0 = x held x 3, channel 1 = another signal"""
    raw = np.zeros((x.shape[0], 3 * x.shape[1], 2), np.int16)
    raw[:, :, 0] = np.repeat(x, 3, axis=1)
    raw[:, :, 1] = -(raw[:, ::-1, 0] // 2) + 5
    return np.ascontiguousarray(raw.reshape(x.shape[0], -1))


def capture_441_mono(x):
    """int16 [n, L] at 16 kHz -> [n, 112 896] at 44.1 kHz by linear interpolation"""
    t = np.arange(FRAMES_441) * (160.0 / 441.0)
    src = np.arange(x.shape[1], dtype=np.float64)
    return np.stack([np.round(np.interp(t, src, c.astype(np.float64))).astype(np.int16) for c in x])


CASES = {
    # name: (format (rate, channels, channel), builder, frames per tick or None)
    '48k_stereo': ((48000, 2, 0), capture_48k_stereo, None),
    '441_mono': ((44100, 1, 0), capture_441_mono, RAGGED),
}


def capture_ticks(case):
    """-> (format, [raw capture of tick 0, tick 1], frames or None)"""
    fmt, build, frames = CASES[case]
    return fmt, [build(x) for x in ticks16k()], frames


def restated(case):
    """the restatement's conversion of the two ticks with the state carried: -> ([(clips16k, out_lens)] per
    tick, the Converter after tick 2)"""
    fmt, raws, frames = capture_ticks(case)
    conv = capture_ref.Converter(STREAMS, *fmt)
    return [conv.convert(r, frames, IPS) for r in raws], conv


def detectors():
    from oracle import webrtc_vad
    return [webrtc_vad.Vad(3) for _ in range(STREAMS)]


def oracle_kept(q, lens, profiles, dets, ips=IPS):
    """kept lengths of one tick's converted clips by the CPU oracles: one gate pass against noise profile
    profiles[c] (None: no gate), PCM_16, then the stream's own webrtc Vad(3) (dets, carried from tick to
    tick) over its clips in order"""
    from oracle import noisereduce as onr
    from oracle import vad as ovad
    import ssim_ref
    kept = []
    for c, clip in enumerate(q):
        det = dets[c // ips]
        y = clip.copy()
        y[lens[c]:] = 0
        if profiles is not None:
            f = (y.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
            y = ssim_ref.pcm16(onr.reduce_noise(f, 16000, cond_ref.noise(profiles[c])))
            y[lens[c]:] = 0
        kept.append(len(ovad.remove_silence(y[:lens[c]], det.is_speech)[0]))
    return np.array(kept)
