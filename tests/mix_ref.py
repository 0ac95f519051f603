"""numpy restatement of the layered mix (mmla_od_mix) and of the pydub arithmetic around it.

The sums are pinned against CPython's audioop.add (tests/test_mix_ref_cpu.py).  pydub itself is not
installed: its slicing arithmetic (len(), frame_count(ms), _parse_position, __getitem__, overlay) is
restated here from its published source, independently of mmla_audio_amd/audio_segment.py, and parity
with the library is unpinned.
"""
import numpy as np

MAX_LAYERS = 8


def chain(canvas, layers):
    """pydub's overlay chain with times = 1 and no gain on int16 samples: for every (src, pos) in order
    canvas[pos : pos + n] = clamp(canvas[pos : pos + n] + src[:n]), n = min(len(src), max(0, len(canvas) -
    pos)).  Each step saturates, so the order matters."""
    v = np.asarray(canvas, np.int16).astype(np.int32)
    for src, pos in layers:
        src = np.asarray(src, np.int16)
        n = min(len(src), max(0, len(v) - pos))
        v[pos:pos + n] = np.clip(v[pos:pos + n] + src[:n].astype(np.int32), -32768, 32767)
    return v.astype(np.int16)


def clipped_sum(canvas, layers):
    """clip(sum of all layers): what the chain is NOT once an intermediate sum saturates"""
    tot = np.asarray(canvas, np.int16).astype(np.int64)
    for src, pos in layers:
        n = min(len(src), max(0, len(tot) - pos))
        tot[pos:pos + n] += np.asarray(src[:n], np.int64)
    return tot, np.clip(tot, -32768, 32767).astype(np.int16)


def audioop_chain(canvas, layers):
    """the same chain as pydub runs it, on bytes through CPython's audioop.add:
    seg1[:pos] + audioop.add(seg1[pos : pos + n], seg2[:n], 2) + the rest"""
    import audioop
    data = np.asarray(canvas, '<i2').tobytes()
    for src, pos in layers:
        head, tail = data[:2 * pos], data[2 * pos:]
        s2 = np.asarray(src, '<i2').tobytes()[:len(tail)]
        data = head + audioop.add(tail[:len(s2)], s2, 2) + tail[len(s2):]
    return np.frombuffer(data, '<i2').astype(np.int16)


def mix(pool, plan, clip_len, chain=chain):
    """mmla_od_mix's rule for a valid plan (n_layers, src_off, src_len, pos) -> (int16 [n, clip_len],
    out_len int32 [n]); chain: the numpy chain, or audioop_chain"""
    pool = np.asarray(pool, np.int16)
    n_layers, src_off, src_len, pos = [np.asarray(a) for a in plan]
    n = len(n_layers)
    out = np.zeros((n, clip_len), np.int16)
    out_len = np.zeros(n, np.int32)
    for c in range(n):
        cl = min(int(src_len[c, 0]), clip_len)
        o = int(src_off[c, 0])
        layers = [(pool[int(src_off[c, l]):int(src_off[c, l]) + int(src_len[c, l])], int(pos[c, l]))
                  for l in range(1, int(n_layers[c]))]
        out[c, :cl] = chain(pool[o:o + cl], layers)
        out_len[c] = cl
    return out, out_len


# ---- pydub's millisecond arithmetic ---------------------------------------------------------------

def ms_len(frames, rate):
    """len(seg) = round(1000 * (frame_count() / frame_rate))"""
    return round(1000 * (float(frames) / rate))


def parse_position(ms, rate):
    """int(frame_count(ms=ms)) = int(ms * (frame_rate / 1000.0))"""
    return int(ms * (rate / 1000.0))


def canvas_frames(F, rate=16000):
    """generate_overlap_segment's canvas = canvas[:time_durations * 1000] of an utterance of F frames ->
    (time_durations, frames of the canvas, the argument of randrange)"""
    dur = F / rate
    td = 1.5 if dur > 1.5 else dur
    end = min(td * 1000, ms_len(F, rate))
    return td, parse_position(end, rate), int(td * 10) - 2


def whole_ms(canvas, rate):
    """overlay returns seg1[:position] + mixed seg1[position:], two millisecond slices: together
    int(len() * rate / 1000) frames -- the canvas cut, or filled up with silence (at most 2 ms, which
    rounding to a millisecond never exceeds), to a whole number of milliseconds"""
    canvas = np.asarray(canvas, np.int16)
    frames = parse_position(ms_len(len(canvas), rate), rate)
    if len(canvas) == 0:
        return canvas
    assert frames - len(canvas) <= 2 * (rate / 1000.0)
    out = np.zeros(frames, np.int16)
    m = min(frames, len(canvas))
    out[:m] = canvas[:m]
    return out


def overlay(canvas, seg, position_ms, rate, times=1):
    """AudioSegment.overlay(seg, position, times=times) on mono int16 at one rate (times < 0: loop)"""
    v = whole_ms(canvas, rate)
    p = parse_position(min(position_ms, ms_len(len(canvas), rate)), rate)
    layers = []
    while times and len(seg) and p < len(v):
        layers.append((seg, p))
        p += len(seg)
        times -= 1
    return chain(v, layers)


def overlap_segment(utterances, draws_ms, rate=16000):
    """generate_overlap_segment on decoded utterances with the positions it drew"""
    _, frames, _ = canvas_frames(len(utterances[0]), rate)
    v = np.asarray(utterances[0], np.int16)[:frames]
    for seg, ms in zip(utterances[1:], draws_ms):
        v = overlay(v, seg, ms, rate)
    return v
