"""CPU: the streaming capture conversion's arithmetic (tests/capture_ref.py, the definition the kernels of
mmla_capture_convert implement) pinned against stdlib audioop, fragment by fragment with audioop's own
returned state: samples, counts and the state (d, cur >> 16) after every fragment, for the sequential
loop, the closed form and its vectorised twin.  audioop is part of CPython up to 3.12; skipped without it.
"""
import warnings

import numpy as np
import pytest

import capture_ref as cr

with warnings.catch_warnings():
    warnings.simplefilter('ignore', DeprecationWarning)
    audioop = pytest.importorskip('audioop')

RATES = (48000, 44100, 32000, 22050, 16000, 11025, 8000)
FRAGMENTS = (1, 2, 7, 0, 300, 441, 1000, 3, 5000)
FORMATS = ((1, 0), (2, 0), (2, 1), (2, cr.MEAN))
TOMONO_CORNERS = ((-3, 0), (-1, 0), (32767, 32767), (-32768, -32768), (5, 2), (-5, -2))


def _capture(rng, n, channels):
    x = (rng.standard_normal(n * channels) * 9000).clip(-32768, 32767).astype('<i2')
    edge = np.array([32767, -32768, 32767, -32768, -1, 1, -32768, 32767], '<i2')
    x[:min(len(edge), len(x))] = edge[:len(x)]
    return x


def _audioop_mono(frag, channels, channel):
    if channels == 1:
        return frag
    if channel == cr.MEAN:
        return audioop.tomono(frag, 2, 0.5, 0.5)
    return np.frombuffer(frag, '<i2')[channel::channels].astype('<i2').tobytes()


def test_tomono_corner_values():
    pairs = np.array(TOMONO_CORNERS, '<i2')
    want = np.frombuffer(audioop.tomono(pairs.tobytes(), 2, 0.5, 0.5), '<i2')
    got = cr.mono(pairs.reshape(-1), 2, cr.MEAN)
    assert got.tolist() == want.tolist() == [-2, -1, 32767, -32768, 3, -4]


def test_audio_segment_set_channels_is_tomono():
    from mmla_audio_amd.audio_segment import AudioSegment
    rng = np.random.default_rng(3)
    raw = _capture(rng, 4001, 2)
    raw[8:8 + 2 * len(TOMONO_CORNERS)] = np.array(TOMONO_CORNERS, '<i2').reshape(-1)
    seg = AudioSegment(raw, 48000, 2)
    mono = seg.set_channels(1)
    assert mono.channels == 1 and mono.frame_rate == 48000 and mono.frame_count == 4001
    assert mono.data.tobytes() == audioop.tomono(raw.tobytes(), 2, 0.5, 0.5)
    assert seg.set_channels(2) is seg and mono.set_channels(1) is mono
    with pytest.raises(ValueError):
        mono.set_channels(2)


@pytest.mark.parametrize('channels,channel', FORMATS)
@pytest.mark.parametrize('rate', RATES)
def test_fragments_with_carried_state(rate, channels, channel):
    rng = np.random.default_rng(rate + 10 * channels + channel)
    state = None
    mine = {fn: cr.fresh(rate) for fn in (cr.ratecv_loop, cr.ratecv_closed, cr.ratecv_fast)}
    ir, orr = cr.reduced(rate)
    for n in FRAGMENTS:
        raw = _capture(rng, n, channels)
        if channels == 2 and n >= len(TOMONO_CORNERS):
            raw[:2 * len(TOMONO_CORNERS)] = np.array(TOMONO_CORNERS, '<i2').reshape(-1)
        frag = _audioop_mono(raw.tobytes(), channels, channel)
        x = cr.mono(raw, channels, channel)
        assert x.tobytes() == frag
        data, state = audioop.ratecv(frag, 2, 1, rate, 16000, state)
        want = np.frombuffer(data, '<i2')
        want_state = (state[0], state[1][0][1] >> 16)
        for fn in mine:
            d0 = mine[fn][0]
            got, mine[fn] = fn(x, rate, mine[fn])
            assert got.dtype == np.int16 and len(got) == len(want), (fn.__name__, rate, n)
            assert np.array_equal(got, want), (fn.__name__, rate, n)
            assert mine[fn] == want_state, (fn.__name__, rate, n, mine[fn], want_state)
            assert -max(ir, orr) <= mine[fn][0] < 0
            assert len(got) <= cr.out_clip_len(max(n, 1), rate)
            assert len(got) == ((n * orr + d0) // ir + 1 if n * orr + d0 >= 0 else 0)


def test_pick_commutes_with_per_channel_ratecv():
    """picking a channel, then ratecv == ratecv of the interleaved stereo, then picking: the order of
    the reference's offline scripts (set_frame_rate on stereo, then split)"""
    rng = np.random.default_rng(7)
    raw = _capture(rng, 3001, 2)
    both = np.frombuffer(audioop.ratecv(raw.tobytes(), 2, 2, 48000, 16000, None)[0], '<i2')
    for ch in (0, 1):
        got, _ = cr.ratecv_fast(cr.mono(raw, 2, ch), 48000, cr.fresh(48000))
        assert np.array_equal(got, both[ch::2])


def test_converter_streams_and_zero_tail():
    """Converter.convert: ragged frames (zero included), two items per stream, zeros behind out_lens"""
    rng = np.random.default_rng(11)
    clip_frames = 441
    pcm = _capture(rng, 6 * clip_frames, 2).reshape(6, -1)
    frames = np.array([441, 0, 7, 441, 300, 1], np.int32)
    conv = cr.Converter(3, 44100, 2, cr.MEAN)
    out, lens = conv.convert(pcm, frames, items_per_stream=2)
    assert out.shape == (6, cr.out_clip_len(clip_frames, 44100))
    for s in range(3):
        state = None
        for c in (2 * s, 2 * s + 1):
            frag = audioop.tomono(pcm[c, :2 * frames[c]].tobytes(), 2, 0.5, 0.5)
            data, state = audioop.ratecv(frag, 2, 1, 44100, 16000, state)
            want = np.frombuffer(data, '<i2')
            assert lens[c] == len(want) and np.array_equal(out[c, :lens[c]], want)
            assert not out[c, lens[c]:].any()
        assert conv.states[s] == (state[0], state[1][0][1] >> 16)
