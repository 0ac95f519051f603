"""The slice of pydub and librosa.load that the reference's offline pre-conditioning calls.

``standardize_audio`` in both offline scripts (OverlapDetection/scripts/
overlap_detection_post_processing.py:101-148, SpeakerIdentification/scripts/
speaker_identification_post_processing.py:136-188) goes through

* ``AudioSegment.from_file(path, format)`` / ``.set_frame_rate(16000)`` / ``.dBFS`` /
  ``.apply_gain(db)`` / ``.export(path, format='wav')`` (pydub), and
* ``librosa.load(path)`` at its DEFAULT rate 22050 (SI :142; librosa 0.8 resamples with resampy's
  ``kaiser_best`` filter) and ``librosa.load(path, sr=None)``.

``AudioSegment`` keeps pydub's semantics for 16-bit WAV data of any channel count and rate:
``set_frame_rate`` is ``audioop.ratecv(data, 2, channels, rate, new_rate, None)`` and runs on the
GPU (mmla_ratecv, resample.hip; bit-identical to CPython's audioop, tests/test_gpu_resample.py);
``dBFS`` is pydub's ``20 * math.log(audioop.rms / 2^15, 10)`` and ``apply_gain`` ``audioop.mul(data, 2,
10^(db/20))`` (host arithmetic, pinned against stdlib audioop in tests/test_resample_cpu.py).
``duration_seconds``, millisecond slices and ``overlay`` are what ``generate_overlap_segment``
(OverlapDetection/scripts/data_augmentation.py:20-34) calls: ``overlay`` is ``audioop.add`` on the canvas
behind the position and runs on the GPU (mmla_od_mix, mix.hip; bit-identical to CPython's audioop,
tests/test_gpu_od_mix.py), the millisecond arithmetic around it is restated from pydub's source.
``load`` is librosa.load(path, sr=22050 | None, mono=True) for WAV files; its resampling step is
resampy's sinc interpolation on the GPU (mmla_resample_sinc) with the ``kaiser_best`` filter built
here -- resampy is not installed in this image, so that step's parity is unpinned.
"""
import math
import wave

import numpy as np

from . import _lib

# resampy 0.2 'kaiser_best': Kaiser-windowed sinc, 64 zero crossings, 2^9 samples per crossing
KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)


def kaiser_best_table():
    """resampy.filters.sinc_window(num_zeros=64, precision=9, window=kaiser(beta), rolloff) ->
    (right half of the interpolated filter, float64 [64 * 512 + 1], samples per zero crossing)"""
    p = KAISER_BEST
    num_bits = 2 ** p['precision']
    n = num_bits * p['num_zeros']
    sinc_win = p['rolloff'] * np.sinc(p['rolloff'] * np.linspace(0, p['num_zeros'], num=n + 1,
                                                                   endpoint=True))
    taper = np.kaiser(2 * n + 1, p['beta'])[n:]
    return taper * sinc_win, num_bits


_TABLE = {}


def resample(y, orig_sr, target_sr, ctx=None):
    """librosa 0.8 ``resample(y, orig_sr, target_sr, res_type='kaiser_best', fix=True)`` of float32
    mono audio: resampy's sinc interpolation (GPU), then fix_length to ceil(n * ratio)."""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    if orig_sr == target_sr:
        return y
    ctx = ctx or _lib.default_context()
    if 'kb' not in _TABLE:
        _TABLE['kb'] = kaiser_best_table()
    win, num_table = _TABLE['kb']
    n_samples = int(np.ceil(y.shape[-1] * float(target_sr) / orig_sr))
    y_hat = ctx.resample_sinc(y, orig_sr, target_sr, win, num_table)
    if len(y_hat) < n_samples:
        y_hat = np.pad(y_hat, (0, n_samples - len(y_hat)))
    return np.ascontiguousarray(y_hat[:n_samples], dtype=np.float32)


def _read_wav(path):
    """(rate, channels, sample width, interleaved samples) of a PCM WAV file"""
    with wave.open(path, 'rb') as f:
        nch, width, rate, n = f.getparams()[:4]
        data = f.readframes(n)
    if width == 2:
        x = np.frombuffer(data, dtype='<i2').astype(np.int16)
    elif width == 4:
        x = np.frombuffer(data, dtype='<i4').astype(np.int32)
    elif width == 1:
        x = np.frombuffer(data, dtype=np.uint8).copy()
    else:
        raise ValueError(f'{path}: {8 * width}-bit WAV data is not supported')
    return rate, nch, width, x


def load(path, sr=22050, mono=True, ctx=None):
    """``librosa.load(path, sr=sr, mono=True)`` for WAV files -> (float32 y, sr).  soundfile's
    float32 scaling (16-bit x / 2^15, 32-bit x / 2^31, unsigned 8-bit (x - 128) / 2^7), the float32
    channel mean, then -- unless sr is None or the file's rate -- the kaiser_best resampling."""
    if not mono:
        raise ValueError('only mono=True (the reference never asks for more)')
    rate, nch, width, x = _read_wav(path)
    if width == 2:
        y = x.astype(np.float32) / np.float32(32768.0)
    elif width == 4:
        y = x.astype(np.float32) * np.float32(2.0 ** -31)
    else:
        y = (x.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)
    if nch > 1:
        y = np.mean(y.reshape(-1, nch).T, axis=0)        # librosa.to_mono
    y = np.ascontiguousarray(y, dtype=np.float32)
    if sr is not None and sr != rate:
        y = resample(y, rate, sr, ctx)
        rate = sr
    return y, rate


class AudioSegment:
    """pydub.AudioSegment for 16-bit PCM WAV data (what the reference's recordings and zoom
    exports are): ``data`` int16 interleaved frames."""

    sample_width = 2

    def __init__(self, data, frame_rate, channels=1, ctx=None):
        self.data = np.ascontiguousarray(data, dtype=np.int16).reshape(-1)
        if self.data.size % channels:
            raise ValueError(f'{self.data.size} samples are not whole {channels}-channel frames')
        self.frame_rate = int(frame_rate)
        self.channels = int(channels)
        self._ctx = ctx

    @classmethod
    def from_file(cls, path, format=None, ctx=None):
        rate, nch, width, x = _read_wav(path)
        if width != 2:
            raise ValueError(f'{path}: {8 * width}-bit WAV; the GPU ratecv is built for 16-bit PCM')
        return cls(x, rate, nch, ctx)

    from_wav = from_file

    @property
    def ctx(self):
        return self._ctx or _lib.default_context()

    def _spawn(self, data, frame_rate=None):
        return AudioSegment(data, frame_rate or self.frame_rate, self.channels, self._ctx)

    def __len__(self):
        """duration in ms, as pydub"""
        return round(1000 * (self.data.size // self.channels) / self.frame_rate)

    @property
    def frame_count(self):
        return self.data.size // self.channels

    def get_array_of_samples(self):
        return self.data.copy()

    # -- millisecond slices and overlay: the part of pydub that generate_overlap_segment calls
    # (OverlapDetection/scripts/data_augmentation.py:20-34).  pydub is not installed here: __len__,
    # frame_count(ms), _parse_position, __getitem__ and overlay are restated from its published source
    # (0.25), Python-float arithmetic included, and parity with the library itself is unpinned
    # (tests/mix_ref.py restates the same rules a second time; the sums are pinned against audioop.add).
    @property
    def duration_seconds(self):
        """pydub: frame_count() / frame_rate"""
        return self.frame_rate and self.frame_count / self.frame_rate or 0.0

    def _ms_len(self):
        """pydub's len(): round(1000 * (frame_count() / frame_rate)), in its order of operations"""
        return round(1000 * (float(self.frame_count) / self.frame_rate))

    def _parse_position(self, ms):
        """pydub: a millisecond position -> int(frame_count(ms=...)) = int(ms * (frame_rate / 1000.0));
        negative positions count from the end"""
        if ms < 0:
            ms = self._ms_len() - abs(ms)
        if ms == float('inf'):
            ms = self._ms_len()
        return int(ms * (self.frame_rate / 1000.0))

    def _frames(self, start, end):
        """frames [start, end) as pydub's __getitem__ returns them: a slice that ends up to 2 ms past the
        data (len() rounds to whole milliseconds) is filled up with silence, a larger gap is an error"""
        ch = self.channels
        d = self.data[max(start, 0) * ch:max(end, 0) * ch]
        missing = (end - start) - d.size // ch
        if missing > 0 and d.size:
            if missing > 2 * (self.frame_rate / 1000.0):
                raise ValueError(f'{missing} frames are missing from the slice: pydub raises '
                                 'TooManyMissingFrames here')
            d = np.concatenate([d, np.zeros(missing * ch, np.int16)])
        return d

    def __getitem__(self, millisecond):
        """seg[a:b] in milliseconds (floats allowed), seg[t] = one millisecond, as pydub"""
        if isinstance(millisecond, slice):
            if millisecond.step:
                raise ValueError('stepped millisecond slices are not built')
            n = self._ms_len()
            start = millisecond.start if millisecond.start is not None else 0
            end = millisecond.stop if millisecond.stop is not None else n
            start, end = min(start, n), min(end, n)
        else:
            start, end = millisecond, millisecond + 1
        return self._spawn(self._frames(self._parse_position(start), self._parse_position(end)))

    def _overlay_many(self, items):
        """A chain of pydub overlays on this canvas in ONE pass: items = [(seg, position ms, times)], times
        < 0 = loop to the end.  Every overlay is audioop.add on the canvas behind its position, clamped,
        in order (mmla_od_mix on the GPU: the canvas and the segments are the pool, a repeat is one more
        layer on the same samples, and more than 7 layers go through further calls on the result).
        pydub's overlay returns seg1[:position] + the mixed seg1[position:], both millisecond slices: the
        result has int(len() * frame_rate / 1000) frames, i.e. a canvas that is not a whole number of
        milliseconds is cut, or filled up with silence, to one."""
        ch = self.channels
        n_ms = self._ms_len()
        frames = self._parse_position(n_ms)
        canvas = self._frames(0, frames) if items else self.data
        if canvas.size // ch != frames:      # (an empty canvas stays empty)
            return self._spawn(canvas)
        layers = []                          # (segment samples, position in samples)
        for seg, position, times in items:
            seg = seg.set_frame_rate(self.frame_rate).set_channels(ch)
            p = self._parse_position(min(position, n_ms)) * ch
            m = seg.data.size
            while times and m and p < canvas.size:      # pydub's `while times:`, the last repeat truncated
                layers.append((seg.data, p))
                p += m
                times -= 1
        if layers and canvas.size > 600000:
            raise ValueError(f'overlay on a canvas of {canvas.size} samples: the mix takes at most 600000')
        room = _lib.MIX_MAX_LAYERS - 1
        for g in range(0, len(layers), room):
            group = layers[g:g + room]
            srcs, offs = {}, []      # every distinct segment once in the pool
            pool = [canvas]
            used = canvas.size
            for d, p in group:
                if id(d) not in srcs:
                    srcs[id(d)] = used
                    pool.append(d)
                    used += d.size
                offs.append((srcs[id(d)], d.size, p))
            plan = _lib.MixPlan.from_layers([[(0, canvas.size, 0)] + offs])
            out, _ = self.ctx.od_mix(np.concatenate(pool), plan, clip_len=canvas.size)
            canvas = out[0]
        return self._spawn(canvas)

    def overlay(self, seg, position=0, loop=False, times=None, gain_during_overlay=None):
        """pydub's overlay: `seg` (brought to this segment's rate and channels) added onto the canvas from
        `position` ms on, audioop.add per sample (clamped to int16), cut at the canvas's end; times=k
        repeats it back to back, loop=True until the end.  On the GPU (mmla_od_mix)."""
        if gain_during_overlay:
            raise NotImplementedError('gain_during_overlay is not built (the reference never passes it)')
        if loop:
            times = -1
        elif times is None:
            times = 1
        elif times == 0:
            return self._spawn(self.data)
        return self._overlay_many([(seg, position, times)])

    def set_frame_rate(self, frame_rate):
        """audioop.ratecv(data, 2, channels, rate, frame_rate, None) on the GPU"""
        if frame_rate == self.frame_rate:
            return self
        if self.data.size == 0:
            return self._spawn(self.data, frame_rate)
        out = self.ctx.ratecv(self.data, self.channels, self.frame_rate, frame_rate)
        return self._spawn(out, frame_rate)

    def set_channels(self, channels):
        """pydub's set_channels(1) of stereo data: audioop.tomono(data, 2, 0.5, 0.5), i.e.
        floor(0.5 l + 0.5 r) per frame (on the host: one pass over the samples)"""
        if channels == self.channels:
            return self
        if channels != 1 or self.channels != 2:
            raise ValueError(f'set_channels({channels}) of {self.channels}-channel data: only the '
                             'stereo-to-mono downmix is built')
        x = self.data.reshape(-1, 2).astype(np.float64)
        mono = np.floor(0.5 * x[:, 0] + 0.5 * x[:, 1]).astype(np.int16)
        return AudioSegment(mono, self.frame_rate, 1, self._ctx)

    @property
    def rms(self):
        """audioop.rms(data, 2): (unsigned int) sqrt(sum(x^2) / n) with a float64 running sum,
        accumulated sample by sample in order as CPython's loop does (np.add.accumulate is that
        sequential loop; np.sum's pairwise sum and an exact int64 sum differ from it once the sum
        passes 2^53, i.e. after ~8.4 M full-scale samples).  Chunks of 2^20 samples carry the running
        sum, so memory stays O(chunk) for hour-long files with the same summation order."""
        if self.data.size == 0:
            return 0
        flat = self.data.reshape(-1)
        total = 0.0
        for i in range(0, flat.size, 1 << 20):
            c = flat[i:i + (1 << 20)].astype(np.float64)
            total = float(np.add.accumulate(np.concatenate(([total], c * c)))[-1])
        return int(np.sqrt(total / self.data.size))

    max_possible_amplitude = 2 ** 15

    @property
    def dBFS(self):
        """pydub: ratio_to_db(rms / max_possible_amplitude) = 20 * math.log(ratio, 10) (pydub's own
        expression: math.log with a base is log(x) / log(10), which can differ from log10 in the
        last bit); -inf for silence"""
        rms = self.rms
        if not rms:
            return -float('inf')
        return 20 * math.log(rms / float(self.max_possible_amplitude), 10)

    def apply_gain(self, volume_change):
        """audioop.mul(data, 2, 10 ** (volume_change / 20)): per sample x * factor in double,
        bounded (> 32767 -> 32767, < -32767 -> -32768) and floored"""
        factor = 10.0 ** (float(volume_change) / 20.0)
        return self._spawn(mul(self.data, factor))

    def export(self, out_f, format='wav'):
        if format not in (None, 'wav'):
            raise ValueError(f'export format {format!r}: only wav')
        with wave.open(out_f, 'wb') as f:
            f.setnchannels(self.channels)
            f.setsampwidth(2)
            f.setframerate(self.frame_rate)
            f.writeframes(self.data.astype('<i2').tobytes())
        return out_f


def mul(pcm, factor):
    """audioop.mul(pcm, 2, factor) on int16 samples"""
    v = np.asarray(pcm, dtype=np.float64) * float(factor)
    v = np.where(v > 32767.0, 32767.0, np.where(v < -32767.0, -32768.0, v))
    return np.floor(v).astype(np.int16)


def rms(pcm):
    return AudioSegment(pcm, 16000).rms
