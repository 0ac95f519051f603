"""Both detectors for a room of microphones: who speaks and whether speakers overlap, for every
microphone's clip, from ONE conditioning (the noise gate and the silence removal both PC loops run
through save_wave_file(noise_reduce=True, silence_remove=True) before they classify a clip).

Calling ``OverlapDetectionModel.predict_wavs_conditioned`` and ``SpeakerIdModel.predict_wavs_conditioned``
one after the other on one context conditions every clip twice and advances every microphone's
persistent detector twice over the same audio.  ``Room.tick`` is mmla_room_pipeline_conditioned: the
conditioning once, then both networks on the conditioned clips; its results are those of the two
single calls, each on a context of its own.

A room whose microphones do not deliver 16 kHz mono (USB microphones and conference arrays: 44.1 or 48 kHz,
usually interleaved stereo) names its format once, ``Room(..., capture=CaptureFormat(48000, 2, 0))``: every
tick then converts the raw capture on the device first (mmla_room_pipeline_capture), bit-identical to
audioop.ratecv with its state carried per microphone from tick to tick.
"""
from collections import namedtuple

import numpy as np

from .overlap_detection_post_processing import LABELS as _OD_LABELS

RoomResult = namedtuple('RoomResult', 'od_probs od_argmax si_probs si_argmax silent kept_len pcm',
                        defaults=(None,))

MEAN = -1      # CaptureFormat.channel: pydub's set_channels(1) of a stereo capture


class CaptureFormat(namedtuple('CaptureFormat', 'rate channels channel', defaults=(1, 0))):
    """``CaptureFormat(rate, channels=1, channel=0)``: the microphones' capture is 16-bit PCM at `rate` Hz
    with `channels` interleaved channels; the mono signal the room listens to is channel `channel`
    (the Pi loops' ``[k::channels]``) or, for stereo, ``MEAN``: audioop.tomono(data, 2, 0.5, 0.5)."""
    __slots__ = ()

    def __new__(cls, rate, channels=1, channel=0):
        rate, channels, channel = int(rate), int(channels), int(channel)
        if not 1 <= rate <= 384000:
            raise ValueError(f'capture rate {rate} outside 1..384000 Hz')
        if not 1 <= channels <= 8:
            raise ValueError(f'{channels} capture channels outside 1..8')
        if channel == MEAN and channels != 2:
            raise ValueError('CaptureFormat MEAN is for stereo capture')
        if not MEAN <= channel < channels:
            raise ValueError(f'channel {channel} of a {channels}-channel capture')
        return super().__new__(cls, rate, channels, channel)


class Room:
    """``Room(od_model, si_model, noises, vad_mode=3, capture=None)``: the two models (on one context), the ambient-noise
    clip of every microphone (one float32 clip at 16 kHz, or a list with one per microphone) and the
    detectors' aggressiveness.  The noise bank and the detectors are the context's, owned the way
    ``predict_wavs_conditioned`` owns them: the bank is rebuilt only when a noise clip changes, the
    detectors are created on the first tick or when the stream count or the mode changes and keep their
    state from tick to tick otherwise.  ``noises=None``: a room without ambient-noise recordings, gated by
    the non-stationary gate (no bank; the context's nr_set_nonstationary parameters).
    ``capture`` (a CaptureFormat): the ticks take the microphones' raw interleaved capture and convert it to
    16 kHz mono on the device; one converter per stream, owned as the detectors are.  ``noises`` stays
    float32 at 16 kHz either way (``Room.convert`` brings a recording in the room's format there)."""

    def __init__(self, od_model, si_model, noises=None, vad_mode=3, capture=None):
        if od_model.ctx is not si_model.ctx:
            raise ValueError('the OD and the SI model of a Room must share one context '
                             '(create them with the same device=Context)')
        self.od, self.si = od_model, si_model
        self.ctx = od_model.ctx
        self.noises = noises
        self.vad_mode = int(vad_mode)
        self.capture = None if capture is None else CaptureFormat(*capture)

    def tick(self, pcm, mic=None, lens=None, passes=1, silence_remove=True, items_per_stream=1,
             reset_vad=False, return_pcm=False, reset_capture=False):
        """int16 [N, L] (or a list of clips) -> RoomResult(od_probs [N,2], od_argmax [N], si_probs [N,K],
        si_argmax [N], silent [N] bool, kept_len [N], pcm).  Clip c is gated `passes` times against the
        noise clip of microphone mic[c] (default: its stream), its silence is removed by its stream's
        detector (stream s owns clips [s * items_per_stream, (s + 1) * items_per_stream)); with fewer than
        4000 samples left it is 'silent' and both argmax are -1.  pcm (return_pcm=True) is the conditioned
        clips, zeros behind kept_len.  In a room with a capture format pcm is int16 [N, clip_frames *
        channels] interleaved (or a list of such clips), lens counts capture frames, and kept_len and pcm
        are at 16 kHz; reset_capture=True starts the converters afresh."""
        self.si._ensure_loaded()
        fused = (self.ctx.room_pipeline_conditioned if self.capture is None
                 else self.ctx.room_pipeline_capture)

        def call(x, ln, m, p, sr, ips, nonstationary=False):
            return fused(x, ln, m, p, sr, ips, return_pcm=return_pcm, nonstationary=nonstationary)

        return RoomResult(*self.od._predict_conditioned(call, pcm, self.noises, mic, lens, passes,
                                                        silence_remove, items_per_stream, self.vad_mode,
                                                        reset_vad, self.capture, reset_capture))

    def convert(self, recording, chunk_frames=480000):
        """A whole recording in the room's capture format (interleaved int16) -> int16 at 16 kHz mono: the
        ticks' conversion from a fresh state, the converters of the live streams left alone.  For the
        ambient-noise and registration recordings, e.g. ``noises=[room.convert(r) / 32768.0 ...]``."""
        if self.capture is None:
            raise ValueError('Room.convert needs a room with a capture format')
        rate, ch, sel = self.capture
        x = np.ascontiguousarray(recording, dtype=np.int16).reshape(-1)
        if x.size % ch:
            raise ValueError(f'{x.size} samples are not whole frames of {ch} channels')
        # one stream of whole chunks and a ragged last one, the state carried across them on the device;
        # a chunk stays below the converted clips' limit of 600000 samples
        chunk = max(1, min(int(chunk_frames), 600000 * rate // 16000 // 2))
        clips = [x[i:i + chunk * ch] for i in range(0, x.size, chunk * ch)]
        if not clips:
            return np.zeros(0, np.int16)
        live = (getattr(self.ctx, 'capture_format', None), getattr(self.ctx, 'capture_streams', None))
        if live[0] != tuple(self.capture):
            # no converters in this format yet: the format is the context's, so create them (fresh)
            self.ctx.capture_reset(live[1] if live[0] is not None and live[1] else 1, rate, ch, sel)
        out, lens = self.ctx.capture_convert(clips, items_per_stream=len(clips), fresh=True)
        return np.concatenate([out[i, :lens[i]] for i in range(len(clips))])

    @staticmethod
    def labels(result, speaker_id_dict):
        """-> (overlap labels, speaker labels) per clip in the reference's strings: 'overlapped' /
        'non-overlapped' and speaker_id_dict[str(argmax)]; 'silent' where the argmax is -1."""
        od = [_OD_LABELS[str(int(a))] for a in np.asarray(result.od_argmax)]
        si = ['silent' if a < 0 else speaker_id_dict[str(int(a))] for a in np.asarray(result.si_argmax)]
        return od, si
