"""Both detectors for a room of microphones: who speaks and whether speakers overlap, for every
microphone's clip, from ONE conditioning (the noise gate and the silence removal both PC loops run
through save_wave_file(noise_reduce=True, silence_remove=True) before they classify a clip).

Calling ``OverlapDetectionModel.predict_wavs_conditioned`` and ``SpeakerIdModel.predict_wavs_conditioned``
one after the other on one context conditions every clip twice and advances every microphone's
persistent detector twice over the same audio.  ``Room.tick`` is mmla_room_pipeline_conditioned: the
conditioning once, then both networks on the conditioned clips; its results are those of the two
single calls, each on a context of its own.
"""
from collections import namedtuple

import numpy as np

from .overlap_detection_post_processing import LABELS as _OD_LABELS

RoomResult = namedtuple('RoomResult', 'od_probs od_argmax si_probs si_argmax silent kept_len pcm',
                        defaults=(None,))


class Room:
    """``Room(od_model, si_model, noises, vad_mode=3)``: the two models (on one context), the ambient-noise
    clip of every microphone (one float32 clip at 16 kHz, or a list with one per microphone) and the
    detectors' aggressiveness.  The noise bank and the detectors are the context's, owned the way
    ``predict_wavs_conditioned`` owns them: the bank is rebuilt only when a noise clip changes, the
    detectors are created on the first tick or when the stream count or the mode changes and keep their
    state from tick to tick otherwise.  ``noises=None``: a room without ambient-noise recordings, gated by
    the non-stationary gate (no bank; the context's nr_set_nonstationary parameters)."""

    def __init__(self, od_model, si_model, noises=None, vad_mode=3):
        if od_model.ctx is not si_model.ctx:
            raise ValueError('the OD and the SI model of a Room must share one context '
                             '(create them with the same device=Context)')
        self.od, self.si = od_model, si_model
        self.ctx = od_model.ctx
        self.noises = noises
        self.vad_mode = int(vad_mode)

    def tick(self, pcm, mic=None, lens=None, passes=1, silence_remove=True, items_per_stream=1,
             reset_vad=False, return_pcm=False):
        """int16 [N, L] (or a list of clips) -> RoomResult(od_probs [N,2], od_argmax [N], si_probs [N,K],
        si_argmax [N], silent [N] bool, kept_len [N], pcm).  Clip c is gated `passes` times against the
        noise clip of microphone mic[c] (default: its stream), its silence is removed by its stream's
        detector (stream s owns clips [s * items_per_stream, (s + 1) * items_per_stream)); with fewer than
        4000 samples left it is 'silent' and both argmax are -1.  pcm (return_pcm=True) is the conditioned
        clips, zeros behind kept_len."""
        self.si._ensure_loaded()

        def call(x, ln, m, p, sr, ips, nonstationary=False):
            return self.ctx.room_pipeline_conditioned(x, ln, m, p, sr, ips, return_pcm=return_pcm,
                                                      nonstationary=nonstationary)

        return RoomResult(*self.od._predict_conditioned(call, pcm, self.noises, mic, lens, passes,
                                                        silence_remove, items_per_stream, self.vad_mode,
                                                        reset_vad))

    @staticmethod
    def labels(result, speaker_id_dict):
        """-> (overlap labels, speaker labels) per clip in the reference's strings: 'overlapped' /
        'non-overlapped' and speaker_id_dict[str(argmax)]; 'silent' where the argmax is -1."""
        od = [_OD_LABELS[str(int(a))] for a in np.asarray(result.od_argmax)]
        si = ['silent' if a < 0 else speaker_id_dict[str(int(a))] for a in np.asarray(result.si_argmax)]
        return od, si
