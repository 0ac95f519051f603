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

from .overlap_detection_post_processing import class_label as _od_label

RoomResult = namedtuple('RoomResult', 'od_probs od_argmax si_probs si_argmax silent kept_len pcm',
                        defaults=(None,))

OverlapCheck = namedtuple('OverlapCheck', 'confusion recall precision probs argmax labels talkers n_windows')

OverlapAdapt = namedtuple('OverlapAdapt', 'before after history epochs_run n_windows')

Registration = namedtuple('Registration', 'speaker_id_dict accuracy kept_len n_windows history '
                          'fine_tune_history', defaults=(None,))

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
        """int16 [N, L] (or a list of clips) -> RoomResult(od_probs [N,C] for an OD model of C classes
        (2 for the deployed one), od_argmax [N], si_probs [N,K], si_argmax [N], silent [N] bool, kept_len [N],
        pcm).  Clip c is gated `passes` times against the
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

    def _enrol(self, recordings, mic, passes, silence_remove, return_pcm):
        """The conditioning of whole recordings that register and overlap_check share: one int16 recording
        per speaker (through ``Room.convert`` in a room with a capture format), all conditioned in one batch
        with the room's gate (its noise bank with mic[k], default 0; the non-stationary gate when ``noises
        is None``) and a fresh detector each -- the live streams' detectors and converters are left alone.
        -> (the 16 kHz recordings, ``Context.si_enrol_embed``'s result)"""
        from . import _lib, noisereduce
        K = len(recordings)
        ns = self.noises is None
        one = isinstance(self.noises, np.ndarray) and self.noises.ndim == 1
        noises = [] if ns else [np.ascontiguousarray(x, dtype=np.float32).ravel()
                                for x in ([self.noises] if one else self.noises)]
        mic = np.zeros(K, np.int32) if mic is None else np.ascontiguousarray(mic, dtype=np.int32)
        if mic.shape != (K,):
            raise ValueError(f'mic must hold one entry per speaker, got shape {mic.shape}')
        if not ns and (mic.min() < 0 or mic.max() >= len(noises)):
            raise ValueError(f'mic must hold one index into the {len(noises)} noise clips per speaker')
        recs = [self.convert(r) if self.capture is not None
                else np.ascontiguousarray(r, dtype=np.int16).reshape(-1) for r in recordings]
        longest = max(len(r) for r in recs)
        if longest > _lib.ENROL_MAX_SAMPLES:
            raise ValueError(f'a recording of {longest} samples at 16 kHz exceeds {_lib.ENROL_MAX_SAMPLES}')
        self.si._ensure_loaded()
        if not ns and passes > 0:
            noisereduce._set_noise_bank(self.ctx, noises, 16000)
        return recs, self.ctx.si_enrol_embed(
            recs, profile=mic, passes=passes, silence_remove=silence_remove, vad_mode=self.vad_mode,
            nonstationary=ns, return_pcm=return_pcm)

    def register(self, recordings, names, mic=None, passes=1, silence_remove=True, seed=1, epochs=500,
                 restarts=1, save_to=None, fine_tune=False, fine_tune_epochs=20):
        """Enrol the room's speakers (step 2 and 3 of the reference's manual: SpeakerIdentification/scripts/
        record_on_pc.py:300-346) on the context the room ticks on: ``recordings`` is one int16 array per
        speaker -- interleaved capture in a room with a capture format (it goes through ``Room.convert``:
        fresh states, the live converters left alone), 16 kHz mono otherwise -- and ``names`` their unique
        names; class k is names[k].  All recordings are conditioned in one batch with the room's gate (its
        noise bank with mic[k], default 0; the non-stationary gate when ``noises is None``) and a fresh
        detector each (the live streams' detectors are left alone), cut into 256-frame windows, embedded by
        the frozen base (``mmla_si_enrol_embed``) and fitted (``fit_registration``: the reference's call,
        test split 0; labels k repeated n_windows[k] times).  The fitted head is installed in place
        (``SpeakerIdModel.set_head``): the next tick answers with the new speakers.  ``save_to`` also writes
        the deployed bundle and speaker_id_dict.json there, so ``load_model(save_to)`` gives the same model.
        -> Registration(speaker_id_dict {str(k): names[k]}, accuracy (validation, of the kept restart),
        kept_len [K] (the reference asks to re-record when less than 50 s are left), n_windows [K], history
        [restarts, epochs, 4], fine_tune_history).  ``fine_tune=True`` adds stage 2 of the reference's
        transfer_learning (``speaker_identification.fine_tune``): the fitted head plus the base, every
        layer trainable, `fine_tune_epochs` epochs of RMSprop at 1e-6 on the MFCC windows of the same
        conditioned recordings (``si_features_seq_batch`` of what the enrolment kept); the room then loads
        the whole fine-tuned network once instead of the head, ``save_to`` holds it, accuracy is stage 2's
        final val_acc and fine_tune_history its [fine_tune_epochs, 4] (None without stage 2).  A speaker
        with no window left raises ValueError naming the speaker; the room is unchanged when anything
        raises."""
        import json
        import os

        from . import _lib, tfbundle
        from . import speaker_identification as _si
        from .speaker_identification import deployed_weights, fit_registration
        names = [str(x) for x in names]
        K = len(names)
        if K < 1 or len(recordings) != K:
            raise ValueError(f'{len(recordings)} recordings for {K} names: one recording per speaker')
        if len(set(names)) != K:
            raise ValueError('speaker names must be unique: '
                             f'{sorted(x for x in set(names) if names.count(x) > 1)} repeat')
        if K > _lib.SI_TRAIN_MAX_CLASSES:
            raise ValueError(f'{K} speakers: the head trainer fits at most {_lib.SI_TRAIN_MAX_CLASSES}')
        if epochs < 1 or restarts < 1 or passes < 0:
            raise ValueError('epochs and restarts must be >= 1, passes >= 0')
        ft_epochs = int(fine_tune_epochs) if fine_tune else 0
        if ft_epochs < 0:
            raise ValueError('fine_tune_epochs must be >= 0')
        recs, enrolled = self._enrol(recordings, mic, passes, silence_remove, ft_epochs > 0)
        emb, n_windows, kept_len = enrolled[:3]
        out_pcm = enrolled[3] if ft_epochs > 0 else None    # stage 2 needs the windows, not the embeddings
        for k in range(K):
            if n_windows[k] < 1:
                raise ValueError(f'speaker {names[k]!r}: no audio left after conditioning '
                                 f'({len(recs[k])} samples recorded, {int(kept_len[k])} kept)')
        labels = np.repeat(np.arange(K, dtype=np.int32), n_windows)
        x = np.concatenate([emb[k, :n_windows[k]] for k in range(K)])
        fit = fit_registration(x, labels, K, seed, 0, epochs, restarts, self.ctx, ft_epochs)
        W = deployed_weights(self.si.W, fit.w, fit.b)
        accuracy, ft_history = fit.accuracy, None
        if ft_epochs > 0:
            feat, nw = self.ctx.si_features_seq_batch(out_pcm, lens=kept_len)
            if nw.tolist() != list(n_windows):
                raise RuntimeError(f'windows of the conditioned recordings {nw.tolist()} != {list(n_windows)}')
            windows = np.concatenate([feat[k, :n_windows[k]] for k in range(K)])
            W, ft_history = _si.fine_tune(W, K, windows, labels, fit.plan, ft_epochs, device=self.ctx)
            accuracy = _si.fine_tune_accuracy(ft_history, fit.plan)
        speaker_id_dict = {str(k): names[k] for k in range(K)}
        if save_to is not None:
            os.makedirs(save_to, exist_ok=True)
            tfbundle.save_deployed(save_to, W, K)
            with open(os.path.join(save_to, 'speaker_id_dict.json'), 'w') as f:
                json.dump(speaker_id_dict, f)
        if ft_epochs > 0:
            self.si.set_weights(W, K, _lib.HEAD_SIGMOID)
        else:
            self.si.set_head(fit.w, fit.b, _lib.HEAD_SIGMOID)
        return Registration(speaker_id_dict, accuracy, kept_len, n_windows, fit.history, ft_history)

    def _two_class_od(self, what):
        """overlap_plan labels two classes (single / overlapped): an OD model with another head cannot be
        scored or fitted on its mixes"""
        if self.od.n_classes != 2:
            raise ValueError(f'{what}: the mix recipe labels two classes, the OD model has K = {self.od.n_classes}')

    def overlap_check(self, recordings, mic=None, passes=1, silence_remove=True, n_overlapped=256,
                      n_single=256, seed=1):
        """Does the room's OD model tell overlap from single speech for ITS speakers, through its microphones
        and its noise gate?  ``recordings`` is one int16 recording per speaker, as for ``register``, and is
        conditioned exactly as ``register`` conditions it (``_enrol``).  What is kept of every recording is
        cut into whole 24000-sample windows, all windows form one pool, ``data_augmentation.overlap_plan``
        (seeded by ``seed``) draws n_overlapped mixes of 2-5 speakers in the reference's shares and n_single
        single windows, and one ``mmla_od_pipeline_mixed`` mixes and classifies them on the context the room
        ticks on; the mixed PCM never reaches the host.  -> OverlapCheck(confusion [2,2] (rows = truth,
        columns = predicted), recall and precision of 'overlapped' (overlap_detector_temp.py:455-466), probs
        [n,2], argmax [n], labels [n] (1 = overlapped), talkers [n], n_windows [K]).  Fewer than two speakers
        with a window left raises ValueError naming the speakers without one; the room (detectors,
        converters, models) is unchanged."""
        import random

        from . import _lib
        from .data_augmentation import confusion, overlap_plan
        self._two_class_od('overlap_check')
        K = len(recordings)
        if K < 2:
            raise ValueError(f'{K} recordings: an overlap check needs at least two speakers')
        if passes < 0 or n_overlapped < 0 or n_single < 0:
            raise ValueError('passes, n_overlapped and n_single must be >= 0')
        recs, (_, _, kept_len, pcm) = self._enrol(recordings, mic, passes, silence_remove, True)
        n_windows = np.asarray(kept_len, np.int64) // _lib.OD_CLIP
        if np.count_nonzero(n_windows) < 2:
            short = [k for k in range(K) if n_windows[k] == 0]
            raise ValueError(f'speakers {short}: fewer than {_lib.OD_CLIP} samples left after conditioning '
                             f'({[len(recs[k]) for k in short]} recorded, {[int(kept_len[k]) for k in short]} '
                             'kept); an overlap check needs two speakers with a whole window')
        pool = np.concatenate([pcm[k, :n_windows[k] * _lib.OD_CLIP] for k in range(K)])
        plan, labels, talkers = overlap_plan(n_windows * _lib.OD_CLIP, range(K), n_overlapped, n_single,
                                             random.Random(seed))
        probs, argmax, _ = self.od.predict_mixed(pool, plan)
        matrix, recall, precision = confusion(labels, argmax)
        return OverlapCheck(matrix, recall, precision, probs, argmax, labels, talkers, n_windows.astype(np.int32))

    def overlap_adapt(self, recordings, mic=None, passes=1, silence_remove=True, n_overlapped=256, n_single=256,
                      epochs=20, batch=16, weighted=True, patience=10, seed=1, save_to=None, install=True):
        """The remedy when ``overlap_check`` says the room's OD model does poorly for its speakers: fit it
        further on their own voices (``overlap_detector.continue_train``: the reference's
        ``continue_train_model`` on the device).  ``recordings`` is one int16 recording per speaker, conditioned
        as ``overlap_check`` conditions it.  Each speaker's first 80 % of whole 24000-sample windows go to the
        training pool and the rest to the validation pool, so validation mixes are made of audio the fit never
        saw.  ``data_augmentation.overlap_plan`` (one random.Random(seed)) draws n_overlapped + n_single
        training mixes, then a quarter as many (at least one each) validation mixes; ``od_mix`` mixes them and
        the project's front end makes the feature images, of the model's image type (a three-channel model of any
        type; a one-channel model raises ValueError).  The validation mixes are scored with the current
        model (`before`), the fit runs `epochs` epochs at most (Adadelta, the cosine schedule, class weights
        when `weighted`, early stopping with `patience`), and they are scored again (`after`).  ``install``
        loads the new weights into the room in place; ``save_to`` writes them (``tfbundle.save_overlap``).
        -> OverlapAdapt(before, after: (confusion [2,2], recall, precision); history [epochs, 5];
        epochs_run; n_windows [K]).  A speaker without a window in either pool raises ValueError naming the
        speaker; the room (detectors, converters, both models) is unchanged when anything raises, and with
        ``install=False``."""
        import os
        import random

        from . import _lib, overlap_detector, tfbundle
        from .data_augmentation import confusion, overlap_plan
        self._two_class_od('overlap_adapt')
        if self.od.channels != 3:
            raise ValueError(f'overlap_adapt: the OD model reads {self.od.channels}-channel images; training on '
                             'device-made images is built for three-channel models only')
        K = len(recordings)
        if K < 2:
            raise ValueError(f'{K} recordings: an overlap adaptation needs at least two speakers')
        if passes < 0 or n_overlapped < 1 or n_single < 1 or epochs < 0 or batch < 1 or patience < 0:
            raise ValueError('passes, epochs and patience must be >= 0; n_overlapped, n_single and batch >= 1')
        recs, (_, _, kept_len, pcm) = self._enrol(recordings, mic, passes, silence_remove, True)
        n_windows = np.asarray(kept_len, np.int64) // _lib.OD_CLIP
        n_tr = n_windows * 4 // 5
        for k in range(K):
            if n_tr[k] < 1 or n_windows[k] - n_tr[k] < 1:
                raise ValueError(f'speaker {k}: {int(n_windows[k])} whole windows of {_lib.OD_CLIP} samples left '
                                 f'after conditioning ({len(recs[k])} samples recorded, {int(kept_len[k])} kept); '
                                 'the training and the validation pool each need one')
        clip = _lib.OD_CLIP
        pool_tr = np.concatenate([pcm[k, :n_tr[k] * clip] for k in range(K)])
        pool_va = np.concatenate([pcm[k, n_tr[k] * clip:n_windows[k] * clip] for k in range(K)])
        rng = random.Random(seed)
        plan_tr, labels_tr, _ = overlap_plan(n_tr * clip, range(K), n_overlapped, n_single, rng)
        plan_va, labels_va, _ = overlap_plan((n_windows - n_tr) * clip, range(K), max(n_overlapped // 4, 1),
                                             max(n_single // 4, 1), rng)

        def images(pool, plan):
            clips, lens = self.ctx.od_mix(pool, plan)
            return self.ctx.od_features(clips, lens=lens, db=False, norm=False, zcr=False,
                                        image_type=self.od.image_type)['img']

        img_tr, img_va = images(pool_tr, plan_tr), images(pool_va, plan_va)

        def score():
            return confusion(labels_va, self.od.predict(img_va).argmax(axis=1))

        before = score()
        plan = overlap_detector.fit_plan(labels_tr, seed, epochs, val_ratio=0)
        n = len(labels_tr)
        plan['train'], plan['val'] = np.arange(n), n + np.arange(len(labels_va))
        old = self.od.W
        W, history, epochs_run = overlap_detector.continue_train(
            old, np.concatenate([img_tr, img_va]), np.concatenate([labels_tr, labels_va]), plan, epochs, batch,
            weighted=weighted, patience=patience, device=self.ctx)
        try:
            self.od.set_weights(W)
            after = score()
            if save_to is not None:
                os.makedirs(save_to, exist_ok=True)
                tfbundle.save_overlap(save_to, W)
        except BaseException:
            self.od.set_weights(old)
            raise
        if not install:
            self.od.set_weights(old)
        return OverlapAdapt(before, after, history, epochs_run, n_windows.astype(np.int32))

    @staticmethod
    def labels(result, speaker_id_dict):
        """-> (overlap labels, speaker labels) per clip in the reference's strings: 'overlapped' /
        'non-overlapped' (the class number for an OD model of more than two classes) and
        speaker_id_dict[str(argmax)]; 'silent' where the argmax is -1."""
        k = np.shape(result.od_probs)[1]
        od = [_od_label(a, k) for a in np.asarray(result.od_argmax)]
        si = ['silent' if a < 0 else speaker_id_dict[str(int(a))] for a in np.asarray(result.si_argmax)]
        return od, si
