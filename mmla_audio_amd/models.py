"""``load_model(path).predict(x)`` facade for the two reference networks.

Replaces ``tf.keras.models.load_model`` + ``Model.predict`` at the reference call sites
(OD ``record_on_pc.py:88,159``; SI ``record_on_pc.py:77,136``;
``speaker_identification_post_processing.py:206,272``; ``overlap_detection_post_processing.py``).

Weights: if ``<path>/variables/variables.data-00000-of-00001`` exists the trained tensors are read
from the TF bundle (``tfbundle.load_bundle``).  The reference does not ship that file
(``.MISSING_LARGE_BLOBS``); like ``tf.keras.models.load_model`` on an incomplete SavedModel, loading
then raises -- a drop-in must not log confident labels from a random net.  Seeded synthetic
weights in the exact reference layout are used only on request (``allow_synthetic=True``;
``model.synthetic`` is then True).
"""
import os
import warnings

import numpy as np

from . import _lib, tfbundle, weights


def _layout_from_path(path):
    """(kind, n_classes, head) from the bundle index (tfbundle.layout), or None without one"""
    idx = os.path.join(path, 'variables', 'variables.index')
    if os.path.exists(idx):
        try:
            return tfbundle.layout(tfbundle.variable_shapes(idx))[:3]
        except ValueError:
            return None
    return None


def _od_channels_from_path(path):
    """the channels the bundle index names for an OD stem kernel [1,1,C,16]; 3 without one"""
    idx = os.path.join(path, 'variables', 'variables.index')
    if os.path.exists(idx):
        k0 = tfbundle.variable_shapes(idx).get('layer_with_weights-0/kernel')
        if k0 is not None and len(k0) == 4 and int(k0[2]) in weights.OD_CHANNELS:
            return int(k0[2])
    return 3


def _kind_from_path(path):
    lay = _layout_from_path(path)
    if lay is not None:
        return lay[0]
    low = path.replace('\\', '/').lower()
    return weights.OD if 'overlap' in low or 'timit2' in low or 'timit1' in low else weights.SI


class _Model:
    kind = None

    def __init__(self, W, n_classes, head, device=None, synthetic=False):
        self.ctx = _lib.default_context(device) if device is None or isinstance(device, int) else device
        self.n_classes = n_classes
        self.head = head
        self.synthetic = synthetic
        self.W = W
        self._load()

    def _pack(self):
        return weights.pack(self.kind, self.W, self.n_classes)

    def _load(self):
        self.ctx.load_weights(self.kind, self._pack(), self.n_classes, self.head)

    def _ensure_loaded(self):
        # several models can share one context; re-load if another model of this kind replaced ours
        cls = self.ctx.od_classes if self.kind == weights.OD else self.ctx.si_classes
        if getattr(self.ctx, f'_owner_{self.kind}', None) is not self or cls != self.n_classes:
            self._load()
            setattr(self.ctx, f'_owner_{self.kind}', self)

    def _predict_conditioned(self, call, pcm, noise, mic, lens, passes, silence_remove,
                             items_per_stream, vad_mode, reset_vad, capture=None, reset_capture=False):
        """the shared body of predict_wavs_conditioned: the bank, the detectors, the converters (capture:
        a room.CaptureFormat; `call` is then the context's *_pipeline_capture), the fused call"""
        from . import noisereduce
        self._ensure_loaded()
        n = len(pcm) if isinstance(pcm, (list, tuple)) else (1 if np.ndim(pcm) == 1 else len(pcm))
        ips = int(items_per_stream)
        if ips < 1 or n % ips:
            raise ValueError(f'{n} clips are not whole streams of {ips}')
        ns = noise is None      # no ambient-noise clips: the non-stationary gate, no bank
        one = isinstance(noise, np.ndarray) and noise.ndim == 1
        noises = [] if ns else [np.ascontiguousarray(x, dtype=np.float32).ravel()
                                for x in ([noise] if one else noise)]
        if mic is None:     # the clip's stream is its microphone
            mic = np.zeros(n, np.int32) if len(noises) <= 1 else np.arange(n, dtype=np.int32) // ips
        mic = np.ascontiguousarray(mic, dtype=np.int32)
        if ns:
            if mic.shape != (n,):
                raise ValueError(f'mic must hold one entry per clip, got shape {mic.shape}')
        elif passes > 0:
            if mic.shape != (n,) or (n and (mic.min() < 0 or mic.max() >= len(noises))):
                raise ValueError(f'mic must hold one index into the {len(noises)} noise clips per clip')
            noisereduce._set_noise_bank(self.ctx, noises, 16000)
        if silence_remove:
            # the reference's module-level webrtcvad.Vad(3): created once, its state carried from
            # clip to clip; one per stream here
            tag = ('conditioned', n // ips, int(vad_mode))
            if reset_vad or getattr(self.ctx, 'vad_owner', None) != tag:
                self.ctx.vad_reset(n // ips, vad_mode)
                self.ctx.vad_owner = tag
        if capture is not None:
            # one audioop.ratecv state per stream, owned as the detectors are: created on the first call
            # or when the stream count or the format changes, carried from call to call otherwise
            fmt = (int(capture.rate), int(capture.channels), int(capture.channel))
            if (reset_capture or getattr(self.ctx, 'capture_format', None) != fmt or
                    getattr(self.ctx, 'capture_streams', None) != n // ips):
                self.ctx.capture_reset(n // ips, *fmt)
        return call(pcm, lens, mic, passes, silence_remove, ips, nonstationary=ns)


class OverlapDetectionModel(_Model):
    """OD-NET (ResLSTM, overlap_detector_temp.py:280-303): predict(float32 [N,128,151,3]) -> [N,K].  K, the
    classes of the softmax head, is the width of W's Dense kernel: 2 for the deployed model, 3 for the
    reference's research models; every [N,2] below is [N,K] for such a model.

    ``channels`` is the stem kernel's [1,1,C,16]: 3, or 1 for a model of ``OverlapDetector(imagetype='gray')``
    (overlap_detector.py:84-90), whose predict reads [N,128,151,1].  ``image_type`` ('zcr', 'gray' or
    'viridis') is the feature image the model was trained on, what ``predict_wavs*`` make in front of the
    network; default 'zcr' for three channels and 'gray' for one (a one-channel model takes no other).  The
    type is not stored in a TF checkpoint -- a three-channel model trained on gray or viridis images must
    be told: ``load_model(path, image_type='viridis')``."""
    kind = weights.OD

    def __init__(self, W, device=None, synthetic=False, image_type=None):
        self.channels = weights.od_channels(W)
        if image_type is None:
            image_type = 'gray' if self.channels == 1 else 'zcr'
        t = _lib.od_image_type(image_type)
        self.image_type = {v: k for k, v in _lib.OD_IMAGE_TYPES.items()}[t]
        if self.channels == 1 and t != _lib.OD_IMG_GRAY:
            raise ValueError(f"a one-channel OD model reads gray images, not {self.image_type!r}")
        super().__init__(W, weights.od_classes(W), _lib.HEAD_SOFTMAX, device, synthetic)
        setattr(self.ctx, f'_owner_{self.kind}', self)

    def _pack(self):
        return weights.pack(self.kind, self.W, self.n_classes, weights.od_channels(self.W))

    def _load(self):
        super()._load()      # the load resets the context's image type to the channel count's default
        self.ctx.od_set_image_type(self.image_type)

    def _ensure_loaded(self):
        super()._ensure_loaded()
        if self.ctx.od_image_type != _lib.od_image_type(self.image_type):   # set behind the model's back
            self.ctx.od_set_image_type(self.image_type)

    def set_weights(self, W):
        """Replace every tensor of the model in place (one ``mmla_load_weights`` of the whole blob): the
        network an adaptation produced (``overlap_detector.continue_train``).  self.W follows only once
        the load succeeded."""
        k, ch = weights.od_classes(W), weights.od_channels(W)
        if ch != self.channels:
            raise ValueError(f'set_weights: a {ch}-channel network for a {self.channels}-channel model')
        blob = weights.pack(self.kind, W, k, ch)
        self.ctx.load_weights(self.kind, blob, k, _lib.HEAD_SOFTMAX)
        self.ctx.od_set_image_type(self.image_type)
        setattr(self.ctx, f'_owner_{self.kind}', self)
        self.W, self.n_classes = dict(W), k

    def predict(self, x, batch_size=None, verbose=0):
        self._ensure_loaded()
        x = np.asarray(x)
        if x.ndim != 4 or x.shape[1:] != (128, 151, self.channels):
            raise ValueError(f'OD model expects [N,128,151,{self.channels}], got {x.shape}')
        return self.ctx.od_forward(x)

    def predict_wavs(self, pcm, lens=None):
        """Fused WAV -> class (no PNG round trip): int16 [N, L] -> (probs [N,2], argmax [N]
        (-1 = 'silent', fewer than 4000 samples: record_on_pc.py:141-154), silent [N])."""
        self._ensure_loaded()
        return self.ctx.od_pipeline(pcm, lens)

    def predict_mixed(self, pool, plan):
        """predict_wavs on clips synthesised on the device: `plan` (a _lib.MixPlan, e.g. from
        data_augmentation.overlap_plan) mixes recordings of the int16 `pool` into 1.5 s clips by the
        reference's overlay chain (data_augmentation.py:20-34), and the network reads them where they
        are -> (probs [N,2], argmax [N] (-1 = 'silent': a canvas below 4000 samples), silent [N])."""
        self._ensure_loaded()
        return self.ctx.od_pipeline_mixed(pool, plan)

    def predict_wavs_gated(self, pcm, noise=None, lens=None, passes=4, threshold=0.3):
        """predict_wavs with the edge loop's silent check (record_on_pi.py:103-124): every clip is
        denoised `passes` times against the float32 noise clip `noise` (16 kHz), a clip whose feature
        image has an SSIM below `threshold` with its denoised image is 'silent', and the network reads
        the denoised image -> (probs [N,2], argmax [N] (-1 = 'silent'), silent [N], ssim [N]).
        noise=None: the passes run the non-stationary gate, which needs no noise clip."""
        from . import noisereduce
        self._ensure_loaded()
        if noise is None:
            return self.ctx.od_pipeline_gated(pcm, lens, passes, threshold, nonstationary=True)
        if passes > 0:
            yn = np.ascontiguousarray(noise, dtype=np.float32).ravel()
            noisereduce._set_noise(self.ctx, yn, 16000)
        return self.ctx.od_pipeline_gated(pcm, lens, passes, threshold)

    def predict_wavs_conditioned(self, pcm, noise=None, mic=None, lens=None, passes=1, silence_remove=True,
                                 items_per_stream=1, vad_mode=3, reset_vad=False, capture=None,
                                 reset_capture=False):
        """predict_wavs behind the PC loop's save_wave_file(noise_reduce=True, silence_remove=True)
        (record_on_pc.py:141-154,200-226) for a room of microphones: clip c is denoised `passes` times
        against the ambient-noise clip of its microphone (`noise`: one float32 clip, or a list with one
        per microphone; `mic[c]` picks the clip's, default its stream), its silence is removed by its
        stream's webrtcvad.Vad(vad_mode) (stream s owns clips [s * items_per_stream, (s + 1) *
        items_per_stream); the detectors are created on the first call or when the stream count or
        the mode changes, and keep their state across calls otherwise; reset_vad=True starts afresh),
        and a clip with fewer than 4000 samples left is 'silent' -> (probs [N,2], argmax [N] (-1 =
        'silent'), silent [N], kept_len [N]).  The bank of profiles is rebuilt only when a noise clip
        changes.  noise=None: the passes run the non-stationary gate (the context's nr_set_nonstationary
        parameters), no bank is built and `mic` is only checked for its shape.
        capture (a room.CaptureFormat): pcm is the microphones' interleaved capture, int16 [N, clip_frames *
        channels] or a list of such clips, `lens` counts capture frames, and every clip is converted to
        16 kHz mono on the device first, by its stream's audioop.ratecv state (created and reset under the
        detectors' rule; reset_capture=True starts afresh); kept_len is at 16 kHz.  capture=None: 16 kHz
        mono in, as before."""
        call = self.ctx.od_pipeline_conditioned if capture is None else self.ctx.od_pipeline_capture
        return self._predict_conditioned(call, pcm, noise, mic, lens, passes, silence_remove,
                                         items_per_stream, vad_mode, reset_vad, capture, reset_capture)


class SpeakerIdModel(_Model):
    """SI-NET (res_model + head, speaker_identification.py:193-218,401-410): predict([N,256,39])."""
    kind = weights.SI

    def __init__(self, W, n_classes, head, device=None, synthetic=False):
        super().__init__(W, n_classes, head, device, synthetic)
        setattr(self.ctx, f'_owner_{self.kind}', self)

    def predict(self, x, batch_size=None, verbose=0):
        self._ensure_loaded()
        x = np.asarray(x)
        if x.ndim != 3 or x.shape[1:] != (256, 39):
            raise ValueError(f'SI model expects [N,256,39], got {x.shape}')
        return self.ctx.si_forward(x)

    def set_head(self, w, b, head=_lib.HEAD_SIGMOID):
        """Replace the Dense head in place (``mmla_si_set_head``): w [512, K], b [K] -- the head a
        registration just fitted, installed without re-uploading the frozen base.  self.W, n_classes and
        head follow, so a later re-load (another model took the context) gives the same model."""
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if w.ndim != 2 or w.shape[0] != _lib.SI_EMBED or b.shape != (w.shape[1],) or w.shape[1] < 1:
            raise ValueError(f'w {w.shape} / b {b.shape}: expected [512,K] and [K], K >= 1')
        if head not in (_lib.HEAD_SOFTMAX, _lib.HEAD_SIGMOID):
            raise ValueError(f'unknown head {head}')
        self._ensure_loaded()
        self.ctx.si_set_head(w, b, head)
        name = weights.si_spec(w.shape[1])[-2][0].rsplit('/', 1)[0]
        W = dict(self.W)
        W[name + '/kernel'] = w.copy()
        W[name + '/bias'] = b.copy()
        self.W, self.n_classes, self.head = W, int(w.shape[1]), int(head)

    def set_weights(self, W, n_classes, head=_lib.HEAD_SIGMOID):
        """Replace every tensor of the model (one ``mmla_load_weights`` of the whole blob): the network
        a fine-tuned registration produced.  self.W, n_classes and head follow only once the load
        succeeded."""
        blob = weights.pack(self.kind, W, int(n_classes))
        self.ctx.load_weights(self.kind, blob, int(n_classes), int(head))
        setattr(self.ctx, f'_owner_{self.kind}', self)
        self.W, self.n_classes, self.head = dict(W), int(n_classes), int(head)

    def save(self, path):
        """``model.save(path)`` for a softmax-headed model (a base model: ``res_model`` / ``train``): its
        variables in the base layout (``tfbundle.save_speaker_base``), which ``load_model(path)`` and
        ``transfer_learning(..., base_model_path=path)`` read back bit for bit.  A sigmoid-headed
        (deployed) model is what ``transfer_learning`` writes itself."""
        if self.head != _lib.HEAD_SOFTMAX:
            raise ValueError('save() writes base models (softmax head); transfer_learning saves the deployed one')
        os.makedirs(path, exist_ok=True)
        tfbundle.save_speaker_base(path, self.W, self.n_classes)

    def predict_wavs(self, pcm, lens=None):
        """Fused WAV -> speaker: -> (probs [N,K], argmax [N] (-1 = 'silent'), silent [N])."""
        self._ensure_loaded()
        return self.ctx.si_pipeline(pcm, lens)

    def predict_wavs_conditioned(self, pcm, noise=None, mic=None, lens=None, passes=1, silence_remove=True,
                                 items_per_stream=1, vad_mode=3, reset_vad=False, capture=None,
                                 reset_capture=False):
        """predict_wavs behind save_wave_file(noise_reduce=True, silence_remove=True) (SI
        record_on_pc.py:117-134,178-205, record_on_pi.py:101-127,228-240); arguments and the returned
        (probs [N,K], argmax, silent, kept_len) as OverlapDetectionModel.predict_wavs_conditioned."""
        call = self.ctx.si_pipeline_conditioned if capture is None else self.ctx.si_pipeline_capture
        return self._predict_conditioned(call, pcm, noise, mic, lens, passes, silence_remove,
                                         items_per_stream, vad_mode, reset_vad, capture, reset_capture)


def load_model(path, kind=None, n_classes=None, head=None, seed=0, device=None,
               allow_synthetic=False, image_type=None):
    """tf.keras.models.load_model drop-in for the reference's model directories: the OD base models
    (timit/models/timit{1.0,2.0}), the SI base model (timit/model, Dense(630) softmax) and the
    deployed SI model transfer_learning saves (experiment/model: the sliced base nested inside a
    model with the customized_dense sigmoid head, speaker_identification.py:401-410,456) -- the
    layout is read from the bundle index (tfbundle.layout), K and the head from its head kernel.
    Raises FileNotFoundError when the trained variables are absent, unless allow_synthetic=True.
    image_type (OD only): the feature image the model reads, 'zcr', 'gray' or 'viridis'; None = 'zcr' for a
    three-channel model, 'gray' for a one-channel one.  A TF checkpoint does not store it."""
    lay = _layout_from_path(path)
    kind = (lay[0] if lay else _kind_from_path(path)) if kind is None else kind
    synthetic = False
    shard = os.path.join(path, 'variables', 'variables.data-00000-of-00001')
    if os.path.exists(shard):
        # present: any failure (a corrupt bundle, libmmla.so missing for the CRC) is a real error
        W, (bkind, bk, bhead) = tfbundle.load_bundle(path, with_layout=True)
        if bkind != kind:
            raise ValueError(f'{path}: bundle holds a {"OD" if bkind == weights.OD else "SI"} model')
        if kind == weights.SI:
            n_classes = bk
            head = bhead if head is None else head
    else:
        if not allow_synthetic:
            raise FileNotFoundError(
                f'{path}: trained variables not found ({shard} is absent); the reference ships only '
                f'variables.index (.MISSING_LARGE_BLOBS). Pass allow_synthetic=True for seeded '
                f'synthetic weights in the reference layout.')
        if lay is not None and kind == weights.SI:   # the layout the index names (K, head)
            n_classes = lay[1] if n_classes is None else n_classes
            head = lay[2] if head is None else head
        if lay is not None and kind == weights.OD and lay[0] == weights.OD and n_classes is None:
            n_classes = lay[1]                        # the Dense shape the index names
        warnings.warn(f'{path}: trained weights absent (reference .MISSING_LARGE_BLOBS); using seeded '
                      f'synthetic weights in the reference layout (seed={seed})')
        channels = _od_channels_from_path(path) if kind == weights.OD else 3
        W = weights.synthetic(kind, seed=seed, n_classes=n_classes, channels=channels)
        synthetic = True
    if kind == weights.OD:
        return OverlapDetectionModel(W, device=device, synthetic=synthetic, image_type=image_type)
    if n_classes is None:
        n_classes = W['layer_with_weights-42/kernel'].shape[1]
    if head is None:
        head = _lib.HEAD_SOFTMAX if n_classes == 630 else _lib.HEAD_SIGMOID
    return SpeakerIdModel(W, n_classes, head, device=device, synthetic=synthetic)
