"""ctypes binding of libmmla.so (include/mmla.h).  The only way the Python side reaches the GPU.

There is deliberately no CPU fallback: if the in-tree ``libmmla.so`` is missing or no HIP device is
present, every entry point raises.  (The numpy restatement in ``oracle/`` is test infrastructure and
is never imported from here.)
"""
import ctypes
import os
import threading
from collections import namedtuple

import numpy as np

from . import weights

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmmla.so')

MMLA_OK = 0
MMLA_DEVICE_PTR = 0x1
MMLA_NR_NONSTATIONARY = 0x2
MMLA_CAPTURE_FRESH = 0x4
MMLA_CAPTURE_MEAN = -1
MODEL_OD, MODEL_SI = 0, 1
HEAD_SOFTMAX, HEAD_SIGMOID = 0, 1
# the OD feature images (mmla.h MMLA_OD_IMG_*); a feature call takes the type in two flag bits
OD_IMG_ZCR, OD_IMG_GRAY, OD_IMG_VIRIDIS = 0, 1, 2
OD_IMAGE_TYPES = {'zcr': OD_IMG_ZCR, 'gray': OD_IMG_GRAY, 'viridis': OD_IMG_VIRIDIS}
_OD_IMG_SHIFT = 4


def od_image_type(t):
    """'zcr' / 'gray' / 'viridis' (or the OD_IMG_* integer, or None = ZCR) -> the OD_IMG_* integer"""
    if t is None:
        return OD_IMG_ZCR
    if isinstance(t, str):
        if t not in OD_IMAGE_TYPES:
            raise ValueError(f'image type {t!r}: expected one of {sorted(OD_IMAGE_TYPES)}')
        return OD_IMAGE_TYPES[t]
    if int(t) not in OD_IMAGE_TYPES.values():
        raise ValueError(f'image type {t!r}: expected one of {sorted(OD_IMAGE_TYPES)}')
    return int(t)


def _img_flags(t):
    return od_image_type(t) << _OD_IMG_SHIFT
PREC_F32, PREC_F16X3 = 0, 1

OD_MELS, OD_FRAMES, OD_CLIP = 128, 151, 24000
SI_FRAMES, SI_DIMS, SI_SILENT_LEN = 256, 39, 4000
SI_EMBED, SI_TRAIN_MAX_CLASSES = 512, 32
SI_BASE_MAX_CLASSES = 1024
OD_TRAIN_MAX_BATCH, OD_DROP_UNITS = 64, 512
OD_AUG_MAX_LEVELS = 8
ENROL_MAX_SAMPLES = 1966080
MIX_MAX_LAYERS = 8


def si_seq_frames(n):
    """psf's frame count T(n) of a signal of n >= 1 samples (400-sample frames, step 160)"""
    n = int(n)
    return 1 if n <= 400 else 1 + -(-(n - 400) // 160)


def si_seq_windows(n):
    """256-frame windows of a signal of n samples: ceil(T(n) / 256), 0 for an empty signal"""
    return -(-si_seq_frames(n) // SI_FRAMES) if int(n) > 0 else 0

MMLA_E_INVALID = -1
MMLA_E_RANGE = -6
_ERRORS = {-1: 'MMLA_E_INVALID', -2: 'MMLA_E_HIP', -3: 'MMLA_E_NOWEIGHTS', -4: 'MMLA_E_OOM',
           -5: 'MMLA_E_SHAPE', -6: 'MMLA_E_RANGE'}

_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32
_U32 = ctypes.c_uint32

# ctx, pcm, n_clips, clip_stride, lens (capture: frames), clip_len (clip_frames), profile, nr_passes,
# silence_remove, items_per_stream, out_pcm, kept_len: what mmla_condition and the conditioned and capture
# pipelines all begin with; each network adds (probs, argmax), the pipelines `silent`, then the flags
_COND = [_P, _P, _I64, _I64, _P, _I32, _P, _I32, _I32, _I64, _P, _P]

# name -> argtypes (all return int)
SIGNATURES = {
    'mmla_nr_set_noise': [_P, _P, _I64, ctypes.c_int32, ctypes.c_uint32],
    'mmla_nr_reduce': [_P, _P, _I64, _I64, _I64, _P, ctypes.c_uint32],
    'mmla_nr_set_noise_bank': [_P, _P, _I64, _I64, _P, _I32, _I32, _U32],
    'mmla_nr_reduce_bank': [_P, _P, _I64, _I64, _I64, _P, _P, _U32],
    'mmla_nr_set_nonstationary': [_P, ctypes.c_double, ctypes.c_double, ctypes.c_double, _I32],
    'mmla_nr_reduce_ns': [_P, _P, _I64, _I64, _I64, _P, _U32],
    'mmla_condition': _COND + [_U32],
    'mmla_od_pipeline_conditioned': _COND + [_P] * 3 + [_U32],
    'mmla_si_pipeline_conditioned': _COND + [_P] * 3 + [_U32],
    'mmla_room_pipeline_conditioned': _COND + [_P] * 5 + [_U32],
    'mmla_capture_reset': [_P, _I64, _I32, _I32, _I32],
    'mmla_capture_convert': [_P, _P, _I64, _I64, _P, _I32, _I64, _P, _I64, _P, _U32],
    'mmla_capture_state': [_P, _P, _P],
    'mmla_od_pipeline_capture': _COND + [_P] * 3 + [_U32],
    'mmla_si_pipeline_capture': _COND + [_P] * 3 + [_U32],
    'mmla_room_pipeline_capture': _COND + [_P] * 5 + [_U32],
    'mmla_debug_vad_path': [_P, _I64, ctypes.POINTER(_I32)],
    'mmla_debug_nr_thresh': [_P, _P, _I64, ctypes.POINTER(_I64)],
    'mmla_abi_version': [],
    'mmla_crc32c': [_P, _I64, ctypes.POINTER(_U32)],
    'mmla_png_unfilter': [_P, _I64, _I64, _I32, _P],
    'mmla_debug_od_image_lut': [_I32, _P],
    'mmla_create': [ctypes.c_int, ctypes.POINTER(_P)],
    'mmla_destroy': [_P],
    'mmla_set_stream': [_P, _P],
    'mmla_synchronize': [_P],
    'mmla_set_microbatch': [_P, _I64, _I64],
    'mmla_get_microbatch': [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)],
    'mmla_release_workspace': [_P],
    'mmla_range_check': [_P, ctypes.POINTER(_I64)],
    'mmla_set_precision': [_P, ctypes.c_int],
    'mmla_load_weights': [_P, ctypes.c_int, _P, _I64, _I32, _I32],
    'mmla_od_features': [_P, _P, _I64, _I64, _P, _I32, _P, _P, _P, _P, _U32],
    'mmla_od_features_f32': [_P, _P, _I64, _I64, _P, _I32, _P, _P, _P, _P, _U32],
    'mmla_si_features': [_P, _P, _I64, _I64, _P, _I32, _P, _P, _U32],
    'mmla_si_features_seq': [_P, _P, _I64, _I64, _P, _U32],
    'mmla_si_features_seq_batch': [_P, _P, _I64, _I64, _P, _I32, _P, _P, _U32],
    'mmla_si_enrol_embed': [_P, _P, _I64, _I64, _P, _I32, _P, _I32, _I32, _I32, _P, _P, _P, _P, _U32],
    'mmla_si_set_head': [_P, _P, _P, _I32, _I32],
    'mmla_od_forward': [_P, _P, _I64, _P, _U32],
    'mmla_od_forward_u8': [_P, _P, _I64, _P, _U32],
    'mmla_si_forward': [_P, _P, _I64, _P, _U32],
    'mmla_si_embed': [_P, _P, _I64, _P, _U32],
    'mmla_si_head_fit': [_P, _P, _P, _I64, _P, _P, _I64, _I32, _I32, _I32, _I32, ctypes.c_float,
                         _P, _P, _P, _P, _P, _P, _U32],
    'mmla_si_loss_grad': [_P, _P, _I64, _I32, _P, _P, _I64, _P, _P, _U32],
    'mmla_si_finetune': [_P, _P, _I64, _I32, _P, _P, _I64, _P, _P, _I64, _I32, _I32, ctypes.c_float,
                         _P, _P, _P, _U32],
    # ctx, drop_seed, epoch, sample_ids, n, mask_a, mask_b
    'mmla_si_base_drop_mask': [_P, _I64, _I32, _P, _I64, _P, _P, _U32],
    # ctx, packed, n_floats, n_classes, x, labels, n, drop_seed, epoch, sample_ids, loss, grad, moving_out
    'mmla_si_base_loss_grad': [_P, _P, _I64, _I32, _P, _P, _I64, _I64, _I32, _P, _P, _P, _P, _U32],
    # ctx, packed, n_floats, n_classes, x, labels, n_train, val_x, val_labels, n_val, epochs, batch, lr, perm,
    # drop_seed, patience, ckpt_period, packed_out, best_out, history, epochs_run, best_epoch
    'mmla_si_base_train': [_P, _P, _I64, _I32, _P, _P, _I64, _P, _P, _I64, _I32, _I32, ctypes.c_float, _P, _I64,
                           _I32, _I32, _P, _P, _P, _P, _P, _U32],
    # ctx, packed, n_floats, img_u8, labels, n, h, w, class_w, drop_mask, loss, grad, moving_out
    'mmla_od_loss_grad': [_P, _P, _I64, _P, _P, _I64, _I32, _I32, _P, _P, _P, _P, _P, _U32],
    # ctx, packed, n_floats, img_u8, labels, n_train, val_img, val_labels, n_val, h, w, class_w, epochs, batch,
    # lr, perm, drop_mask, patience, packed_out, history, epochs_run
    'mmla_od_finetune': [_P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I32, _I32, _P, _I32, _I32, _P, _P, _P, _I32,
                         _P, _P, _P, _U32],
    # ctx, img, n, h, w, src, levels, m, out
    'mmla_od_augment': [_P, _P, _I64, _I32, _I32, _P, _P, _I64, _P, _U32],
    # ctx, probs, labels, n, auc_out
    'mmla_od_auc': [_P, _P, _P, _I64, _P, _U32],
    # ctx, probs, labels, n, n_classes, auc_out
    'mmla_od_auc_k': [_P, _P, _P, _I64, _I32, _P, _U32],
    'mmla_od_classes': [_P, _P],
    'mmla_od_set_image_type': [_P, _I32],
    'mmla_od_image': [_P, _P, _P],
    # ctx, drop_seed, epoch, sample_ids, n, mask
    'mmla_od_drop_mask': [_P, _I64, _I32, _P, _I64, _P, _U32],
    # ctx, packed, n_floats, img_u8, labels, n_train, val_img, val_labels, n_val, h, w, class_w, epochs, batch,
    # lr, perm, drop_seed, patience, ckpt_period, packed_out, best_out, history, epochs_run, best_epoch
    'mmla_od_train': [_P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I32, _I32, _P, _I32, _I32, _P, _P, _I64, _I32,
                      _I32, _P, _P, _P, _P, _P, _U32],
    'mmla_od_pipeline': [_P, _P, _I64, _I64, _P, _I32, _P, _P, _P, _U32],
    'mmla_si_pipeline': [_P, _P, _I64, _I64, _P, _I32, _P, _P, _P, _U32],
    'mmla_ssim_u8': [_P, _P, _P, _I64, _I32, _I32, _I32, _P, _U32],
    # ctx, pool, pool_len, n_clips, n_layers, src_off, src_len, pos, then the outputs
    'mmla_od_mix': [_P, _P, _I64, _I64, _P, _P, _P, _P, _I32, _P, _I64, _P, _U32],
    'mmla_od_pipeline_mixed': [_P, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _U32],
    'mmla_od_pipeline_gated': [_P, _P, _I64, _I64, _P, _I32, _I32, ctypes.c_float, _P, _P, _P, _P,
                               _U32],
    'mmla_profile_enable': [_P, ctypes.c_int],
    'mmla_profile_read': [_P, _P, _P, _P, ctypes.c_int],
    'mmla_debug_od_trace': [_P, _P, _I64, ctypes.c_int, _P, _I64],
    'mmla_debug_si_trace': [_P, _P, _I64, ctypes.c_int, _P, _I64],
    'mmla_debug_ws_slot': [_P, ctypes.c_int, _P, _P],
    'mmla_debug_counters': [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)],
    'mmla_vad_reset': [_P, _I64, _I32],
    'mmla_vad_remove_silence': [_P, _P, _I64, _I64, _P, _I32, _I64, _P, _P, _P, _I32, _U32],
    'mmla_vad_collect': [_P, _P, _I64, _I64, _P, _I32, _P, _I32, _P, _P, _U32],
    'mmla_pcm16': [_P, _P, _I64, _P, _U32],
    'mmla_ratecv': [_P, _P, _I64, _I32, _I32, _I32, _P, _I64, _U32],
    'mmla_resample_sinc': [_P, _P, _I64, _I32, _I32, _P, _I64, _I32, _P, _I64, _U32],
}

NSTAGES = 7
STAGES = ('od_fe', 'si_fe', 'conv', 'lstm', 'glue', 'head', 'nr')

_lib = None
_lock = threading.Lock()


def load_library(path=LIB_PATH):
    """dlopen libmmla.so (raises OSError with a build hint if it is absent)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise OSError(f'{path} not found: build it with `make -C {os.path.join(_HERE, "csrc")}` '
                          f'or `python -c "import __graft_entry__ as g; g.build()"`')
        # PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64 (same sonames as
        # /opt/rocm's).  The first one loaded serves the whole process; torch cannot initialise on
        # /opt/rocm's newer runtime, while this library runs on torch's.  So when torch is present,
        # load it first: callers may then mix libmmla and torch device buffers in either order.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(path)
        for name, args in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int
        lib.mmla_last_error.argtypes = [_P]
        lib.mmla_last_error.restype = ctypes.c_char_p
        _lib = lib
        return lib


def crc32c(data):
    """CRC-32C of a bytes-like object (mmla_crc32c; host only, no device needed)."""
    lib = load_library()
    buf = np.frombuffer(memoryview(data).cast('B'), np.uint8)
    out = _U32()
    rc = lib.mmla_crc32c(buf.ctypes.data if buf.size else None, buf.size, ctypes.byref(out))
    if rc != MMLA_OK:
        raise MmlaError(f'mmla_crc32c: {_ERRORS.get(rc, rc)}', rc)
    return out.value


def png_unfilter(raw, h, row_bytes, bpp):
    """PNG scanline reconstruction (mmla_png_unfilter; host only, no device needed): the inflated
    IDAT bytes of h rows -> uint8 [h, row_bytes]."""
    lib = load_library()
    buf = np.frombuffer(memoryview(raw).cast('B'), np.uint8)
    if buf.size != h * (row_bytes + 1):
        raise ValueError(f'PNG image data holds {buf.size} bytes, expected {h} rows of '
                         f'{row_bytes + 1}')
    out = np.empty((h, row_bytes), np.uint8)
    rc = lib.mmla_png_unfilter(buf.ctypes.data if buf.size else None, h, row_bytes, bpp,
                               out.ctypes.data if out.size else None)
    if rc != MMLA_OK:
        raise ValueError('PNG image data: unknown scanline filter type')
    return out


def od_image_lut(image_type):
    """The colour map of the 'gray' or 'viridis' feature image as the library holds it (mmla_debug_od_image_lut; host
    only, no device needed) -> uint8 [256, 3]."""
    out = np.empty((256, 3), np.uint8)
    rc = load_library().mmla_debug_od_image_lut(od_image_type(image_type), out.ctypes.data)
    if rc != MMLA_OK:
        raise ValueError(f'image type {image_type!r} has no colour map')
    return out


class MixPlan(namedtuple('MixPlan', 'n_layers src_off src_len pos')):
    """The descriptors of a batch of layered mixes over one pool (mmla_od_mix): n_layers int32 [n] in
    1..MIX_MAX_LAYERS; src_off int64, src_len int32, pos int32, each [n, MIX_MAX_LAYERS].  Layer 0 of a clip
    is its canvas (at position 0), layer l reads src_len samples at pool[src_off] and lands at sample pos."""
    __slots__ = ()

    @classmethod
    def from_layers(cls, clips):
        """clips: per clip a list of (src_off, src_len, pos) layers, the canvas first"""
        n = len(clips)
        nl = np.array([len(c) for c in clips], np.int32)
        if n and (nl.min() < 1 or nl.max() > MIX_MAX_LAYERS):
            raise ValueError(f'a mix has 1..{MIX_MAX_LAYERS} layers, got {nl.min()}..{nl.max()}')
        off = np.zeros((n, MIX_MAX_LAYERS), np.int64)
        ln = np.zeros((n, MIX_MAX_LAYERS), np.int32)
        pos = np.zeros((n, MIX_MAX_LAYERS), np.int32)
        for i, c in enumerate(clips):
            for l, (o, m, p) in enumerate(c):
                off[i, l], ln[i, l], pos[i, l] = o, m, p
        return cls(nl, off, ln, pos)

    def arrays(self):
        """-> the four arrays contiguous in the ABI's types, shapes checked"""
        nl = np.ascontiguousarray(self.n_layers, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(self.src_off, dtype=np.int64)
        ln = np.ascontiguousarray(self.src_len, dtype=np.int32)
        pos = np.ascontiguousarray(self.pos, dtype=np.int32)
        for name, a in (('src_off', off), ('src_len', ln), ('pos', pos)):
            if a.shape != (nl.size, MIX_MAX_LAYERS):
                raise ValueError(f'{name} {a.shape}: expected [{nl.size}, {MIX_MAX_LAYERS}]')
        return nl, off, ln, pos


def _seed64(seed):
    """any Python integer's low 64 bits as the int64_t the ABI takes for a seed"""
    v = int(seed) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return a
    return a.ctypes.data


def _ns(nonstationary):
    """the flag bit of the conditioned calls' nonstationary= keyword"""
    return MMLA_NR_NONSTATIONARY if nonstationary else 0


class MmlaError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class Context:
    """One libmmla context = one HIP device + stream + workspaces + loaded weights.

    Host-array methods take/return numpy arrays (synchronous).  ``*_dev`` methods take raw device
    pointers (ints, e.g. ``torch_tensor.data_ptr()``) and only enqueue on the context stream.
    """

    def __init__(self, device=0):
        self.lib = load_library()
        h = _P()
        rc = self.lib.mmla_create(int(device), ctypes.byref(h))
        if rc != MMLA_OK:
            raise MmlaError(f'mmla_create(device={device}) failed: {_ERRORS.get(rc, rc)} '
                            '(no HIP device visible?)')
        self.h = h
        self.device = device
        self.od_classes = None
        self.od_channels = None      # channels of the loaded OD model's stem: 3, or 1 (imagetype='gray')
        self.od_image_type = None    # OD_IMG_* its pipelines make (od_set_image_type)
        self.si_classes = None

    def close(self):
        if getattr(self, 'h', None):
            self.lib.mmla_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != MMLA_OK:
            msg = self.lib.mmla_last_error(self.h)
            raise MmlaError(f'{what}: {_ERRORS.get(rc, rc)}: {msg.decode() if msg else ""}', rc)

    # -- configuration ------------------------------------------------------------------------
    def set_stream(self, stream_handle):
        self._check(self.lib.mmla_set_stream(self.h, stream_handle), 'mmla_set_stream')

    def synchronize(self):
        self._check(self.lib.mmla_synchronize(self.h), 'mmla_synchronize')

    def set_precision(self, mode):
        """PREC_F16X3 (default, 3xFP16 MFMA convs) or PREC_F32 (exact f32 MFMA convs)."""
        self._check(self.lib.mmla_set_precision(self.h, int(mode)), 'mmla_set_precision')

    def set_microbatch(self, od=0, si=0):
        self._check(self.lib.mmla_set_microbatch(self.h, int(od), int(si)), 'mmla_set_microbatch')

    def get_microbatch(self):
        """-> (od_clips, si_clips) per internal micro-batch for the next call."""
        od, si = _I64(), _I64()
        self._check(self.lib.mmla_get_microbatch(self.h, ctypes.byref(od), ctypes.byref(si)),
                    'mmla_get_microbatch')
        return od.value, si.value

    def release_workspace(self):
        self._check(self.lib.mmla_release_workspace(self.h), 'mmla_release_workspace')

    def range_check(self):
        """Wait for the stream; -> number of host-call micro-batches re-run in exact f32 so far.
        Raises MmlaError (code MMLA_E_RANGE) if a device-pointer call overflowed the fp16 range."""
        n = _I64()
        self._check(self.lib.mmla_range_check(self.h, ctypes.byref(n)), 'mmla_range_check')
        return n.value

    def debug_counters(self):
        """-> (host micro-batches re-run in exact f32, host micro-batches re-run on the unsplit
        BiLSTM after a split-BiLSTM timeout) so far"""
        a, b = _I64(), _I64()
        self._check(self.lib.mmla_debug_counters(self.h, ctypes.byref(a), ctypes.byref(b)),
                    'mmla_debug_counters')
        return a.value, b.value

    def profile_enable(self, on=True):
        self._check(self.lib.mmla_profile_enable(self.h, int(bool(on))), 'mmla_profile_enable')

    def profile_read(self, reset=True):
        """-> {stage: (device ms, launches, algorithmic work)} accumulated since the last reset."""
        ms = np.zeros(NSTAGES, np.float64)
        n = np.zeros(NSTAGES, np.int64)
        wk = np.zeros(NSTAGES, np.float64)
        self._check(self.lib.mmla_profile_read(self.h, _ptr(ms), _ptr(n), _ptr(wk), int(reset)),
                    'mmla_profile_read')
        return {s: (float(ms[i]), int(n[i]), float(wk[i])) for i, s in enumerate(STAGES)}

    def debug_od_trace(self, x, stage):
        """OD-NET intermediate tensor after `stage` (see mmla.h) for float NHWC input x."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        ch = self.od_channels or 3
        if x.shape[1:] != (OD_MELS, OD_FRAMES, ch):
            raise ValueError(f'debug_od_trace: images {x.shape}, the loaded model reads [n,{OD_MELS},{OD_FRAMES},{ch}]')
        shapes = {0: (128, 151, 16), 10: (19, 128), 11: (512,)}
        hw = [(64, 76, 32), (64, 76, 32), (64, 76, 32), (32, 38, 64), (32, 38, 64), (32, 38, 64),
              (16, 19, 128), (16, 19, 128), (16, 19, 128)]
        shape = shapes.get(stage) or hw[stage - 1]
        out = np.empty((n,) + shape, np.float32)
        self._check(self.lib.mmla_debug_od_trace(self.h, _ptr(x), n, int(stage), _ptr(out), out.size),
                    'mmla_debug_od_trace')
        return out

    def debug_si_trace(self, x, stage):
        """SI-NET intermediate tensor after `stage` (see mmla.h) for host features x [n, 256, 39]; a
        stage that the context's launches keep on chip raises MmlaError(MMLA_E_INVALID)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        shapes = {0: (256, 32), 10: (8, 128), 11: (512,), 12: (self.si_classes or 0,)}
        units = [(128, 32), (64, 64), (32, 128)]
        shape = shapes.get(stage) or units[(stage - 1) // 3 if 1 <= stage <= 9 else 0]   # else: the library refuses
        out = np.empty((n,) + shape, np.float32)
        self._check(self.lib.mmla_debug_si_trace(self.h, _ptr(x), n, int(stage), _ptr(out), out.size),
                    'mmla_debug_si_trace')
        return out

    def load_weights(self, kind, packed, n_classes, head=HEAD_SOFTMAX):
        packed = np.ascontiguousarray(packed, dtype=np.float32)
        self._check(self.lib.mmla_load_weights(self.h, int(kind), _ptr(packed), packed.size,
                                               int(n_classes), int(head)), 'mmla_load_weights')
        if kind == MODEL_OD:
            self.od_classes = int(n_classes)
            t, ch = ctypes.c_int32(), ctypes.c_int32()
            self._check(self.lib.mmla_od_image(self.h, ctypes.byref(t), ctypes.byref(ch)), 'mmla_od_image')
            self.od_image_type, self.od_channels = int(t.value), int(ch.value)   # the type resets on load
        else:
            self.si_classes = int(n_classes)

    # -- noise gate --------------------------------------------------------
    def nr_set_noise(self, noise, sr=16000):
        """Noise profile for reduce_noise(y_noise=noise, stationary=True): float32 samples."""
        a = np.ascontiguousarray(noise, dtype=np.float32).ravel()
        self._check(self.lib.mmla_nr_set_noise(self.h, _ptr(a), a.size, int(sr), 0),
                    'mmla_nr_set_noise')
        self._nr_key = None     # what noisereduce._set_noise / _set_noise_bank cached is replaced

    def nr_reduce(self, y):
        """Gate float32 signals y [n, len] (or [len]) with the current noise profile."""
        a = np.ascontiguousarray(y, dtype=np.float32)
        flat = a.ndim == 1
        if flat:
            a = a[None]
        out = np.empty_like(a)
        self._check(self.lib.mmla_nr_reduce(self.h, _ptr(a), a.shape[0], a.shape[1], a.shape[1],
                                            _ptr(out), 0), 'mmla_nr_reduce')
        return out[0] if flat else out

    def nr_reduce_dev(self, y, n, stride, length, out):
        self._check(self.lib.mmla_nr_reduce(self.h, y, n, stride, length, out, MMLA_DEVICE_PTR),
                    'mmla_nr_reduce(dev)')

    def nr_set_noise_bank(self, noises, sr=16000):
        """One noise profile per microphone, all from one launch sequence: `noises` is a list of
        float32 clips (their lengths may differ) or an array [P, len].  Replaces the bank (and the
        profile of nr_set_noise, which is a bank of one)."""
        if isinstance(noises, np.ndarray) and noises.ndim == 2:
            a = np.ascontiguousarray(noises, dtype=np.float32)
            ln = None
        else:
            clips = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in noises]
            a = np.zeros((len(clips), max([x.size for x in clips] + [1])), np.float32)
            ln = np.array([x.size for x in clips], np.int32)
            for i, x in enumerate(clips):
                a[i, :x.size] = x
        self._check(self.lib.mmla_nr_set_noise_bank(self.h, _ptr(a), a.shape[0], a.shape[1], _ptr(ln),
                                                    a.shape[1], int(sr), 0), 'mmla_nr_set_noise_bank')
        self.nr_bank_builds = getattr(self, 'nr_bank_builds', 0) + 1
        self._nr_key = None

    def nr_reduce_bank(self, y, profile=None):
        """nr_reduce with signal i gated against noise profile profile[i] of the bank (an int: every
        signal against that profile; None: profile 0)."""
        a = np.ascontiguousarray(y, dtype=np.float32)
        flat = a.ndim == 1
        if flat:
            a = a[None]
        pr = self._profile(profile, a.shape[0])
        out = np.empty_like(a)
        self._check(self.lib.mmla_nr_reduce_bank(self.h, _ptr(a), a.shape[0], a.shape[1], a.shape[1],
                                                 _ptr(pr), _ptr(out), 0), 'mmla_nr_reduce_bank')
        return out[0] if flat else out

    def nr_reduce_bank_dev(self, y, n, stride, length, out, profile=0):
        """profile: device int32 [n] (0: profile 0); indices outside the bank are clamped"""
        self._check(self.lib.mmla_nr_reduce_bank(self.h, y, n, stride, length, profile or None, out,
                                                 MMLA_DEVICE_PTR), 'mmla_nr_reduce_bank(dev)')

    def debug_nr_thresh(self):
        """-> float32 [P, 513]: the stationary gate's thresholds (dB) as the device holds them, one row
        per profile of the bank.  MmlaError without a bank."""
        n = _I64(0)
        rc = self.lib.mmla_debug_nr_thresh(self.h, None, 0, ctypes.byref(n))   # too small: the size only
        if n.value <= 0:
            self._check(rc, 'mmla_debug_nr_thresh')
        out = np.empty((n.value, 513), np.float32)
        self._check(self.lib.mmla_debug_nr_thresh(self.h, _ptr(out), out.size, ctypes.byref(n)),
                    'mmla_debug_nr_thresh')
        return out

    def nr_set_nonstationary(self, time_constant_s=2.0, thresh_n_mult=2.0, sigmoid_slope=10.0, sr=16000):
        """Parameters of the non-stationary gate (nr_reduce_ns, nonstationary=True); a context starts
        with these defaults."""
        self._check(self.lib.mmla_nr_set_nonstationary(self.h, float(time_constant_s), float(thresh_n_mult),
                                                       float(sigmoid_slope), int(sr)),
                    'mmla_nr_set_nonstationary')

    def nr_reduce_ns(self, y):
        """Gate float32 signals y [n, len] (or [len]) with the non-stationary gate: no noise profile."""
        a = np.ascontiguousarray(y, dtype=np.float32)
        flat = a.ndim == 1
        if flat:
            a = a[None]
        out = np.empty_like(a)
        self._check(self.lib.mmla_nr_reduce_ns(self.h, _ptr(a), a.shape[0], a.shape[1], a.shape[1],
                                               _ptr(out), 0), 'mmla_nr_reduce_ns')
        return out[0] if flat else out

    def nr_reduce_ns_dev(self, y, n, stride, length, out):
        self._check(self.lib.mmla_nr_reduce_ns(self.h, y, n, stride, length, out, MMLA_DEVICE_PTR),
                    'mmla_nr_reduce_ns(dev)')

    @staticmethod
    def _profile(profile, n):
        if profile is None:
            return None
        if np.ndim(profile) == 0:
            return np.full(n, int(profile), np.int32)
        pr = np.ascontiguousarray(profile, dtype=np.int32)
        if pr.shape != (n,):
            raise ValueError(f'profile {pr.shape}: expected one index per clip ({n})')
        return pr

    # -- silence removal -----------------------------------------------------
    def vad_reset(self, n_streams=1, mode=3):
        """n_streams fresh webrtcvad.Vad(mode) detectors (state kept in the context)."""
        self._check(self.lib.mmla_vad_reset(self.h, int(n_streams), int(mode)), 'mmla_vad_reset')
        self.vad_streams = int(n_streams)
        # whoever tagged the detector before (post-processing _vad_owner) no longer owns it
        self.vad_owner = None

    def vad_remove_silence(self, pcm, lens=None, items_per_stream=1):
        """save_wave_file(silence_remove=True) of every item: int16 [n, L] (or a list) ->
        (voiced PCM list of int16 arrays, per-frame speech flags list).  Items of one stream are
        consecutive and processed in order with that stream's detector state."""
        a, ln, L = self._pcm(pcm, lens)
        n = a.shape[0]
        nf = max(1, (a.shape[1] - 1) // 480) if a.shape[1] > 480 else 1
        out = np.empty_like(a)
        olen = np.empty(n, np.int32)
        sp = np.zeros((n, nf), np.uint8)
        self._check(self.lib.mmla_vad_remove_silence(
            self.h, _ptr(a), n, a.shape[1], _ptr(ln), L, int(items_per_stream), _ptr(out),
            _ptr(olen), _ptr(sp), nf, 0), 'mmla_vad_remove_silence')
        lens_in = ln if ln is not None else np.full(n, L, np.int32)
        nfr = [(int(m) - 1) // 480 if m > 480 else 0 for m in lens_in]
        return [out[i, :olen[i]].copy() for i in range(n)], [sp[i, :nfr[i]].astype(bool) for i in range(n)]

    def vad_collect(self, pcm, speech, lens=None):
        """the collector + rewrite alone on given per-frame decisions (list of bool arrays)"""
        a, ln, L = self._pcm(pcm, lens)
        n = a.shape[0]
        nf = max([1] + [len(s) for s in speech])
        sp = np.zeros((n, nf), np.uint8)
        for i, s in enumerate(speech):
            sp[i, :len(s)] = np.asarray(s, np.uint8)
        out = np.empty_like(a)
        olen = np.empty(n, np.int32)
        self._check(self.lib.mmla_vad_collect(self.h, _ptr(a), n, a.shape[1], _ptr(ln), L, _ptr(sp),
                                              nf, _ptr(out), _ptr(olen), 0), 'mmla_vad_collect')
        return [out[i, :olen[i]].copy() for i in range(n)]

    def pcm16(self, y):
        """float audio -> int16 as soundfile writes PCM_16"""
        a = np.ascontiguousarray(y, dtype=np.float32)
        out = np.empty(a.shape, np.int16)
        self._check(self.lib.mmla_pcm16(self.h, _ptr(a), a.size, _ptr(out), 0), 'mmla_pcm16')
        return out

    # -- rate conversion (offline pre-conditioning) ---------------------------------------------
    @staticmethod
    def ratecv_frames(n_frames, inrate, outrate):
        """output frames of audioop.ratecv(..., state=None) on n_frames input frames"""
        from math import gcd
        g = gcd(int(inrate), int(outrate))
        return (int(n_frames) - 1) * (int(outrate) // g) // (int(inrate) // g) + 1 if n_frames > 0 else 0

    def ratecv(self, pcm, nchannels, inrate, outrate):
        """audioop.ratecv(pcm, 2, nchannels, inrate, outrate, None)[0] (pydub set_frame_rate) on
        interleaved int16 frames -> int16 [out_frames * nchannels]"""
        a = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
        if a.size % nchannels:
            raise MmlaError(f'{a.size} samples are not whole frames of {nchannels} channels')
        nf = a.size // nchannels
        m = self.ratecv_frames(nf, inrate, outrate)
        out = np.empty(m * nchannels, np.int16)
        self._check(self.lib.mmla_ratecv(self.h, _ptr(a), nf, int(nchannels), int(inrate), int(outrate),
                                         _ptr(out), m, 0), 'mmla_ratecv')
        return out

    def resample_sinc(self, x, sr_orig, sr_new, half_window, num_table):
        """resampy.resample(x, sr_orig, sr_new, filter=(half_window, num_table)) on float32 mono"""
        a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        w = np.ascontiguousarray(half_window, dtype=np.float64)
        m = int(a.size * (float(sr_new) / sr_orig))
        out = np.empty(m, np.float32)
        self._check(self.lib.mmla_resample_sinc(self.h, _ptr(a), a.size, int(sr_orig), int(sr_new),
                                                _ptr(w), w.size, int(num_table), _ptr(out), m, 0),
                    'mmla_resample_sinc')
        return out

    # -- host-array API -----------------------------------------------------------------------
    @staticmethod
    def _pcm(pcm, lens):
        """-> (contiguous int16 [n, L], lens int32 [n] or None, clip_len)."""
        if isinstance(pcm, (list, tuple)):
            n = len(pcm)
            L = max([len(p) for p in pcm] + [1])
            buf = np.zeros((n, L), np.int16)
            ln = np.zeros(n, np.int32)
            for i, p in enumerate(pcm):
                buf[i, :len(p)] = np.asarray(p, np.int16)
                ln[i] = len(p)
            return buf, ln, L
        a = np.ascontiguousarray(pcm, dtype=np.int16)
        if a.ndim == 1:
            a = a[None]
        ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
        return a, ln, a.shape[1]

    @staticmethod
    def _float_pcm(pcm, lens):
        """float audio (librosa.load scale: any floating dtype, or a list of float arrays) ->
        (contiguous float32 [n, L], lens int32 [n] or None, clip_len); None for integer PCM"""
        if isinstance(pcm, (list, tuple)):
            if not any(np.issubdtype(np.asarray(p).dtype, np.floating) for p in pcm):
                return None
            n = len(pcm)
            L = max([len(p) for p in pcm] + [1])
            buf = np.zeros((n, L), np.float32)
            ln = np.zeros(n, np.int32)
            for i, p in enumerate(pcm):
                buf[i, :len(p)] = np.asarray(p, np.float32)
                ln[i] = len(p)
            return buf, ln, L
        a = np.asarray(pcm)
        if not np.issubdtype(a.dtype, np.floating):
            return None
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim == 1:
            a = a[None]
        ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
        return a, ln, a.shape[1]

    def od_set_image_type(self, image_type):
        """The image the pipelines make in front of the loaded OD model: 'zcr', 'gray' or 'viridis' (or
        OD_IMG_*).  A one-channel model takes 'gray' only; loading a model resets the type."""
        t = od_image_type(image_type)
        self._check(self.lib.mmla_od_set_image_type(self.h, t), 'mmla_od_set_image_type')
        self.od_image_type = t

    def od_features(self, pcm, lens=None, db=True, norm=True, zcr=True, img=True, image_type=None):
        """int16 PCM [n, L] (or a list of 1-D int16 arrays) -> dict of features.  Float audio
        (librosa.load scale, any floating dtype or a list of float arrays) goes through
        mmla_od_features_f32 instead.  image_type: 'zcr' (default), 'gray' or 'viridis' -- img is
        [n,128,151,3] for all three (gray as R = G = B)."""
        fl = self._float_pcm(pcm, lens)
        if fl is not None:
            a, ln, L = fl
            fn = self.lib.mmla_od_features_f32
        else:
            a, ln, L = self._pcm(pcm, lens)
            fn = self.lib.mmla_od_features
        n = a.shape[0]
        out = {}
        bufs = {}
        for key, want, shape, dt in (('db', db, (n, OD_MELS, OD_FRAMES), np.float32),
                                     ('norm', norm, (n, OD_MELS, OD_FRAMES), np.float32),
                                     ('zcr', zcr, (n, OD_FRAMES), np.float32),
                                     ('img', img, (n, OD_MELS, OD_FRAMES, 3), np.uint8)):
            bufs[key] = np.empty(shape, dt) if want else None
        self._check(fn(
            self.h, _ptr(a), n, a.shape[1], _ptr(ln), L, _ptr(bufs['db']), _ptr(bufs['norm']),
            _ptr(bufs['zcr']), _ptr(bufs['img']), _img_flags(image_type)), 'mmla_od_features')
        for k, v in bufs.items():
            if v is not None:
                out[k] = v
        return out

    def si_features(self, pcm, lens=None):
        a, ln, L = self._pcm(pcm, lens)
        n = a.shape[0]
        feat = np.empty((n, SI_FRAMES, SI_DIMS), np.float32)
        silent = np.empty(n, np.uint8)
        self._check(self.lib.mmla_si_features(self.h, _ptr(a), n, a.shape[1], _ptr(ln), L,
                                              _ptr(feat), _ptr(silent), 0), 'mmla_si_features')
        return feat, silent.astype(bool)

    def si_features_seq(self, sig):
        """Whole-signal features cut into 256-frame windows -> float32 [S, 256, 39]."""
        sig = np.ascontiguousarray(sig, dtype=np.int16).ravel()
        n = sig.size
        T = 1 if n <= 400 else 1 + -(-(n - 400) // 160)
        S = -(-T // SI_FRAMES)
        feat = np.empty((S, SI_FRAMES, SI_DIMS), np.float32)
        self._check(self.lib.mmla_si_features_seq(self.h, _ptr(sig), n, S, _ptr(feat), 0),
                    'mmla_si_features_seq')
        return feat

    def si_features_seq_batch(self, pcm, lens=None):
        """si_features_seq of a ragged batch in one launch: int16 [n, L] with lens (or a list of
        signals) -> (float32 [n, w_max, 256, 39], n_windows int32 [n]); w_max = si_seq_windows(L).
        Window w < n_windows[i] is what si_features_seq gives for signal i alone, every other zeros."""
        a, ln, L = self._pcm(pcm, lens)
        n = a.shape[0]
        feat = np.empty((n, si_seq_windows(L), SI_FRAMES, SI_DIMS), np.float32)
        nw = np.empty(n, np.int32)
        self._check(self.lib.mmla_si_features_seq_batch(self.h, _ptr(a), n, a.shape[1], _ptr(ln), L,
                                                        _ptr(feat), _ptr(nw), 0),
                    'mmla_si_features_seq_batch')
        return feat, nw

    def si_enrol_embed(self, pcm, lens=None, profile=None, passes=1, silence_remove=True, vad_mode=3,
                       nonstationary=False, return_pcm=False):
        """Registration recordings int16 [n, L] (or a list; L up to ENROL_MAX_SAMPLES) -> (emb float32
        [n, w_max, 512], n_windows [n], kept_len [n][, conditioned int16 [n, L]]): condition() with one
        fresh temporary detector of mode vad_mode per recording (the vad_reset detectors are left
        alone), si_features_seq_batch of the conditioned recordings, si_embed of every window.  Rows of
        emb at or past n_windows[i] carry no meaning."""
        a, ln, L = self._pcm(pcm, lens)
        n = a.shape[0]
        pr = self._profile(profile, n)
        emb = np.empty((n, si_seq_windows(L), SI_EMBED), np.float32)
        nw = np.empty(n, np.int32)
        kept = np.empty(n, np.int32)
        out = np.empty((n, L), np.int16) if return_pcm else None
        self._check(self.lib.mmla_si_enrol_embed(
            self.h, _ptr(a), n, a.shape[1], _ptr(ln), L, _ptr(pr), int(passes), int(bool(silence_remove)),
            int(vad_mode), _ptr(out), _ptr(kept), _ptr(nw), _ptr(emb), _ns(nonstationary)),
            'mmla_si_enrol_embed')
        return (emb, nw, kept, out) if return_pcm else (emb, nw, kept)

    def si_set_head(self, w, b, head=HEAD_SIGMOID):
        """Replace the Dense head of the loaded SI model in place: w [512, K], b [K] (host arrays)."""
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if w.ndim != 2 or w.shape[0] != SI_EMBED or b.shape != (w.shape[1],):
            raise ValueError(f'w {w.shape} / b {b.shape}: expected [512,K] and [K]')
        k = w.shape[1]
        self._check(self.lib.mmla_si_set_head(self.h, _ptr(w) if k else None, _ptr(b) if k else None, k,
                                              int(head)), 'mmla_si_set_head')
        self.si_classes = int(k)

    def _od_k(self):
        """the classes of the loaded OD model (2 before one is loaded: the library refuses the call)"""
        return self.od_classes or 2

    def od_forward(self, x):
        """x [n,128,151,C], C = od_channels of the loaded model (uint8, or float 0..255) -> probs [n,K],
        K = od_classes"""
        x = np.ascontiguousarray(x)
        n = x.shape[0]
        ch = self.od_channels or 3
        # the library reads n * 128 * 151 * C values: an array of another shape never reaches it
        if x.ndim != 4 or x.shape[1:] != (OD_MELS, OD_FRAMES, ch):
            raise ValueError(f'od_forward: images {x.shape}, the loaded model reads [n,{OD_MELS},{OD_FRAMES},{ch}]')
        probs = np.empty((n, self._od_k()), np.float32)
        if x.dtype == np.uint8:
            rc = self.lib.mmla_od_forward_u8(self.h, _ptr(x), n, _ptr(probs), 0)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            rc = self.lib.mmla_od_forward(self.h, _ptr(x), n, _ptr(probs), 0)
        self._check(rc, 'mmla_od_forward')
        return probs

    def si_forward(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        probs = np.empty((n, self.si_classes or 0), np.float32)
        self._check(self.lib.mmla_si_forward(self.h, _ptr(x), n, _ptr(probs), 0), 'mmla_si_forward')
        return probs

    def si_embed(self, x):
        """SI-NET up to the BiLSTM output (base_model.layers[-2].output): [n,256,39] -> float32
        [n,512].  Whatever head is loaded does not enter the result."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        emb = np.empty((n, SI_EMBED), np.float32)
        self._check(self.lib.mmla_si_embed(self.h, _ptr(x), n, _ptr(emb), 0), 'mmla_si_embed')
        return emb

    def si_head_fit(self, emb, labels, val_emb, val_labels, w0, b0, perm, epochs, batch=16, lr=1e-4):
        """Fit R sigmoid heads side by side in one launch (mmla_si_head_fit).  emb [n,512], labels
        [n] ints; val_* likewise (None or empty: no validation set); w0 [R,512,K], b0 [R,K]; perm
        [R,epochs,n].  -> (w [R,512,K], b [R,K], history [R,epochs,4] = loss, acc, val_loss, val_acc)"""
        emb = np.ascontiguousarray(emb, dtype=np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        w0 = np.ascontiguousarray(w0, dtype=np.float32)
        b0 = np.ascontiguousarray(b0, dtype=np.float32)
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        if w0.ndim != 3 or w0.shape[1] != SI_EMBED or b0.shape != (w0.shape[0], w0.shape[2]):
            raise ValueError(f'w0 {w0.shape} / b0 {b0.shape}: expected [R,512,K] and [R,K]')
        R, _, K = w0.shape
        n = labels.shape[0]
        if emb.shape != (n, SI_EMBED):
            raise ValueError(f'emb {emb.shape}: expected [{n},512]')
        if perm.shape != (R, int(epochs), n):
            raise ValueError(f'perm {perm.shape}: expected [{R},{int(epochs)},{n}]')
        nv = 0 if val_labels is None else len(val_labels)
        ve = vl = None
        if nv:
            ve = np.ascontiguousarray(val_emb, dtype=np.float32)
            vl = np.ascontiguousarray(val_labels, dtype=np.int32)
            if ve.shape != (nv, SI_EMBED):
                raise ValueError(f'val_emb {ve.shape}: expected [{nv},512]')
        w = np.empty_like(w0)
        b = np.empty_like(b0)
        hist = np.empty((R, int(epochs), 4), np.float32)
        self._check(self.lib.mmla_si_head_fit(
            self.h, _ptr(emb), _ptr(labels), n, _ptr(ve), _ptr(vl), nv, K, R, int(epochs), int(batch),
            float(lr), _ptr(w0), _ptr(b0), _ptr(perm), _ptr(w), _ptr(b), _ptr(hist), 0),
            'mmla_si_head_fit')
        return w, b, hist

    @staticmethod
    def _si_windows(x, labels, what):
        x = np.ascontiguousarray(x, dtype=np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if x.ndim != 3 or x.shape[1:] != (256, 39) or labels.shape != (x.shape[0],):
            raise ValueError(f'{what} {x.shape} / labels {labels.shape}: expected [n,256,39] and [n]')
        return x, labels

    @staticmethod
    def _fit_args(perm, epochs, n, val_x, val_labels, prep, what='val_x', trim=False):
        """What the fit wrappers prepare alike: perm as int32 [epochs, n] (trim: rows past epochs dropped), the
        optional validation set through prep(val_x, val_labels, what).  -> (epochs, perm, vx, vl, nv, opt);
        opt(a) is a's pointer, or None in a zero-epoch call, which must not read it."""
        epochs = int(epochs)
        perm = np.ascontiguousarray(perm, dtype=np.int32).reshape(-1, n) if epochs else np.zeros((0, n), np.int32)
        if trim:
            perm = np.ascontiguousarray(perm[:epochs])
        if perm.shape != (epochs, n):
            raise ValueError(f'perm {perm.shape}: expected [{epochs},{n}]')
        nv = 0 if val_labels is None else len(val_labels)
        vx = vl = None
        if nv:
            vx, vl = prep(val_x, val_labels, what)
        return epochs, perm, vx, vl, nv, (_ptr if epochs else lambda a: None)

    def _si_grad_args(self, packed, x, labels):
        """-> (packed flat float32, x, labels, loss [2], grad like packed) of the two SI loss-grad wrappers"""
        packed = np.ascontiguousarray(packed, dtype=np.float32).ravel()
        x, labels = self._si_windows(x, labels, 'x')
        return packed, x, labels, np.empty(2, np.float32), np.empty_like(packed)

    def si_loss_grad(self, packed, n_classes, x, labels):
        """The stage-2 loss of ONE batch and its gradient (mmla_si_loss_grad): packed = the SI blob of
        weights.pack with an n_classes-way head, x [n,256,39], labels [n] -> (loss float32 [2] = data
        term, L2 penalty; grad float32 [n_floats] in the packed order, 0 in the moving statistics)."""
        packed, x, labels, loss, grad = self._si_grad_args(packed, x, labels)
        self._check(self.lib.mmla_si_loss_grad(self.h, _ptr(packed), packed.size, int(n_classes), _ptr(x),
                                               _ptr(labels), x.shape[0], _ptr(loss), _ptr(grad), 0),
                    'mmla_si_loss_grad')
        return loss, grad

    def si_finetune(self, packed, n_classes, x, labels, val_x, val_labels, perm, epochs, batch=8, lr=1e-6):
        """Stage 2 of a registration (mmla_si_finetune): RMSprop through the whole SI network from the
        blob `packed`.  x [n,256,39], labels [n]; val_* likewise (None or empty: no validation set);
        perm [epochs,n] the sample order of every epoch.  -> (packed_out float32 [n_floats], history
        [epochs,4] = loss, acc, val_loss, val_acc)."""
        packed = np.ascontiguousarray(packed, dtype=np.float32).ravel()
        x, labels = self._si_windows(x, labels, 'x')
        n = x.shape[0]
        epochs, perm, vx, vl, nv, opt = self._fit_args(perm, epochs, n, val_x, val_labels, self._si_windows)
        out = np.empty_like(packed)
        hist = np.empty((epochs, 4), np.float32)
        self._check(self.lib.mmla_si_finetune(
            self.h, _ptr(packed), packed.size, int(n_classes), _ptr(x), _ptr(labels), n, _ptr(vx), _ptr(vl),
            nv, epochs, int(batch), float(lr), opt(perm), _ptr(out), opt(hist), 0), 'mmla_si_finetune')
        return out, hist

    def si_base_drop_mask(self, drop_seed, epoch, sample_ids, n=None):
        """The dropout keep-bits of a base-model fit as bytes (mmla_si_base_drop_mask): sample_ids [n]
        (None: 0..n-1) -> (mask_a uint8 [n,32,128] in front of the avg-pool, mask_b uint8 [n,512] on the
        embedding); 1 = kept."""
        ids = None
        if sample_ids is not None:
            ids = np.ascontiguousarray(sample_ids, dtype=np.int32).ravel()
            n = ids.size
        n = int(n)
        mask_a = np.empty((max(n, 0), 32, 128), np.uint8)
        mask_b = np.empty((max(n, 0), 512), np.uint8)
        self._check(self.lib.mmla_si_base_drop_mask(self.h, _seed64(drop_seed), int(epoch), _ptr(ids), n,
                                                    _ptr(mask_a), _ptr(mask_b), 0), 'mmla_si_base_drop_mask')
        return mask_a, mask_b

    def si_base_loss_grad(self, packed, n_classes, x, labels, drop_seed=0, epoch=0, sample_ids=None,
                          moving=False):
        """The training-mode loss of ONE batch of SI base-model training and its gradient
        (mmla_si_base_loss_grad): BatchNorm on batch statistics, both dropouts (keep-bits of drop_seed,
        epoch, sample_ids), the softmax head's loss on the logits.  -> (loss float32 [2] = data term, L2
        penalty; grad float32 [n_floats], 0 in the moving statistics) and, with moving=True, the blob with
        only its moving statistics advanced one step."""
        packed, x, labels, loss, grad = self._si_grad_args(packed, x, labels)
        ids = None
        if sample_ids is not None:
            ids = np.ascontiguousarray(sample_ids, dtype=np.int32).ravel()
            if ids.shape != labels.shape:
                raise ValueError(f'sample_ids {ids.shape}: expected {labels.shape}')
        mov = np.empty_like(packed) if moving else None
        self._check(self.lib.mmla_si_base_loss_grad(
            self.h, _ptr(packed), packed.size, int(n_classes), _ptr(x), _ptr(labels), x.shape[0], _seed64(drop_seed),
            int(epoch), _ptr(ids), _ptr(loss), _ptr(grad), _ptr(mov), 0), 'mmla_si_base_loss_grad')
        return (loss, grad, mov) if moving else (loss, grad)

    def si_base_train(self, packed, n_classes, x, labels, val_x, val_labels, perm, epochs, batch=32, lr=1e-4,
                      drop_seed=0, patience=0, ckpt_period=0):
        """The reference's train() on the device (mmla_si_base_train): RMSprop through the whole SI network
        in training mode from the blob `packed`.  x [n,256,39], labels [n]; val_* likewise (None or empty:
        no validation set); perm [epochs,n].  -> (packed_out, best float32 [n_floats] or None, history
        [epochs,4] = loss, categorical_accuracy, val_loss, val_categorical_accuracy with NaN rows after an
        early stop, epochs_run, best_epoch or -1)."""
        packed = np.ascontiguousarray(packed, dtype=np.float32).ravel()
        x, labels = self._si_windows(x, labels, 'x')
        n = x.shape[0]
        epochs, perm, vx, vl, nv, opt = self._fit_args(perm, epochs, n, val_x, val_labels, self._si_windows)
        out = np.empty_like(packed)
        best = np.empty_like(packed)
        hist = np.empty((epochs, 4), np.float32)
        ran = np.zeros(1, np.int32)
        best_ep = np.full(1, -1, np.int32)
        self._check(self.lib.mmla_si_base_train(
            self.h, _ptr(packed), packed.size, int(n_classes), _ptr(x), _ptr(labels), n, _ptr(vx), _ptr(vl), nv,
            epochs, int(batch), float(lr), opt(perm), _seed64(drop_seed), int(patience), int(ckpt_period),
            _ptr(out), _ptr(best), opt(hist), _ptr(ran), _ptr(best_ep), 0), 'mmla_si_base_train')
        return out, (best if best_ep[0] >= 0 else None), hist, int(ran[0]), int(best_ep[0])

    @staticmethod
    def _od_images(img, labels, what):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if img.ndim != 4 or img.shape[3] not in weights.OD_CHANNELS or labels.shape != (img.shape[0],):
            raise ValueError(f'{what} {img.shape} / labels {labels.shape}: expected [n,h,w,C] (C = 3 or 1) and [n]')
        return img, labels

    @staticmethod
    def _od_blob_channels(packed, img):
        """the images' channels must be the blob's (weights.od_layout_of): the library reads h w C bytes per image"""
        ch = weights.od_layout_of(packed.size)[1]
        if img.shape[3] != ch:
            raise ValueError(f'img {img.shape}: the blob of {packed.size} floats has a {ch}-channel stem')

    @staticmethod
    def _od_class_w(class_w, n_floats):
        """class_w as float32 [K], K read from the blob's size (None: ones)"""
        k = weights.od_layout_of(n_floats)[0]
        if class_w is None:
            return np.ones(k, np.float32)
        return np.ascontiguousarray(class_w, dtype=np.float32).reshape(k)

    def od_loss_grad(self, packed, img, labels, class_w=None, drop_mask=None, moving=False):
        """The training-mode loss of ONE batch of OD feature images and its gradient (mmla_od_loss_grad):
        packed = the OD blob of weights.pack (any K; C = 3 or 1 channels), img uint8 [n,h,w,C], labels [n] in [0,K), class_w [K]
        (None: ones), drop_mask uint8
        [n,512] (None: every unit kept) -> (loss float32 [1], grad float32 [n_floats] in the packed order, 0
        in the moving statistics[, the blob with only the moving statistics advanced one step])."""
        packed = np.ascontiguousarray(packed, dtype=np.float32).ravel()
        img, labels = self._od_images(img, labels, 'img')
        self._od_blob_channels(packed, img)
        n, h, w = img.shape[:3]
        cw = self._od_class_w(class_w, packed.size)
        if drop_mask is not None:
            drop_mask = np.ascontiguousarray(drop_mask, dtype=np.uint8)
            if drop_mask.shape != (n, OD_DROP_UNITS):
                raise ValueError(f'drop_mask {drop_mask.shape}: expected [{n},{OD_DROP_UNITS}]')
        loss = np.empty(1, np.float32)
        grad = np.empty_like(packed)
        mov = np.empty_like(packed) if moving else None
        self._check(self.lib.mmla_od_loss_grad(self.h, _ptr(packed), packed.size, _ptr(img), _ptr(labels), n, h, w,
                                               _ptr(cw), _ptr(drop_mask), _ptr(loss), _ptr(grad), _ptr(mov), 0),
                    'mmla_od_loss_grad')
        return (loss, grad, mov) if moving else (loss, grad)

    def od_finetune(self, packed, img, labels, val_img, val_labels, class_w, lr, perm, drop_mask, epochs,
                    batch=16, patience=0):
        """OverlapDetector.continue_train_model on the device (mmla_od_finetune): Adadelta through the whole
        OD network from the blob `packed`, BatchNorm on batch statistics.  img uint8 [n,h,w,C] with the blob's C
        (3, or 1 for a one-channel stem; the blob coming out has the same layout), labels [n];
        val_* likewise (None or empty: no validation set); lr [epochs]; perm [epochs,n] the sample order
        of every epoch; drop_mask uint8 [epochs,n,512] indexed by sample (None: every unit kept).
        -> (packed_out float32 [n_floats], history [epochs,5] = loss, acc, val_loss, val_acc, lr (NaN rows
        after an early stop), epochs_run)."""
        packed = np.ascontiguousarray(packed, dtype=np.float32).ravel()
        img, labels = self._od_images(img, labels, 'img')
        self._od_blob_channels(packed, img)
        n, h, w = img.shape[:3]
        epochs, perm, vi, vl, nv, opt = self._fit_args(perm, epochs, n, val_img, val_labels, self._od_images, 'val_img',
                                                        trim=True)
        cw = self._od_class_w(class_w, packed.size)
        lr = np.ascontiguousarray(lr, dtype=np.float32).ravel()[:epochs]
        if lr.shape != (epochs,):
            raise ValueError(f'lr {lr.shape}: expected [{epochs}]')
        if drop_mask is not None:
            drop_mask = np.ascontiguousarray(np.asarray(drop_mask, dtype=np.uint8)[:epochs])
            if drop_mask.shape != (epochs, n, OD_DROP_UNITS):
                raise ValueError(f'drop_mask {drop_mask.shape}: expected [{epochs},{n},{OD_DROP_UNITS}]')
        if nv and vi.shape[1:] != img.shape[1:]:
            raise ValueError(f'val_img {vi.shape}: expected [n,{h},{w},{img.shape[3]}]')
        out = np.empty_like(packed)
        hist = np.empty((epochs, 5), np.float32)
        ran = np.zeros(1, np.int32)
        self._check(self.lib.mmla_od_finetune(
            self.h, _ptr(packed), packed.size, _ptr(img), _ptr(labels), n, _ptr(vi), _ptr(vl), nv, h, w, _ptr(cw),
            epochs, int(batch), opt(lr), opt(perm), opt(drop_mask), int(patience), _ptr(out), opt(hist), _ptr(ran), 0),
            'mmla_od_finetune')
        return out, hist, int(ran[0])

    def od_train(self, packed, img, labels, val_img, val_labels, class_w, lr, perm, epochs, batch=16, drop_seed=0,
                 patience=0, ckpt_period=0):
        """OverlapDetector.train_model's fit on the device (mmla_od_train): od_finetune's arguments with the
        dropout keep-bits generated on the device from drop_seed and ModelCheckpoint(val_acc, 'max',
        ckpt_period).  -> (packed_out, best float32 [n_floats] or None, history [epochs,7] = loss, acc,
        val_loss, val_acc, lr, auc, val_auc (NaN rows after an early stop), epochs_run, best_epoch or -1)."""
        packed = np.ascontiguousarray(packed, dtype=np.float32).ravel()
        img, labels = self._od_images(img, labels, 'img')
        self._od_blob_channels(packed, img)
        n, h, w = img.shape[:3]
        epochs, perm, vi, vl, nv, opt = self._fit_args(perm, epochs, n, val_img, val_labels, self._od_images, 'val_img',
                                                        trim=True)
        cw = self._od_class_w(class_w, packed.size)
        lr = np.ascontiguousarray(lr, dtype=np.float32).ravel()[:epochs]
        if lr.shape != (epochs,):
            raise ValueError(f'lr {lr.shape}: expected [{epochs}]')
        if nv and vi.shape[1:] != img.shape[1:]:
            raise ValueError(f'val_img {vi.shape}: expected [n,{h},{w},{img.shape[3]}]')
        out = np.empty_like(packed)
        best = np.empty_like(packed)
        hist = np.empty((epochs, 7), np.float32)
        ran = np.zeros(1, np.int32)
        best_ep = np.full(1, -1, np.int32)
        self._check(self.lib.mmla_od_train(
            self.h, _ptr(packed), packed.size, _ptr(img), _ptr(labels), n, _ptr(vi), _ptr(vl), nv, h, w, _ptr(cw),
            epochs, int(batch), opt(lr), opt(perm), _seed64(drop_seed), int(patience), int(ckpt_period), _ptr(out),
            _ptr(best), opt(hist), _ptr(ran), _ptr(best_ep), 0), 'mmla_od_train')
        return out, (best if best_ep[0] >= 0 else None), hist, int(ran[0]), int(best_ep[0])

    def od_drop_mask(self, drop_seed, epoch, sample_ids, n=None):
        """The dropout keep-bits of an mmla_od_train fit as bytes (mmla_od_drop_mask): sample_ids [n] (None:
        0..n-1) -> uint8 [n,512] on the embedding; 1 = kept."""
        ids = None
        if sample_ids is not None:
            ids = np.ascontiguousarray(sample_ids, dtype=np.int32).ravel()
            n = ids.size
        n = int(n)
        mask = np.empty((max(n, 0), OD_DROP_UNITS), np.uint8)
        self._check(self.lib.mmla_od_drop_mask(self.h, _seed64(drop_seed), int(epoch), _ptr(ids), n, _ptr(mask), 0),
                    'mmla_od_drop_mask')
        return mask

    def od_augment(self, img, src, levels):
        """The pyramid blur of augment_images (mmla_od_augment): img uint8 [n,h,w,3] (h even in [8,128], w odd
        in [9,151]), src [m] rows of img, levels [m] in [0, 8] -> uint8 [m,h,w,3]; out[k] = img[src[k]] after
        levels[k] rounds of pyrDown + pyrUp, cropped once."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim != 4 or img.shape[3] != 3:
            raise ValueError(f'img {img.shape}: expected [n,h,w,3]')
        src = np.ascontiguousarray(src, dtype=np.int32).ravel()
        levels = np.ascontiguousarray(levels, dtype=np.int32).ravel()
        if src.shape != levels.shape:
            raise ValueError(f'src {src.shape} / levels {levels.shape}: expected one level per source row')
        n, h, w = img.shape[:3]
        out = np.empty((src.size, h, w, 3), np.uint8)
        self._check(self.lib.mmla_od_augment(self.h, _ptr(img), n, h, w, _ptr(src), _ptr(levels), src.size, _ptr(out),
                                             0), 'mmla_od_augment')
        return out

    def od_auc(self, probs, labels):
        """tf.keras.metrics.AUC() at its defaults (mmla_od_auc_k) of probs float32 [n,K] against labels [n] in
        [0,K) -> float32 scalar."""
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
        if probs.ndim != 2 or probs.shape[0] != labels.size:
            raise ValueError(f'probs {probs.shape} / labels {labels.shape}: expected [n,K] and [n]')
        out = np.empty(1, np.float32)
        self._check(self.lib.mmla_od_auc_k(self.h, _ptr(probs), _ptr(labels), labels.size, probs.shape[1], _ptr(out),
                                           0), 'mmla_od_auc_k')
        return out[0]

    def od_pipeline(self, pcm, lens=None):
        """-> (probs [n,K], argmax [n] (-1 = 'silent'), silent [n] bool)."""
        a, ln, L = self._pcm(pcm, lens)
        n = a.shape[0]
        probs = np.empty((n, self._od_k()), np.float32)
        am = np.empty(n, np.int32)
        silent = np.empty(n, np.uint8)
        self._check(self.lib.mmla_od_pipeline(self.h, _ptr(a), n, a.shape[1], _ptr(ln), L,
                                              _ptr(probs), _ptr(am), _ptr(silent), 0),
                    'mmla_od_pipeline')
        return probs, am, silent.astype(bool)

    def od_pipeline_gated(self, pcm, lens=None, passes=4, threshold=0.3, nonstationary=False):
        """od_pipeline with the denoise-and-compare silence gate of record_on_pi.py:103-124 (noise
        profile: nr_set_noise; nonstationary=True: the gate of nr_reduce_ns, no profile) -> (probs [n,K]
        of the denoised clips, argmax [n] (-1 = 'silent'), silent [n] bool, ssim [n] of each clip's
        image against its `passes` x denoised image)."""
        a, ln, L = self._pcm(pcm, lens)
        n = a.shape[0]
        probs = np.empty((n, self._od_k()), np.float32)
        am = np.empty(n, np.int32)
        silent = np.empty(n, np.uint8)
        ssim = np.empty(n, np.float32)
        self._check(self.lib.mmla_od_pipeline_gated(
            self.h, _ptr(a), n, a.shape[1], _ptr(ln), L, int(passes), float(threshold), _ptr(probs),
            _ptr(am), _ptr(silent), _ptr(ssim), _ns(nonstationary)), 'mmla_od_pipeline_gated')
        return probs, am, silent.astype(bool), ssim

    # -- overlap synthesis: layered mixes over one pool of recordings ------------------------------
    def od_mix(self, pool, plan, clip_len=OD_CLIP):
        """pydub's overlay chain (audioop.add per layer, clamped, in order) for every clip of `plan` (a
        MixPlan) over the int16 `pool` -> (clips int16 [n, clip_len], zeros behind each clip's canvas;
        out_len int32 [n] = the canvas length)."""
        pool = np.ascontiguousarray(pool, dtype=np.int16).reshape(-1)
        nl, off, ln, pos = MixPlan(*plan).arrays()
        n = nl.size
        out = np.empty((n, int(clip_len)), np.int16)
        olen = np.empty(n, np.int32)
        hold = np.zeros(1, np.int16)       # a non-null pool for an empty one
        self._check(self.lib.mmla_od_mix(self.h, _ptr(pool if pool.size else hold), pool.size, n, _ptr(nl),
                                         _ptr(off), _ptr(ln), _ptr(pos), int(clip_len), _ptr(out),
                                         int(clip_len), _ptr(olen), 0), 'mmla_od_mix')
        return out, olen

    def od_mix_dev(self, pool, pool_len, n, n_layers, src_off, src_len, pos, out, out_stride,
                   clip_len=OD_CLIP, out_len=0):
        """device plans are not checked: the kernel reads inside the pool only (see mmla.h)"""
        self._check(self.lib.mmla_od_mix(self.h, pool, pool_len, n, n_layers, src_off, src_len, pos,
                                         int(clip_len), out, out_stride, out_len or None, MMLA_DEVICE_PTR),
                    'mmla_od_mix(dev)')

    def od_pipeline_mixed(self, pool, plan):
        """od_mix at 24000 samples fused in front of od_pipeline, the mixed clips staying on the device ->
        (probs [n,K], argmax [n] (-1 = 'silent': a canvas below 4000 samples), silent [n] bool); the bits of
        od_pipeline(*od_mix(pool, plan))."""
        pool = np.ascontiguousarray(pool, dtype=np.int16).reshape(-1)
        nl, off, ln, pos = MixPlan(*plan).arrays()
        n = nl.size
        probs = np.empty((n, self._od_k()), np.float32)
        am = np.empty(n, np.int32)
        silent = np.empty(n, np.uint8)
        hold = np.zeros(1, np.int16)
        self._check(self.lib.mmla_od_pipeline_mixed(
            self.h, _ptr(pool if pool.size else hold), pool.size, n, _ptr(nl), _ptr(off), _ptr(ln), _ptr(pos),
            _ptr(probs), _ptr(am), _ptr(silent), 0), 'mmla_od_pipeline_mixed')
        return probs, am, silent.astype(bool)

    def od_pipeline_mixed_dev(self, pool, pool_len, n, n_layers, src_off, src_len, pos, probs=0, argmax=0,
                              silent=0):
        self._check(self.lib.mmla_od_pipeline_mixed(
            self.h, pool, pool_len, n, n_layers, src_off, src_len, pos, probs or None, argmax or None,
            silent or None, MMLA_DEVICE_PTR), 'mmla_od_pipeline_mixed(dev)')

    # -- the PC loops' pre-conditioning (noise gate + silence removal) in front of the networks ---
    def _fused(self, name, n_classes, clips, profile, passes, silence_remove, items_per_stream, return_pcm,
               nonstationary):
        """The shared body of condition and the {od,si,room}_pipeline_{conditioned,capture} calls.
        clips: (int16 [n, stride], lens or frames, clip_len or clip_frames, row width of the conditioned
        clips); n_classes: one width per network, () for the conditioning alone."""
        a, ln, L, width = clips
        n = a.shape[0]
        pr = self._profile(profile, n)
        out = np.empty((n, width), np.int16) if return_pcm else None
        kept = np.empty(n, np.int32)
        nets = []
        for k in n_classes:
            nets += [np.empty((n, k), np.float32), np.empty(n, np.int32)]
        silent = np.empty(n, np.uint8)
        tail = nets + [silent] if n_classes else []
        self._fused_call(name, False, _ptr(a), n, a.shape[1], _ptr(ln), L, passes, silence_remove,
                         items_per_stream, [_ptr(x) for x in tail], _ptr(out), _ptr(kept), _ptr(pr), nonstationary)
        if not n_classes:
            return out, kept
        res = tuple(nets) + (silent.astype(bool), kept)
        return res + (out,) if return_pcm else res

    def _cond_clips(self, pcm, lens):
        a, ln, L = self._pcm(pcm, lens)
        return a, ln, L, a.shape[1]

    def condition(self, pcm, lens=None, profile=None, passes=1, silence_remove=True,
                  items_per_stream=1, nonstationary=False):
        """The batched save_wave_file(noise_reduce=True, silence_remove=...) of record_on_pc.py: int16
        [n, L] (or a list) -> (conditioned int16 [n, L], zeros behind each clip's kept samples; kept_len
        [n]).  Clip c is gated `passes` times against noise profile profile[c] (nr_set_noise_bank; None:
        profile 0; nonstationary=True: the gate of nr_reduce_ns, no bank, profile ignored); silence removal runs on the vad_reset detectors, stream s owning clips
        [s * items_per_stream, (s + 1) * items_per_stream), and their state persists across calls."""
        return self._fused('mmla_condition', (), self._cond_clips(pcm, lens), profile, passes, silence_remove,
                           items_per_stream, True, nonstationary)

    def od_pipeline_conditioned(self, pcm, lens=None, profile=None, passes=1, silence_remove=True,
                                items_per_stream=1, return_pcm=False, nonstationary=False):
        """condition() fused in front of od_pipeline -> (probs [n,K], argmax [n] (-1 = 'silent': fewer
        than 4000 samples kept), silent [n] bool, kept_len [n]); return_pcm adds the conditioned clips."""
        return self._fused('mmla_od_pipeline_conditioned', (self._od_k(),), self._cond_clips(pcm, lens), profile,
                           passes, silence_remove, items_per_stream, return_pcm, nonstationary)

    def si_pipeline_conditioned(self, pcm, lens=None, profile=None, passes=1, silence_remove=True,
                                items_per_stream=1, return_pcm=False, nonstationary=False):
        """condition() fused in front of si_pipeline -> (probs [n,K], argmax, silent, kept_len)"""
        return self._fused('mmla_si_pipeline_conditioned', (self.si_classes or 0,), self._cond_clips(pcm, lens),
                           profile, passes, silence_remove, items_per_stream, return_pcm, nonstationary)

    def room_pipeline_conditioned(self, pcm, lens=None, profile=None, passes=1, silence_remove=True,
                                  items_per_stream=1, return_pcm=False, nonstationary=False):
        """condition() once in front of od_pipeline and si_pipeline -> (od_probs [n,K_od], od_argmax [n],
        si_probs [n,K], si_argmax [n], silent [n] bool, kept_len [n]); return_pcm adds the conditioned
        clips.  Both argmax are -1 where fewer than 4000 samples were kept."""
        return self._fused('mmla_room_pipeline_conditioned', (self._od_k(), self.si_classes or 0),
                           self._cond_clips(pcm, lens), profile, passes, silence_remove, items_per_stream,
                           return_pcm, nonstationary)

    # -- a room's capture format: streaming conversion to 16 kHz mono in front of the pipelines ----
    def capture_reset(self, n_streams, rate, channels=1, channel=0):
        """The capture format of every later capture call (rate in Hz, interleaved channels, channel k
        or MMLA_CAPTURE_MEAN for stereo) and n_streams fresh audioop.ratecv states."""
        self._check(self.lib.mmla_capture_reset(self.h, int(n_streams), int(rate), int(channels),
                                                int(channel)), 'mmla_capture_reset')
        self.capture_format = (int(rate), int(channels), int(channel))
        self.capture_streams = int(n_streams)

    @staticmethod
    def capture_out_len(clip_frames, rate):
        """the longest a clip of clip_frames capture frames can become at 16 kHz (the row width of the
        converted clips)"""
        from math import gcd
        g = gcd(int(rate), 16000)
        return (int(clip_frames) * (16000 // g) - 1) // (int(rate) // g) + 1

    def _capture_pcm(self, pcm, frames):
        """-> (contiguous int16 [n, clip_frames * channels], frames int32 [n] or None, clip_frames)"""
        fmt = getattr(self, 'capture_format', None)
        if fmt is None:
            raise MmlaError('capture_reset must be called first', -1)
        ch = fmt[1]
        if isinstance(pcm, (list, tuple)):
            for p in pcm:
                if len(p) % ch:
                    raise MmlaError(f'{len(p)} samples are not whole frames of {ch} channels', -1)
        a, ln, width = self._pcm(pcm, None)
        if isinstance(pcm, (list, tuple)):
            if width % ch:      # (only the placeholder width of a list of empty clips)
                a = np.zeros((a.shape[0], ch), np.int16)
            fr = ln // ch
        else:
            if a.shape[1] % ch:
                raise MmlaError(f'rows of {a.shape[1]} samples are not whole frames of {ch} channels', -1)
            fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
            if fr is not None and fr.shape != (a.shape[0],):
                raise ValueError(f'frames {fr.shape}: expected one count per clip ({a.shape[0]})')
        return a, fr, a.shape[1] // ch

    def capture_convert(self, pcm, frames=None, items_per_stream=1, fresh=False):
        """Interleaved capture int16 [n, clip_frames * channels] (or a list of clips) with frames[c]
        valid frames -> (int16 [n, out_clip_len] at 16 kHz mono, zeros behind out_lens; out_lens [n]).
        Stream s owns clips [s * items_per_stream, (s + 1) * items_per_stream) and its audioop state
        carries from clip to clip and from call to call.  fresh=True: from fresh states instead, the
        context's left alone."""
        a, fr, cf = self._capture_pcm(pcm, frames)
        n = a.shape[0]
        ocl = self.capture_out_len(max(cf, 1), self.capture_format[0])
        out = np.empty((n, ocl), np.int16)
        olen = np.empty(n, np.int32)
        self._check(self.lib.mmla_capture_convert(
            self.h, _ptr(a), n, a.shape[1], _ptr(fr), cf, int(items_per_stream), _ptr(out), ocl,
            _ptr(olen), MMLA_CAPTURE_FRESH if fresh else 0), 'mmla_capture_convert')
        return out, olen

    def capture_convert_dev(self, pcm, n, stride, clip_frames, out, out_stride, out_lens,
                            items_per_stream=1, frames=0, fresh=False):
        self._check(self.lib.mmla_capture_convert(
            self.h, pcm, n, stride, frames or None, clip_frames, int(items_per_stream), out, out_stride,
            out_lens, MMLA_DEVICE_PTR | (MMLA_CAPTURE_FRESH if fresh else 0)), 'mmla_capture_convert(dev)')

    def capture_state(self):
        """-> (d int32 [n_streams], prev int32 [n_streams]): audioop's phase counter and the last mono
        input sample of every stream"""
        n = getattr(self, 'capture_streams', 0)
        d = np.zeros(n, np.int32)
        prev = np.zeros(n, np.int32)
        self._check(self.lib.mmla_capture_state(self.h, _ptr(d) if n else None, _ptr(prev) if n else None),
                    'mmla_capture_state')
        return d, prev

    def _capture_clips(self, pcm, frames):
        a, fr, cf = self._capture_pcm(pcm, frames)
        return a, fr, cf, self.capture_out_len(max(cf, 1), self.capture_format[0])

    def od_pipeline_capture(self, pcm, frames=None, profile=None, passes=1, silence_remove=True,
                            items_per_stream=1, return_pcm=False, nonstationary=False):
        """od_pipeline_conditioned on interleaved capture in the capture_reset format: capture_convert
        of all clips, then the conditioned pipeline on the converted clips, which stay on the device ->
        (probs [n,K], argmax [n], silent [n] bool, kept_len [n] at 16 kHz); return_pcm adds the
        conditioned clips [n, out_clip_len]."""
        return self._fused('mmla_od_pipeline_capture', (self._od_k(),), self._capture_clips(pcm, frames), profile,
                           passes, silence_remove, items_per_stream, return_pcm, nonstationary)

    def si_pipeline_capture(self, pcm, frames=None, profile=None, passes=1, silence_remove=True,
                            items_per_stream=1, return_pcm=False, nonstationary=False):
        """si_pipeline_conditioned on interleaved capture -> (probs [n,K], argmax, silent, kept_len)"""
        return self._fused('mmla_si_pipeline_capture', (self.si_classes or 0,), self._capture_clips(pcm, frames),
                           profile, passes, silence_remove, items_per_stream, return_pcm, nonstationary)

    def room_pipeline_capture(self, pcm, frames=None, profile=None, passes=1, silence_remove=True,
                              items_per_stream=1, return_pcm=False, nonstationary=False):
        """room_pipeline_conditioned on interleaved capture -> (od_probs [n,K_od], od_argmax [n], si_probs
        [n,K], si_argmax [n], silent [n] bool, kept_len [n]); return_pcm adds the conditioned clips."""
        return self._fused('mmla_room_pipeline_capture', (self._od_k(), self.si_classes or 0),
                           self._capture_clips(pcm, frames), profile, passes, silence_remove, items_per_stream,
                           return_pcm, nonstationary)

    def _fused_call(self, name, dev, pcm, n, stride, lens, clip_len, passes, silence_remove, items_per_stream,
                    outs, out_pcm, kept_len, profile, nonstationary):
        """The one C call of condition and the {od,si,room}_pipeline_{conditioned,capture} methods, host
        (dev=False) and *_dev, on addresses (0 or None: a null pointer).  lens, clip_len: frames, clip_frames
        for capture; outs: each network's (probs, argmax), then silent."""
        self._check(getattr(self.lib, name)(
            self.h, pcm, n, stride, lens or None, clip_len, profile or None, int(passes),
            int(bool(silence_remove)), int(items_per_stream), out_pcm or None, kept_len or None,
            *[x or None for x in outs], (MMLA_DEVICE_PTR if dev else 0) | _ns(nonstationary)),
            name + ('(dev)' if dev else ''))

    def od_pipeline_capture_dev(self, pcm, n, stride, clip_frames, passes=1, silence_remove=True,
                                items_per_stream=1, probs=0, argmax=0, silent=0, out_pcm=0, kept_len=0,
                                frames=0, profile=0, nonstationary=False):
        """synchronises the context stream internally when passes > 0 (see mmla.h)"""
        self._fused_call('mmla_od_pipeline_capture', True, pcm, n, stride, frames, clip_frames, passes,
                         silence_remove, items_per_stream, (probs, argmax, silent), out_pcm, kept_len, profile,
                         nonstationary)

    def si_pipeline_capture_dev(self, pcm, n, stride, clip_frames, passes=1, silence_remove=True,
                                items_per_stream=1, probs=0, argmax=0, silent=0, out_pcm=0, kept_len=0,
                                frames=0, profile=0, nonstationary=False):
        """synchronises the context stream internally when passes > 0 (see mmla.h)"""
        self._fused_call('mmla_si_pipeline_capture', True, pcm, n, stride, frames, clip_frames, passes,
                         silence_remove, items_per_stream, (probs, argmax, silent), out_pcm, kept_len, profile,
                         nonstationary)

    def room_pipeline_capture_dev(self, pcm, n, stride, clip_frames, passes=1, silence_remove=True,
                                  items_per_stream=1, od_probs=0, od_argmax=0, si_probs=0, si_argmax=0,
                                  silent=0, out_pcm=0, kept_len=0, frames=0, profile=0, nonstationary=False):
        """synchronises the context stream internally when passes > 0 (see mmla.h)"""
        self._fused_call('mmla_room_pipeline_capture', True, pcm, n, stride, frames, clip_frames, passes,
                         silence_remove, items_per_stream, (od_probs, od_argmax, si_probs, si_argmax, silent),
                         out_pcm, kept_len, profile, nonstationary)

    def debug_vad_path(self, n_streams):
        """True when a detector call over n_streams streams runs the one-stream-per-wave kernel"""
        wave = _I32()
        self._check(self.lib.mmla_debug_vad_path(self.h, int(n_streams), ctypes.byref(wave)),
                    'mmla_debug_vad_path')
        return bool(wave.value)

    def ssim_u8(self, a, b):
        """Mean SSIM (scikit-image defaults, multichannel) of uint8 image pairs a, b [n,h,w,c] (or one
        pair [h,w,c]) -> float32 [n] (or a scalar)."""
        a = np.ascontiguousarray(a)
        b = np.ascontiguousarray(b)
        if a.dtype != np.uint8 or b.dtype != np.uint8 or a.shape != b.shape or a.ndim not in (3, 4):
            raise ValueError(f'ssim_u8 takes two uint8 arrays [n,h,w,c] of one shape, got {a.dtype} '
                             f'{a.shape} and {b.dtype} {b.shape}')
        single = a.ndim == 3
        if single:
            a, b = a[None], b[None]
        n, h, w, c = a.shape
        out = np.empty(n, np.float32)
        self._check(self.lib.mmla_ssim_u8(self.h, _ptr(a) if a.size else None,
                                          _ptr(b) if b.size else None, n, h, w, c, _ptr(out), 0),
                    'mmla_ssim_u8')
        return out[0] if single else out

    def od_pipeline_strided(self, signal, n, stride, clip_len):
        """OD pipeline over n windows of one long int16 signal: window c = signal[c*stride :
        c*stride + clip_len] (overlapping when stride < clip_len; no host-side copies)."""
        sig = np.ascontiguousarray(signal, dtype=np.int16).reshape(-1)
        if n < 0 or (n > 0 and (n - 1) * stride + clip_len > sig.size):
            raise MmlaError(f'{n} windows of {clip_len} at stride {stride} exceed {sig.size} samples')
        probs = np.empty((n, self._od_k()), np.float32)
        am = np.empty(n, np.int32)
        self._check(self.lib.mmla_od_pipeline(self.h, _ptr(sig), n, stride, None, clip_len,
                                              _ptr(probs), _ptr(am), None, 0), 'mmla_od_pipeline')
        return probs, am

    def od_features_strided(self, signal, n, stride, clip_len, db=True, norm=True, zcr=True, img=True,
                            image_type=None):
        """OD features of n windows of one long signal: window c = signal[c*stride : c*stride +
        clip_len] (int16 -> mmla_od_features, float -> mmla_od_features_f32; no host copies)"""
        fl = np.issubdtype(np.asarray(signal).dtype, np.floating)
        sig = np.ascontiguousarray(signal, dtype=np.float32 if fl else np.int16).reshape(-1)
        if n < 0 or (n > 0 and (n - 1) * stride + clip_len > sig.size):
            raise MmlaError(f'{n} windows of {clip_len} at stride {stride} exceed {sig.size} samples')
        bufs = {}
        for key, want, shape, dt in (('db', db, (n, OD_MELS, OD_FRAMES), np.float32),
                                     ('norm', norm, (n, OD_MELS, OD_FRAMES), np.float32),
                                     ('zcr', zcr, (n, OD_FRAMES), np.float32),
                                     ('img', img, (n, OD_MELS, OD_FRAMES, 3), np.uint8)):
            bufs[key] = np.empty(shape, dt) if want else None
        fn = self.lib.mmla_od_features_f32 if fl else self.lib.mmla_od_features
        self._check(fn(self.h, _ptr(sig), n, stride, None, clip_len, _ptr(bufs['db']),
                       _ptr(bufs['norm']), _ptr(bufs['zcr']), _ptr(bufs['img']), _img_flags(image_type)),
                    'mmla_od_features(strided)')
        return {k: v for k, v in bufs.items() if v is not None}

    def si_pipeline(self, pcm, lens=None):
        a, ln, L = self._pcm(pcm, lens)
        n = a.shape[0]
        probs = np.empty((n, self.si_classes or 0), np.float32)
        am = np.empty(n, np.int32)
        silent = np.empty(n, np.uint8)
        self._check(self.lib.mmla_si_pipeline(self.h, _ptr(a), n, a.shape[1], _ptr(ln), L,
                                              _ptr(probs), _ptr(am), _ptr(silent), 0),
                    'mmla_si_pipeline')
        return probs, am, silent.astype(bool)

    # -- device-pointer API (asynchronous on the context stream) -------------------------------
    def od_features_dev(self, pcm, n, stride, clip_len, db=0, norm=0, zcr=0, img=0, lens=0, image_type=None):
        self._check(self.lib.mmla_od_features(self.h, pcm, n, stride, lens or None, clip_len,
                                              db or None, norm or None, zcr or None, img or None,
                                              MMLA_DEVICE_PTR | _img_flags(image_type)), 'mmla_od_features(dev)')

    def si_features_dev(self, pcm, n, stride, clip_len, feat, silent=0, lens=0):
        self._check(self.lib.mmla_si_features(self.h, pcm, n, stride, lens or None, clip_len, feat,
                                              silent or None, MMLA_DEVICE_PTR),
                    'mmla_si_features(dev)')

    def si_features_seq_batch_dev(self, pcm, n, stride, clip_len, feat, n_windows=0, lens=0):
        """lens: device int32 [n] (0: clip_len each); entries outside [0, clip_len] are clamped"""
        self._check(self.lib.mmla_si_features_seq_batch(self.h, pcm, n, stride, lens or None, clip_len, feat,
                                                        n_windows or None, MMLA_DEVICE_PTR),
                    'mmla_si_features_seq_batch(dev)')

    def si_enrol_embed_dev(self, pcm, n, stride, clip_len, emb, passes=1, silence_remove=True, vad_mode=3,
                           out_pcm=0, kept_len=0, n_windows=0, lens=0, profile=0, nonstationary=False):
        """synchronises the context stream internally (see mmla.h)"""
        self._check(self.lib.mmla_si_enrol_embed(
            self.h, pcm, n, stride, lens or None, clip_len, profile or None, int(passes),
            int(bool(silence_remove)), int(vad_mode), out_pcm or None, kept_len or None, n_windows or None,
            emb, MMLA_DEVICE_PTR | _ns(nonstationary)), 'mmla_si_enrol_embed(dev)')

    def od_pipeline_dev(self, pcm, n, stride, clip_len, probs=0, argmax=0, lens=0, silent=0):
        self._check(self.lib.mmla_od_pipeline(self.h, pcm, n, stride, lens or None, clip_len,
                                              probs or None, argmax or None, silent or None,
                                              MMLA_DEVICE_PTR),
                    'mmla_od_pipeline(dev)')

    def od_pipeline_gated_dev(self, pcm, n, stride, clip_len, passes=4, threshold=0.3, probs=0,
                              argmax=0, silent=0, ssim=0, lens=0, nonstationary=False):
        """synchronises the context stream internally when passes > 0 (see mmla.h)"""
        self._check(self.lib.mmla_od_pipeline_gated(
            self.h, pcm, n, stride, lens or None, clip_len, int(passes), float(threshold),
            probs or None, argmax or None, silent or None, ssim or None,
            MMLA_DEVICE_PTR | _ns(nonstationary)), 'mmla_od_pipeline_gated(dev)')

    def condition_dev(self, pcm, n, stride, clip_len, passes=1, silence_remove=True,
                      items_per_stream=1, out_pcm=0, kept_len=0, lens=0, profile=0, nonstationary=False):
        """synchronises the context stream internally when passes > 0 (see mmla.h)"""
        self._fused_call('mmla_condition', True, pcm, n, stride, lens, clip_len, passes, silence_remove,
                         items_per_stream, (), out_pcm, kept_len, profile, nonstationary)

    def od_pipeline_conditioned_dev(self, pcm, n, stride, clip_len, passes=1, silence_remove=True,
                                    items_per_stream=1, probs=0, argmax=0, silent=0, out_pcm=0,
                                    kept_len=0, lens=0, profile=0, nonstationary=False):
        """synchronises the context stream internally when passes > 0 (see mmla.h)"""
        self._fused_call('mmla_od_pipeline_conditioned', True, pcm, n, stride, lens, clip_len, passes,
                         silence_remove, items_per_stream, (probs, argmax, silent), out_pcm, kept_len, profile,
                         nonstationary)

    def si_pipeline_conditioned_dev(self, pcm, n, stride, clip_len, passes=1, silence_remove=True,
                                    items_per_stream=1, probs=0, argmax=0, silent=0, out_pcm=0,
                                    kept_len=0, lens=0, profile=0, nonstationary=False):
        """synchronises the context stream internally when passes > 0 (see mmla.h)"""
        self._fused_call('mmla_si_pipeline_conditioned', True, pcm, n, stride, lens, clip_len, passes,
                         silence_remove, items_per_stream, (probs, argmax, silent), out_pcm, kept_len, profile,
                         nonstationary)

    def room_pipeline_conditioned_dev(self, pcm, n, stride, clip_len, passes=1, silence_remove=True,
                                      items_per_stream=1, od_probs=0, od_argmax=0, si_probs=0,
                                      si_argmax=0, silent=0, out_pcm=0, kept_len=0, lens=0, profile=0,
                                      nonstationary=False):
        """synchronises the context stream internally when passes > 0 (see mmla.h)"""
        self._fused_call('mmla_room_pipeline_conditioned', True, pcm, n, stride, lens, clip_len, passes,
                         silence_remove, items_per_stream, (od_probs, od_argmax, si_probs, si_argmax, silent),
                         out_pcm, kept_len, profile, nonstationary)

    def ssim_u8_dev(self, a, b, n, h, w, c, out):
        self._check(self.lib.mmla_ssim_u8(self.h, a, b, n, h, w, c, out, MMLA_DEVICE_PTR),
                    'mmla_ssim_u8(dev)')

    def si_pipeline_dev(self, pcm, n, stride, clip_len, probs=0, argmax=0, silent=0, lens=0):
        self._check(self.lib.mmla_si_pipeline(self.h, pcm, n, stride, lens or None, clip_len,
                                              probs or None, argmax or None, silent or None,
                                              MMLA_DEVICE_PTR), 'mmla_si_pipeline(dev)')

    def od_forward_dev(self, x, n, probs, u8=False):
        fn = self.lib.mmla_od_forward_u8 if u8 else self.lib.mmla_od_forward
        self._check(fn(self.h, x, n, probs, MMLA_DEVICE_PTR), 'mmla_od_forward(dev)')

    def si_forward_dev(self, x, n, probs):
        self._check(self.lib.mmla_si_forward(self.h, x, n, probs, MMLA_DEVICE_PTR),
                    'mmla_si_forward(dev)')

    def si_embed_dev(self, x, n, emb):
        self._check(self.lib.mmla_si_embed(self.h, x, n, emb, MMLA_DEVICE_PTR), 'mmla_si_embed(dev)')

    def si_head_fit_dev(self, emb, labels, n_train, val_emb, val_labels, n_val, n_classes, n_restarts,
                        epochs, batch, lr, w0, b0, perm, w, b, history=0):
        """mmla_si_head_fit on device buffers: the caller guarantees labels in [0, K) and that every
        perm row is a permutation (unchecked: the kernel only clamps a perm entry into range)"""
        self._check(self.lib.mmla_si_head_fit(
            self.h, emb, labels, n_train, val_emb or None, val_labels or None, n_val, n_classes,
            n_restarts, epochs, batch, float(lr), w0, b0, perm, w, b, history or None,
            MMLA_DEVICE_PTR), 'mmla_si_head_fit(dev)')

    def si_loss_grad_dev(self, packed, n_floats, n_classes, x, labels, n, loss, grad):
        """mmla_si_loss_grad on device buffers (labels in [0, K) are the caller's to guarantee)"""
        self._check(self.lib.mmla_si_loss_grad(self.h, packed, n_floats, n_classes, x, labels, n, loss, grad,
                                               MMLA_DEVICE_PTR), 'mmla_si_loss_grad(dev)')

    def si_finetune_dev(self, packed, n_floats, n_classes, x, labels, n_train, val_x, val_labels, n_val,
                        epochs, batch, lr, perm, packed_out, history):
        """mmla_si_finetune on device buffers: the caller guarantees labels in [0, K) and that every
        perm row is a permutation; asynchronous on the context's stream"""
        self._check(self.lib.mmla_si_finetune(
            self.h, packed, n_floats, n_classes, x, labels, n_train, val_x or None, val_labels or None,
            n_val, epochs, batch, float(lr), perm, packed_out, history, MMLA_DEVICE_PTR),
            'mmla_si_finetune(dev)')

    def si_base_drop_mask_dev(self, drop_seed, epoch, sample_ids, n, mask_a, mask_b):
        """mmla_si_base_drop_mask on device buffers (sample_ids 0: 0..n-1)"""
        self._check(self.lib.mmla_si_base_drop_mask(self.h, _seed64(drop_seed), epoch, sample_ids or None, n, mask_a,
                                                    mask_b, MMLA_DEVICE_PTR), 'mmla_si_base_drop_mask(dev)')

    def si_base_loss_grad_dev(self, packed, n_floats, n_classes, x, labels, n, drop_seed, epoch, sample_ids,
                              loss, grad, moving_out=0):
        """mmla_si_base_loss_grad on device buffers (labels in [0, K) are the caller's to guarantee)"""
        self._check(self.lib.mmla_si_base_loss_grad(
            self.h, packed, n_floats, n_classes, x, labels, n, _seed64(drop_seed), epoch, sample_ids or None, loss,
            grad, moving_out or None, MMLA_DEVICE_PTR), 'mmla_si_base_loss_grad(dev)')

    def si_base_train_dev(self, packed, n_floats, n_classes, x, labels, n_train, val_x, val_labels, n_val,
                          epochs, batch, lr, perm, drop_seed, patience, ckpt_period, packed_out, best_out,
                          history, epochs_run, best_epoch):
        """mmla_si_base_train on device buffers (epochs_run, best_epoch: device int32 words): the caller
        guarantees labels in [0, K) and that every perm row is a permutation; asynchronous on the context's
        stream unless a callback is on (patience or ckpt_period > 0 with n_val > 0)"""
        self._check(self.lib.mmla_si_base_train(
            self.h, packed, n_floats, n_classes, x, labels, n_train, val_x or None, val_labels or None, n_val,
            epochs, batch, float(lr), perm or None, _seed64(drop_seed), patience, ckpt_period, packed_out,
            best_out or None, history or None, epochs_run, best_epoch, MMLA_DEVICE_PTR),
            'mmla_si_base_train(dev)')

    def od_loss_grad_dev(self, packed, n_floats, img, labels, n, h, w, class_w, drop_mask, loss, grad,
                         moving_out=0):
        """mmla_od_loss_grad on device buffers (class_w: a host float32 [K] array)"""
        cw = self._od_class_w(class_w, n_floats)
        self._check(self.lib.mmla_od_loss_grad(self.h, packed, n_floats, img, labels, n, h, w, _ptr(cw),
                                               drop_mask or None, loss, grad, moving_out or None,
                                               MMLA_DEVICE_PTR), 'mmla_od_loss_grad(dev)')

    def od_finetune_dev(self, packed, n_floats, img, labels, n_train, val_img, val_labels, n_val, h, w, class_w,
                        epochs, batch, lr, perm, drop_mask, patience, packed_out, history, epochs_run):
        """mmla_od_finetune on device buffers (class_w, lr: host float32 arrays): the caller guarantees
        labels in {0, 1} and that every perm row is a permutation; asynchronous on the context's stream
        unless patience > 0 and n_val > 0"""
        cw = self._od_class_w(class_w, n_floats)
        lr = np.ascontiguousarray(lr, dtype=np.float32).ravel()
        self._check(self.lib.mmla_od_finetune(
            self.h, packed, n_floats, img, labels, n_train, val_img or None, val_labels or None, n_val, h, w,
            _ptr(cw), epochs, batch, _ptr(lr), perm, drop_mask or None, patience, packed_out, history,
            epochs_run, MMLA_DEVICE_PTR), 'mmla_od_finetune(dev)')

    def od_train_dev(self, packed, n_floats, img, labels, n_train, val_img, val_labels, n_val, h, w, class_w,
                     epochs, batch, lr, perm, drop_seed, patience, ckpt_period, packed_out, best_out, history,
                     epochs_run, best_epoch):
        """mmla_od_train on device buffers (class_w, lr: host float32 arrays; epochs_run, best_epoch: device
        int32 words): the caller guarantees labels in {0, 1} and that every perm row is a permutation;
        asynchronous on the context's stream unless a callback is on (patience or ckpt_period > 0 with
        n_val > 0)"""
        cw = self._od_class_w(class_w, n_floats)
        lr = np.ascontiguousarray(lr, dtype=np.float32).ravel()
        self._check(self.lib.mmla_od_train(
            self.h, packed, n_floats, img, labels, n_train, val_img or None, val_labels or None, n_val, h, w,
            _ptr(cw), epochs, batch, _ptr(lr), perm or None, _seed64(drop_seed), patience, ckpt_period, packed_out,
            best_out or None, history or None, epochs_run, best_epoch, MMLA_DEVICE_PTR), 'mmla_od_train(dev)')

    def od_drop_mask_dev(self, drop_seed, epoch, sample_ids, n, mask):
        """mmla_od_drop_mask on device buffers (sample_ids 0: 0..n-1)"""
        self._check(self.lib.mmla_od_drop_mask(self.h, _seed64(drop_seed), epoch, sample_ids or None, n, mask,
                                               MMLA_DEVICE_PTR), 'mmla_od_drop_mask(dev)')

    def od_augment_dev(self, img, n, h, w, src, levels, m, out):
        """mmla_od_augment on device buffers (src and levels are clamped into range)"""
        self._check(self.lib.mmla_od_augment(self.h, img, n, h, w, src or None, levels or None, m, out or None,
                                             MMLA_DEVICE_PTR), 'mmla_od_augment(dev)')

    def od_auc_dev(self, probs, labels, n, auc_out):
        """mmla_od_auc on device buffers (a label selects its class by its lowest bit)"""
        self._check(self.lib.mmla_od_auc(self.h, probs, labels, n, auc_out, MMLA_DEVICE_PTR), 'mmla_od_auc(dev)')


_default = {}


def default_context(device=None):
    """Process-wide context per device (device defaults to LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get('LOCAL_RANK', 0))
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]
