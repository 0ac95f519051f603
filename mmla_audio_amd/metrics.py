"""Drop-in for ``skimage.metrics.structural_similarity`` on uint8 images, on the GPU.

The reference's edge loop decides 'silent' by comparing the feature image of a clip with the feature
image of the same clip after four passes of the noise gate (``OverlapDetection/scripts/
record_on_pi.py:39-48,103-124``): ``structural_similarity(image1, image2, multichannel=True) < 0.3``.
``from mmla_audio_amd.metrics import structural_similarity`` keeps that call unchanged; it runs
``mmla_ssim_u8`` (csrc/ssim.hip).  Only what that call uses is built: uint8 images, the default 7 x 7
uniform window, data_range 255, the mean as the only result.  Anything else raises, there is no CPU
fallback.  For whole batches use ``Context.ssim_u8`` or the fused
``OverlapDetectionModel.predict_wavs_gated``.
"""
import numpy as np

from . import _lib

_DEFAULT_KWARGS = {'K1': 0.01, 'K2': 0.03, 'sigma': 1.5, 'use_sample_covariance': True}


def structural_similarity(im1, im2, *, win_size=None, gradient=False, data_range=None,
                          multichannel=False, channel_axis=None, gaussian_weights=False, full=False,
                          **kwargs):
    """Mean structural similarity of two uint8 images [h, w] or, with ``multichannel=True`` /
    ``channel_axis=-1``, [h, w, c] with c in {1, 3, 4} (scikit-image's signature and defaults)."""
    if gradient or full:
        raise NotImplementedError('only the mean similarity is built (gradient=False, full=False)')
    if gaussian_weights:
        raise NotImplementedError('only the uniform window is built (gaussian_weights=False)')
    if win_size not in (None, 7):
        raise NotImplementedError(f'only the default win_size 7 is built (got {win_size})')
    if data_range not in (None, 255):
        raise NotImplementedError(f'only data_range 255 is built (got {data_range})')
    for k, v in kwargs.items():
        if k not in _DEFAULT_KWARGS:
            raise TypeError(f'structural_similarity() got an unexpected keyword argument {k!r}')
        if v != _DEFAULT_KWARGS[k]:
            raise NotImplementedError(f'only the default {k}={_DEFAULT_KWARGS[k]} is built (got {v})')
    a, b = np.asarray(im1), np.asarray(im2)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise NotImplementedError(f'only uint8 images are built (got {a.dtype} and {b.dtype})')
    if a.shape != b.shape:
        raise ValueError('Input images must have the same dimensions.')
    channels = bool(multichannel) or channel_axis is not None
    if a.ndim == 2 and not channels:
        a, b = a[..., None], b[..., None]
    elif a.ndim == 3 and channels:
        if channel_axis not in (None, -1, 2):
            raise NotImplementedError(f'only channels-last images are built (channel_axis={channel_axis})')
        if a.shape[2] not in (1, 3, 4):
            raise NotImplementedError(f'only 1, 3 or 4 channels are built (got {a.shape[2]})')
    else:
        raise NotImplementedError(f'only [h, w] images, or [h, w, c] with multichannel=True / '
                                  f'channel_axis=-1, are built (got {a.ndim} dimensions, '
                                  f'multichannel={bool(channels)})')
    if a.shape[0] < 7 or a.shape[1] < 7:
        raise ValueError('win_size exceeds image extent.')
    return np.float64(_lib.default_context().ssim_u8(a, b))


def auc(probs, labels):
    """``tf.keras.metrics.AUC()`` at its defaults, as ``OverlapDetector.train_model`` compiles it
    (overlap_detector.py:403), through ``mmla_od_auc_k``: probs float32 [n, K] against labels [n] in [0, K) (or
    their one-hot rows [n, K]), K = 2 .. 8 -> float.  multi_label = False: the n K entries are binary
    predictions against the one-hot entries.  include/mmla.h states the thresholds and the one deliberate
    deviation (the final sum in double)."""
    labels = np.asarray(labels)
    if labels.ndim == 2:
        labels = labels.argmax(axis=1)
    return float(_lib.default_context().od_auc(probs, labels))


def compare_images(img1_path, img2_path, threshold=0.3):
    """``compare_images`` of record_on_pi.py:39-48: True ('silent') when the two PNG files' similarity
    is below the threshold.  The files are read as 3 channels (``cv2.imread`` drops alpha too, and its
    BGR order does not change a mean over channels)."""
    from . import tf_compat as tf
    image1 = tf.image.decode_png(tf.io.read_file(img1_path), 3).numpy()
    image2 = tf.image.decode_png(tf.io.read_file(img2_path), 3).numpy()
    s = structural_similarity(image1, image2, multichannel=True)
    if s < threshold:
        print('The similarity is too low, which is ', s)
        return True
    return False
