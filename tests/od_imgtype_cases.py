"""TEST INFRASTRUCTURE: inputs and rules of the OD image-type tests (gray and viridis images, the one-channel
network) -- tests/test_od_imgtype_cpu.py checks their conditions, tests/test_gpu_od_imgtype.py holds the kernels
to them.  Everything computed here is computed once per process, shared and never modified.

The image rule (what ``plt.imsave(path, norm, origin="lower", cmap=name)`` writes for the float32
``normalize_matrix`` output, checked against matplotlib in the CPU test):

    row h of the image = band 127 - h;  idx = min(trunc(float32(v) * 256), 255);  pixel = LUT[name][idx];
    a NaN v (digital silence) -> (0, 0, 0) (imsave's RGBA (0, 0, 0, 0))

with LUT = ``matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3]``, kept as the fixture
tests/golden/cmap_lut.npz (tests/golden/make_cmap_lut.py) so that a machine without matplotlib can test.

The one-channel network's gradient and fit cases are those of tests/od_finetune_cases.py on channel 0 of its
images with ``weights.synthetic(OD, seed, channels=1)``; the seeds are chosen here, on the CPU, for the pool
and LeakyReLU margins the d32 rule rests on.
"""
import functools
import os

import numpy as np
import torch

import od_finetune_cases as C
import od_finetune_ref as ref
from mmla_audio_amd import _lib, overlap_detector, weights
from oracle import od_fe, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TYPES = ('gray', 'viridis')
OD = weights.OD

# ---- the image rule -------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def luts():
    """{'gray' | 'viridis': uint8 [256, 3]} of the fixture"""
    z = np.load(os.path.join(GOLDEN, 'cmap_lut.npz'))
    out = {n: np.ascontiguousarray(z[n]) for n in TYPES}
    for v in out.values():
        assert v.shape == (256, 3) and v.dtype == np.uint8
        v.setflags(write=False)
    return out


def index(norm):
    """float32 [..., 128, 151] (not flipped) -> int [...]: min(trunc(v * 256), 255) in float32, -1 where NaN"""
    v = np.asarray(norm, np.float32)
    nan = np.isnan(v)
    with np.errstate(invalid='ignore'):
        s = (np.where(nan, np.float32(0), v) * np.float32(256)).astype(np.float32)
    idx = np.minimum(np.trunc(s).astype(np.int64), 255)
    return np.where(nan, -1, idx)


def rule(norm, name):
    """the model's image of `norm` float32 [..., 128, 151]: uint8 [..., 128, 151, 3], rows flipped"""
    idx = index(norm)
    img = luts()[name][np.maximum(idx, 0)]
    img[idx < 0] = 0
    return np.ascontiguousarray(np.flip(img, axis=-3))


# ---- front-end clips ------------------------------------------------------------------------------------------

N_CLIPS = 32
LENS = (0, 3999, 24000, 40000)
CLIP0 = 4100      # oracle.synth clip indices 4100 .. 4131: every class (i % 5) at every length (i % 4)


@functools.lru_cache(maxsize=None)
def clips():
    """-> (pcm int16 [32, 40000], lens int32 [32]): synth's five classes, digital zeros among them"""
    pcm = synth.batch(CLIP0, N_CLIPS, 40000)
    lens = np.array([LENS[i % len(LENS)] for i in range(N_CLIPS)], np.int32)
    pcm.setflags(write=False)
    lens.setflags(write=False)
    return pcm, lens


@functools.lru_cache(maxsize=None)
def oracle_norms():
    """float32 [32, 128, 151]: the oracle's normalize_matrix output of every clip (NaN for a constant one)"""
    pcm, lens = clips()
    out = np.stack([od_fe.generate_mels(pcm[i, :lens[i]])[1] for i in range(N_CLIPS)]).astype(np.float32)
    out.setflags(write=False)
    return out


# ---- the one-channel network ----------------------------------------------------------------------------------

FWD_SEED = 3


def synthetic1(seed, n_classes=None):
    return weights.synthetic(OD, seed=seed, n_classes=n_classes, channels=1)


def pack1(W):
    return weights.pack(OD, W, weights.od_classes(W), 1)


def unpack1(blob):
    k, ch = weights.od_layout_of(np.asarray(blob).size)
    assert ch == 1
    return weights.unpack(OD, blob, k, 1)


def forward_random(n=2):
    """random one-channel images uint8 [n, 128, 151, 1]"""
    x = np.random.default_rng([FWD_SEED, 97]).integers(0, 256, (n, 128, 151, 1)).astype(np.uint8)
    return x


# (h, w, B) -> seed, chosen on the CPU (tests/test_od_imgtype_cpu.py asserts them): pool and LeakyReLU
# margins >= od_finetune_cases.MARGIN in the float64 run of the one-channel network (seed 1 of (20, 23, 3)
# has a pool window 1e-6 apart)
GRAD_CASES = {(20, 23, 3): 2, (9, 8, 1): 1}


def grad_case(h, w, B):
    """-> (W one-channel, img [B,h,w,1] u8, labels [B], mask [B,512] u8)"""
    seed = GRAD_CASES[(h, w, B)]
    img, labels, mask = C.images(seed + 100 * h + w, B, h, w)
    return synthetic1(seed), np.ascontiguousarray(img[..., :1]), labels, mask


@functools.lru_cache(maxsize=None)
def grad_ref(h, w, B):
    """-> {dtype name: (loss, {name: grad}, {name: value after the moving update}, margins)}"""
    W, img, labels, mask = grad_case(h, w, B)
    return {'f64': ref.loss_and_grad(W, img, labels, C.CLASS_W, mask, torch.float64),
            'f32': ref.loss_and_grad(W, img, labels, C.CLASS_W, mask, torch.float32)}


FIT = C.FIT      # 20 x 23, 10 + 4 images, 3 epochs


def fit_case():
    c = C._fit_case(FIT, overlap_detector.cosine_lr(FIT['epochs']))
    c['W'] = synthetic1(FIT['seed'])
    c['img'] = np.ascontiguousarray(c['img'][..., :1])
    c['val_img'] = np.ascontiguousarray(c['val_img'][..., :1])
    return c


@functools.lru_cache(maxsize=None)
def fit_ref():
    """-> {dtype name: (W_out, history, epochs_run, margins)} of the restatement on fit_case()"""
    return C._fit_ref(fit_case(), FIT, 0)
