"""GPU: the batched, ragged sequence mode of the SI front-end (mmla_si_features_seq_batch).

One batch of nine signals in rows of 82161 samples (w_max = 3) whose lengths sit on every frame-count and
window-count boundary: T = -, 1, 1, 2, 3, 256, 257, 512, 513.  Every valid window must equal, byte for byte,
mmla_si_features_seq of that signal alone; every other window is zeros."""
import numpy as np
import pytest

import enrol_inputs
from mmla_audio_amd import _lib

pytestmark = pytest.mark.gpu

CLIP = 82161
LENS = np.array([0, 1, 400, 401, 561, 41200, 41201, 82160, 82161], np.int32)
N_WINDOWS = [0, 1, 1, 1, 1, 1, 2, 2, 3]


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def batch():
    """distinct, non-periodic content per signal: white noise under a slow random envelope, and garbage
    behind every signal's length (nothing behind lens[i] may enter its features)"""
    rng = np.random.default_rng(7100)
    x = np.empty((len(LENS), CLIP), np.int16)
    for i in range(len(LENS)):
        env = 0.2 + 0.8 * np.abs(np.sin(np.arange(CLIP) * rng.uniform(1e-4, 1e-3) + rng.uniform(0, 6)))
        x[i] = np.round(6000.0 * env * rng.standard_normal(CLIP)).astype(np.int16)
    x.setflags(write=False)
    return x


@pytest.fixture(scope='module')
def alone(ctx, batch):
    """si_features_seq of every non-empty signal alone, computed once"""
    ref = [None if m == 0 else ctx.si_features_seq(batch[i, :m]) for i, m in enumerate(LENS)]
    for r in ref:
        if r is not None:
            r.setflags(write=False)
    return ref


def _check(feat, nw, alone, lens=LENS, n_windows=N_WINDOWS):
    w_max = enrol_inputs.windows(CLIP)
    assert w_max == 3 and feat.shape == (len(lens), w_max, 256, 39) and feat.dtype == np.float32
    assert nw.tolist() == list(n_windows)
    for i, k in enumerate(n_windows):
        if k:
            assert alone[i].shape == (k, 256, 39)
            assert feat[i, :k].tobytes() == alone[i].tobytes(), f'signal {i} (len {lens[i]})'
        assert not feat[i, k:].any(), f'signal {i}: a window past its last is not zero'


def test_window_counts_of_the_shapes():
    assert [enrol_inputs.frames(int(m)) for m in LENS[1:]] == [1, 1, 2, 3, 256, 257, 512, 513]
    assert [enrol_inputs.windows(int(m)) for m in LENS] == N_WINDOWS


def test_batch_equals_every_signal_alone(ctx, batch, alone):
    feat, nw = ctx.si_features_seq_batch(batch, lens=LENS)
    _check(feat, nw, alone)
    # a list of ragged signals is the same batch
    feat2, nw2 = ctx.si_features_seq_batch([batch[i, :m] for i, m in enumerate(LENS)])
    assert feat2.tobytes() == feat.tobytes() and nw2.tolist() == nw.tolist()


def test_device_pointers_and_clamped_lens(ctx, batch, alone):
    import torch
    n, w_max = len(LENS), 3
    x = torch.from_numpy(batch.copy()).cuda()
    lens = LENS.copy()
    lens[8] = CLIP + 1000            # a device lens entry above clip_len behaves as clip_len
    dl = torch.from_numpy(lens).cuda()
    feat = torch.full((n, w_max, 256, 39), 7.0, dtype=torch.float32, device='cuda')
    nw = torch.full((n,), -1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.si_features_seq_batch_dev(x.data_ptr(), n, CLIP, CLIP, feat.data_ptr(), nw.data_ptr(), dl.data_ptr())
    ctx.synchronize()
    _check(feat.cpu().numpy(), nw.cpu().numpy(), alone)
    # without lens every signal has clip_len samples
    ctx.si_features_seq_batch_dev(x.data_ptr(), n, CLIP, CLIP, feat.data_ptr(), nw.data_ptr())
    ctx.synchronize()
    f = feat.cpu().numpy()
    assert nw.cpu().numpy().tolist() == [3] * n
    assert f[8].tobytes() == alone[8].tobytes()


def test_host_lens_above_clip_len_is_rejected(ctx, batch):
    lens = LENS.copy()
    lens[3] = CLIP + 1
    with pytest.raises(_lib.MmlaError) as e:
        ctx.si_features_seq_batch(batch, lens=lens)
    assert e.value.code == -1, e.value
    lens[3] = -1
    with pytest.raises(_lib.MmlaError) as e:
        ctx.si_features_seq_batch(batch, lens=lens)
    assert e.value.code == -1, e.value


def test_the_other_modes_still_run_after_the_batched_one(ctx, batch, alone):
    before, _ = ctx.si_features(batch[5:7, :41200], lens=[41200, 3999])
    ctx.si_features_seq_batch(batch, lens=LENS)
    clip, silent = ctx.si_features(batch[5:7, :41200], lens=[41200, 3999])
    assert silent.tolist() == [False, True] and not clip[1].any() and clip[0].any()
    assert clip.tobytes() == before.tobytes()
    again = ctx.si_features_seq(batch[8])
    assert again.tobytes() == alone[8].tobytes()
