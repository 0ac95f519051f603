"""GPU: the bank of noise profiles (mmla_nr_set_noise_bank / mmla_nr_reduce_bank) -- one profile per
microphone, all from one launch sequence.  Gating against profile p of the bank must give the bytes
of mmla_nr_set_noise(noise_p) + mmla_nr_reduce, whatever the other profiles' lengths are and however
the profiles are mixed within one call."""
import numpy as np
import pytest

import cond_ref
from mmla_audio_amd import _lib

pytestmark = pytest.mark.gpu

NOISE_LENS = (16000, 12345, 2)       # different frame counts per profile; 2: the shortest clip allowed


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def noises():
    return [cond_ref.noise(p)[:m] for p, m in enumerate(NOISE_LENS)]


@pytest.fixture(scope='module')
def signals():
    y = cond_ref.clips().astype(np.float32) / np.float32(32768.0)
    y.setflags(write=False)
    return y


@pytest.fixture(scope='module')
def singles(ctx, noises, signals):
    """the six clips gated against each profile set alone; leaves the bank of three in the context"""
    want = []
    for nz in noises:
        ctx.nr_set_noise(nz)
        want.append(ctx.nr_reduce(signals))
    for w in want:
        w.setflags(write=False)
    ctx.nr_set_noise_bank(noises)
    return want


def test_bank_equals_single_profiles(ctx, signals, singles):
    for p in range(3):
        got = ctx.nr_reduce_bank(signals, profile=p)
        assert got.tobytes() == singles[p].tobytes(), p
    assert singles[0].tobytes() != singles[1].tobytes() != singles[2].tobytes()
    # no profile array, and the call that knows no bank: profile 0
    assert ctx.nr_reduce_bank(signals).tobytes() == singles[0].tobytes()
    assert ctx.nr_reduce(signals).tobytes() == singles[0].tobytes()


def test_mixed_profiles_in_one_call(ctx, signals, singles):
    y = np.concatenate([signals, signals])
    profile = np.array([0, 1, 2, 0, 1, 2, 2, 2, 1, 1, 0, 0], np.int32)
    got = ctx.nr_reduce_bank(y, profile)
    for i, p in enumerate(profile):
        assert got[i].tobytes() == singles[p][i % 6].tobytes(), (i, p)


def test_set_noise_is_a_bank_of_one(ctx, noises, signals, singles):
    try:
        ctx.nr_set_noise(noises[1])
        assert ctx.nr_reduce_bank(signals, profile=0).tobytes() == singles[1].tobytes()
        with pytest.raises(_lib.MmlaError) as e:
            ctx.nr_reduce_bank(signals, profile=1)
        assert e.value.code == -1
    finally:
        ctx.nr_set_noise_bank(noises)


def test_host_profile_outside_the_bank_is_invalid(ctx, signals, singles):
    for bad in (3, -1):
        with pytest.raises(_lib.MmlaError) as e:
            ctx.nr_reduce_bank(signals, profile=np.array([0, 1, 2, bad, 0, 0], np.int32))
        assert e.value.code == -1
    with pytest.raises(_lib.MmlaError) as e:       # a noise clip of one sample
        ctx.nr_set_noise_bank([cond_ref.noise(0), cond_ref.noise(1)[:1]])
    assert e.value.code == -1
    assert ctx.nr_reduce_bank(signals, profile=2).tobytes() == singles[2].tobytes()   # the bank stands


def test_device_profile_is_clamped(ctx, signals, singles):
    """device-pointer calls cannot be checked on the host: the kernels clamp the index into the bank"""
    import torch
    y = torch.from_numpy(np.ascontiguousarray(signals)).cuda()
    out = torch.zeros_like(y)
    prof = torch.tensor([0, 1, 2, 3, 700, -5], dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.nr_reduce_bank_dev(y.data_ptr(), 6, cond_ref.L, cond_ref.L, out.data_ptr(), prof.data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    for i, p in enumerate((0, 1, 2, 2, 2, 0)):
        assert got[i].tobytes() == singles[p][i].tobytes(), (i, p)
