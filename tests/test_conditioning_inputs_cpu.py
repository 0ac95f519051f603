"""CPU: conditions on the inputs of the conditioning tests (tests/cond_ref.py), by the CPU oracles
(oracle.noisereduce, ssim_ref.pcm16, oracle.vad with oracle.webrtc_vad.Vad(3) carried over the six
clips): the GPU tests compare fused against composed calls bit for bit, which only means something if
the clips take every branch -- kept nearly whole, shortened, emptied -- and the profiles differ."""
import numpy as np
import pytest

import cond_ref


@pytest.fixture(scope='module')
def kept():
    x = cond_ref.clips()
    return {p: cond_ref.oracle_kept(x, p) for p in (0, 1, 2, None)}


def test_kept_lengths_are_the_record(kept):
    print(kept)
    assert kept == cond_ref.KEPT      # a record: if a transcription detail moves it, update KEPT


def test_branch_coverage(kept):
    L = cond_ref.L
    for p in (0, 1, 2):
        k = np.array(kept[p])
        assert (k % 480 == 0).all()
        # profile 2 (16 x the clips' own noise level) shortens even the fully voiced clip 0 -- the
        # recorded lengths say so themselves; the 'kept nearly whole' branch is taken under 0 and 1
        if p < 2:
            assert (k >= L - 480).any(), (p, 'a clip kept nearly whole')
        assert ((k >= 4800) & (k <= L - 4800)).any(), (p, 'a shortened clip')
        assert (k == 0).any(), (p, 'an emptied clip')
        # the collector never keeps fewer than 10 frames: '< 4000 samples' with a non-empty clip needs lens
        assert ((k == 0) | (k >= 4800)).all()
        assert k[3] == 0 and k[4] == 0        # noise alone and digital zeros
    assert len({kept[0], kept[1], kept[2]}) == 3, 'the three profiles keep different lengths'
    assert kept[0] != kept[None], 'the gate changes a length'


def test_inputs_are_what_the_recipe_says():
    x = cond_ref.clips()
    assert x.shape == (6, cond_ref.L) and x.dtype == np.int16
    assert not x[4].any() and x[3].any()
    for p in range(cond_ref.N_PROFILES):
        n = cond_ref.noise(p)
        assert n.dtype == np.float32 and n.shape == (16000,)
        assert abs(float(n.std()) / (4 ** p * cond_ref.LV) - 1) < 0.02
