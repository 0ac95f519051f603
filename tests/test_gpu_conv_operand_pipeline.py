"""The conv kernels' LDS operand pipeline (rbs.hip, odu.hip: MFMA fragments fetched a k-step ahead)
only reorders instructions, so every OD block output and the probabilities keep the bits of the
commit before it.  tests/golden/od_trace_r6_sha256.json holds the SHA-256 of the nine block outputs
(debug trace stages 1-9) and of od_forward's probabilities as that commit computed them on an MI355X
for the inputs below; n = 1 and n = 3 clips cross the strip / XCD block ordering with a ragged
count (the kernels' shapes are fixed by the network, the clip count is the only size there is).
Also: the u8 image entry (block 1's u8 staging shares the changed loops) gives the float entry's
bits, and the range guard still trips when block 2's BatchNorm drives its conv input past 65504."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'od_trace_r6_sha256.json')
CLIPS = (1, 3)
STAGES = tuple(range(1, 10))


def od_input(n):
    return np.random.default_rng(9).integers(0, 256, (n, 128, 151, 3)).astype(np.float32)


def od_context():
    from mmla_audio_amd import _lib, weights
    c = _lib.Context(0)
    c.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=8)), 2)
    return c


def od_hashes(c, n):
    """{'stage1' .. 'stage9', 'probs'} -> SHA-256 hex of the tensor's bytes, for n clips"""
    x = od_input(n)
    out = {f'stage{s}': hashlib.sha256(c.debug_od_trace(x, s).tobytes()).hexdigest() for s in STAGES}
    out['probs'] = hashlib.sha256(c.od_forward(x).tobytes()).hexdigest()
    return out


@pytest.fixture(scope='module')
def ctx():
    return od_context()


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('n', CLIPS)
def test_block_outputs_and_probs_keep_the_parent_bits(ctx, golden, n):
    got = od_hashes(ctx, n)
    want = golden[f'n{n}']
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(got) if got[k] != want[k]]
    assert not bad, f'n={n}: bits differ from the parent commit in {bad}'


@pytest.mark.parametrize('n', CLIPS)
def test_u8_entry_gives_the_float_entry_bits(ctx, n):
    x = od_input(n)
    pf, p8 = ctx.od_forward(x), ctx.od_forward(x.astype(np.uint8))
    assert np.isfinite(pf).all()
    assert pf.tobytes() == p8.tobytes()


def test_range_guard_trips_in_block_2():
    """layer_with_weights-6 is block 2's first BatchNorm: x 1e5 puts its ELU output (x 2^4) past the
    fp16 range in rbs.hip's staging split; the host call re-runs the micro-batch in exact f32"""
    from mmla_audio_amd import _lib, weights
    from oracle import synth
    W = weights.synthetic(weights.OD, seed=8)
    W['layer_with_weights-6/gamma'] = W['layer_with_weights-6/gamma'] * 1.0e5
    W['layer_with_weights-6/beta'] = np.abs(W['layer_with_weights-6/beta']) * 1.0e5
    pcm = synth.batch(360, 4, 40000)
    c = _lib.Context(0)
    c.load_weights(weights.OD, weights.pack(weights.OD, W), 2)
    p, a, _ = c.od_pipeline(pcm)
    assert c.range_check() >= 1
    ref = _lib.Context(0)
    ref.load_weights(weights.OD, weights.pack(weights.OD, W), 2)
    ref.set_precision(_lib.PREC_F32)
    p32, a32, _ = ref.od_pipeline(pcm)
    assert np.all(np.isfinite(p))
    assert np.array_equal(p, p32) and np.array_equal(a, a32)
