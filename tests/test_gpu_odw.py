"""OD res_blocks on odu.hip's fused block kernel with two strips per workgroup sharing one weight
stream against the same kernel with one strip (env MMLA_NO_ODW=1): byte for byte at every block output of
stages 4-9 (debug trace) and at od_forward's probabilities.  The network fixes the kernels' shapes,
so the clip count is the only size there is: n = 1 gives odd strip totals in blocks 7-9 (19 and 5
strips per clip), so the last workgroup's second strip does not exist; n = 2 makes a workgroup's
pair straddle two clips; n = 3 does both.  Also the u8 image entry, the range guard tripped inside a
128-channel block, and the launch plan (one conv launch per block, the same booked work)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLIPS = (1, 2, 3)
STAGES = tuple(range(4, 10))


def od_input(n):
    return np.random.default_rng(9).integers(0, 256, (n, 128, 151, 3)).astype(np.float32)


def _ctx(monkeypatch, odw, packed):
    from mmla_audio_amd import _lib, weights
    monkeypatch.setenv('MMLA_NO_ODW', '0' if odw else '1')
    c = _lib.Context(0)
    monkeypatch.delenv('MMLA_NO_ODW')
    c.load_weights(weights.OD, packed, 2)
    return c


@pytest.fixture(scope='module')
def pair():
    """(default context, MMLA_NO_ODW=1 context) with the same seeded synthetic weights"""
    from mmla_audio_amd import weights
    packed = weights.pack(weights.OD, weights.synthetic(weights.OD, seed=8))
    mp = pytest.MonkeyPatch()
    try:
        yield _ctx(mp, True, packed), _ctx(mp, False, packed)
    finally:
        mp.undo()


@pytest.mark.parametrize('n', CLIPS)
def test_blocks_4_to_9_and_probs_equal_odu_byte_for_byte(pair, n):
    new, ref = pair
    x = od_input(n)
    for stage in STAGES:
        a, b = new.debug_od_trace(x, stage), ref.debug_od_trace(x, stage)
        assert np.isfinite(b).all(), stage
        assert a.tobytes() == b.tobytes(), (n, stage, float(np.abs(a - b).max()))
    pa, pb = new.od_forward(x), ref.od_forward(x)
    assert np.isfinite(pb).all()
    assert pa.tobytes() == pb.tobytes()
    assert new.range_check() == 0 and ref.range_check() == 0


@pytest.mark.parametrize('n', CLIPS)
def test_u8_entry_gives_the_float_entry_bits(pair, n):
    new, ref = pair
    x = od_input(n)
    p8 = new.od_forward(x.astype(np.uint8))
    assert p8.tobytes() == new.od_forward(x).tobytes()
    assert p8.tobytes() == ref.od_forward(x.astype(np.uint8)).tobytes()


@pytest.mark.parametrize('lww,cin', [(27, 64), (32, 128)], ids=['block7', 'block8'])
def test_range_guard_trips_in_a_128_channel_block(monkeypatch, lww, cin):
    """layer_with_weights-27 / -32 are the first BatchNorms of blocks 7 and 8 (the 128-channel
    stage): x 1e5 puts the block's staged conv input (x 2^4) past the fp16 range; the guard trips and
    the host call re-runs the micro-batch in exact f32, so the result is the exact-f32 context's"""
    from mmla_audio_amd import _lib, weights
    from oracle import synth
    W = weights.synthetic(weights.OD, seed=8)
    g = f'layer_with_weights-{lww}/gamma'
    assert W[g].shape == (cin,)
    W[g] = W[g] * 1.0e5
    W[f'layer_with_weights-{lww}/beta'] = np.abs(W[f'layer_with_weights-{lww}/beta']) * 1.0e5
    packed = weights.pack(weights.OD, W)
    pcm = synth.batch(360, 3, 40000)
    c = _ctx(monkeypatch, True, packed)
    p, a, _ = c.od_pipeline(pcm)
    assert c.range_check() >= 1
    ref = _ctx(monkeypatch, True, packed)
    ref.set_precision(_lib.PREC_F32)
    p32, a32, _ = ref.od_pipeline(pcm)
    assert np.all(np.isfinite(p))
    assert np.array_equal(p, p32) and np.array_equal(a, a32)


def test_launch_plan_is_odu_s(pair):
    """per stage: the same launch counts and booked work with and without odw (one conv launch per
    block either way; tests/test_gpu_launch_plan.py holds the absolute numbers)"""
    from oracle import synth
    pcm = synth.batch(3300, 3, 40000)
    plans = []
    for c in pair:
        c.profile_enable()
        c.profile_read()
        c.od_pipeline(pcm)
        got = c.profile_read()
        c.profile_enable(False)
        plans.append({s: (got[s][1], got[s][2]) for s in got})
    print(plans[0])
    assert plans[0]['conv'][0] == 9
    assert plans[0] == plans[1]
