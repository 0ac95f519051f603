"""OD res_block 1 on the strip kernel that pairs the clips' 7-column last strips (rbs_tp.hip, the default)
against the strip kernel that gives each of them a workgroup of its own (rbs.hip, env
MMLA_NO_RBS_TAILPAIR=1).  Only the column tables differ, so block 1's output (debug trace stage 1), the
network's probabilities and the pipeline's argmax agree byte for byte, for the u8 image and the float
image.  The network fixes the kernel's shape, so the clip count is the only size there is: n = 1 is an
unpaired tail alone (the pair's second clip absent), n = 2 one full pair, n = 3 and 5 a full pair or two
and an unpaired tail, n = 5 with full strips and tails of different clips in one launch and workgroup
counts (10, 19, 29, 48) that leave a remainder in the XCD remap of the workgroup ids.
A pair's halves are isolated: 1e6 in image columns 143-150 of a pair's second clip changes nothing in its
first clip, which also equals the same clip run alone, and the range guard's outcome is the same under
both settings."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLIPS = (1, 2, 3, 5)


def od_images(n):
    return np.random.default_rng(15).integers(0, 256, (n, 128, 151, 3)).astype(np.uint8)


def _ctx(monkeypatch, tailpair, packed):
    from mmla_audio_amd import _lib, weights
    monkeypatch.setenv('MMLA_NO_RBS_TAILPAIR', '0' if tailpair else '1')
    c = _lib.Context(0)
    monkeypatch.delenv('MMLA_NO_RBS_TAILPAIR')
    c.load_weights(weights.OD, packed, 2)
    return c


@pytest.fixture(scope='module')
def pair():
    """(default context, MMLA_NO_RBS_TAILPAIR=1 context) with the same seeded synthetic weights"""
    from mmla_audio_amd import weights
    packed = weights.pack(weights.OD, weights.synthetic(weights.OD, seed=15))
    mp = pytest.MonkeyPatch()
    try:
        yield _ctx(mp, True, packed), _ctx(mp, False, packed)
    finally:
        mp.undo()


def _range_outcome(c):
    """the range guard's report since the last one: ('ok', host re-runs so far) or ('range', code)"""
    from mmla_audio_amd import _lib
    try:
        return 'ok', c.range_check()
    except _lib.MmlaError as e:
        return 'range', e.code


@pytest.mark.parametrize('n', CLIPS)
def test_block_1_and_probs_equal_unpaired_kernel_byte_for_byte(pair, n):
    from oracle import synth
    new, ref = pair
    reruns = new.range_check(), ref.range_check()                      # host re-runs in exact f32 so far
    img = od_images(n)
    x = img.astype(np.float32)
    a, b = new.debug_od_trace(x, 1), ref.debug_od_trace(x, 1)          # float image
    assert np.isfinite(b).all() and float(np.abs(b).max()) > 0.0
    assert a.tobytes() == b.tobytes(), (n, float(np.abs(a - b).max()))
    for im in (img, x):                                                 # u8 image, float image
        pa, pb = new.od_forward(im), ref.od_forward(im)
        assert np.isfinite(pb).all()
        assert pa.tobytes() == pb.tobytes(), (n, im.dtype)
    pcm = synth.batch(1500 + n, n, 40000)                               # u8 image from the front-end
    qa, la, _ = new.od_pipeline(pcm)
    qb, lb, _ = ref.od_pipeline(pcm)
    assert np.isfinite(qb).all()
    assert qa.tobytes() == qb.tobytes() and la.tobytes() == lb.tobytes()
    assert (new.range_check(), ref.range_check()) == reruns            # nothing tripped the range guard


def test_first_clip_of_a_pair_equals_the_clip_alone(pair):
    new, _ = pair
    x = od_images(3).astype(np.float32)
    all3 = new.debug_od_trace(x, 1)
    for i in range(3):                     # clip 0: part 0 of a pair, clip 1: part 1, clip 2: unpaired
        alone = new.debug_od_trace(x[i:i + 1], 1)
        assert alone[0].tobytes() == all3[i].tobytes(), i


@pytest.mark.parametrize('victim', [0, 1], ids=['first_of_pair', 'second_of_pair'])
def test_huge_values_in_one_tail_stay_in_that_clip(pair, victim):
    """1e6 in image columns 143-150 of one clip of a pair: past the fp16 range once staged, so that clip
    trips the range guard under either setting.  The other clip of the pair must not see them (a junk
    tile column reading across the ring's halves would), and everything agrees with the unpaired kernel"""
    import torch
    from mmla_audio_amd import _lib
    new, ref = pair
    x = od_images(3).astype(np.float32)
    clean = ref.debug_od_trace(x, 1)
    x[victim, :, 143:151, :] = 1.0e6
    a, b = new.debug_od_trace(x, 1), ref.debug_od_trace(x, 1)
    assert a.tobytes() == b.tobytes()
    for i in range(3):
        if i != victim:
            assert a[i].tobytes() == clean[i].tobytes(), i
    # only the victim's pooled columns fed by image columns >= 142 may differ from the clean run
    assert a[victim, :, :70].tobytes() == clean[victim, :, :70].tobytes()
    # the range guard: a device-pointer call reports MMLA_E_RANGE under either setting ...
    xd = torch.from_numpy(x).cuda()
    got = []
    for c in (new, ref):
        c.range_check()
        p = torch.empty((3, 2), dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        c.od_forward_dev(xd.data_ptr(), 3, p.data_ptr())
        got.append((_range_outcome(c), p.cpu().numpy().tobytes()))
    assert got[0] == got[1]
    assert got[0][0] == ('range', _lib.MMLA_E_RANGE), got[0][0]
    # ... and a host call re-runs the micro-batch in exact f32, once, under either setting
    before = new.range_check(), ref.range_check()
    pa, pb = new.od_forward(x), ref.od_forward(x)
    assert pa.tobytes() == pb.tobytes()
    assert (new.range_check() - before[0], ref.range_check() - before[1]) == (1, 1)


def test_launch_plan_is_the_unpaired_kernel_s(pair):
    """one conv launch per block and the same booked work with either kernel
    (tests/test_gpu_launch_plan.py holds the absolute numbers)"""
    from oracle import synth
    pcm = synth.batch(1500, 3, 40000)
    plans = []
    for c in pair:
        c.profile_enable()
        c.profile_read()
        c.od_pipeline(pcm)
        got = c.profile_read()
        c.profile_enable(False)
        plans.append({s: (got[s][1], got[s][2]) for s in got})
    assert plans[0]['conv'][0] == 9
    assert plans[0] == plans[1]
