"""OD res_blocks 2-3 on the strip kernel that keeps GEMM 1's weights in LDS (rbs_w1l.hip, the default)
against the strip kernel that streams them from global memory every chunk (rbs.hip, env
MMLA_NO_RBS_W1L=1).  Both run the same MFMA sequence per accumulator, so the block outputs (debug trace
stages 2 and 3) and the probabilities agree byte for byte.  The network fixes the kernel's shape, so
the clip count is the only size there is: n = 1, 2, 3 clips are 5, 10 and 15 workgroups, which cover
the first and the last strip of a clip (their out-of-image columns differ: image column -1, and
columns 76-79) and the XCD remap of the workgroup ids with a remainder (5 % 8, 10 % 8, 15 % 8).
The range guard trips inside the new kernel (block 2's staging split, block 2's t1 split, block 3's
staging split) and a device-pointer call reports MMLA_E_RANGE."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLIPS = (1, 2, 3)


def od_images(n):
    return np.random.default_rng(14).integers(0, 256, (n, 128, 151, 3)).astype(np.uint8)


def _ctx(monkeypatch, w1l, packed):
    from mmla_audio_amd import _lib, weights
    monkeypatch.setenv('MMLA_NO_RBS_W1L', '0' if w1l else '1')
    c = _lib.Context(0)
    monkeypatch.delenv('MMLA_NO_RBS_W1L')
    c.load_weights(weights.OD, packed, 2)
    return c


@pytest.fixture(scope='module')
def pair():
    """(default context, MMLA_NO_RBS_W1L=1 context) with the same seeded synthetic weights"""
    from mmla_audio_amd import weights
    packed = weights.pack(weights.OD, weights.synthetic(weights.OD, seed=14))
    mp = pytest.MonkeyPatch()
    try:
        yield _ctx(mp, True, packed), _ctx(mp, False, packed)
    finally:
        mp.undo()


@pytest.mark.parametrize('n', CLIPS)
def test_blocks_2_3_and_probs_equal_global_weight_kernel_byte_for_byte(pair, n):
    from oracle import synth
    new, ref = pair
    img = od_images(n)
    x = img.astype(np.float32)
    for stage in (2, 3):
        a, b = new.debug_od_trace(x, stage), ref.debug_od_trace(x, stage)
        assert np.isfinite(b).all() and float(np.abs(b).max()) > 0.0, stage
        assert a.tobytes() == b.tobytes(), (n, stage, float(np.abs(a - b).max()))
    pa, pb = new.od_forward(img), ref.od_forward(img)
    assert np.isfinite(pb).all()
    assert pa.tobytes() == pb.tobytes()
    pcm = synth.batch(1400 + n, n, 40000)
    qa, la, _ = new.od_pipeline(pcm)
    qb, lb, _ = ref.od_pipeline(pcm)
    assert np.isfinite(qb).all()
    assert qa.tobytes() == qb.tobytes() and la.tobytes() == lb.tobytes()
    assert new.range_check() == 0 and ref.range_check() == 0


def test_launch_plan_is_the_global_weight_kernel_s(pair):
    """one conv launch per block and the same booked work with either kernel
    (tests/test_gpu_launch_plan.py holds the absolute numbers)"""
    from oracle import synth
    pcm = synth.batch(1400, 3, 40000)
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


# the BatchNorms whose output the new kernel splits: layer_with_weights-6 / -8 are block 2's first and
# second (its staging split and its t1 split), -10 is block 3's first (block 1 holds layers 1-5)
@pytest.mark.parametrize('lww', [6, 8, 10], ids=['block2_x', 'block2_t1', 'block3_x'])
def test_range_guard_device_call_reports_range(monkeypatch, lww):
    """the BatchNorm x 1e5 puts the ELU output (x 2^4) past the fp16 range where the new kernel splits
    it; everything before that split is in range, so the first kernel to flag it is the new one.  A
    device-pointer call reports MMLA_E_RANGE once; a host call re-runs in exact f32"""
    import torch
    from mmla_audio_amd import _lib, weights
    from oracle import synth
    W = weights.synthetic(weights.OD, seed=14)
    g, b = f'layer_with_weights-{lww}/gamma', f'layer_with_weights-{lww}/beta'
    assert W[g].shape == (32,)
    W[g] = W[g] * 1.0e5
    W[b] = np.abs(W[b]) * 1.0e5
    packed = weights.pack(weights.OD, W)
    c = _ctx(monkeypatch, True, packed)
    host = synth.batch(1410, 3, 40000)
    pcm = torch.from_numpy(host).cuda()
    probs = torch.empty((3, 2), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    c.od_pipeline_dev(pcm.data_ptr(), 3, 40000, 40000, probs.data_ptr())
    with pytest.raises(_lib.MmlaError) as e:
        c.range_check()
    assert e.value.code == _lib.MMLA_E_RANGE
    assert c.range_check() == 0                   # reported once, then cleared
    p, a, _ = c.od_pipeline(host)
    assert c.range_check() >= 1
    ref = _ctx(monkeypatch, True, packed)
    ref.set_precision(_lib.PREC_F32)
    p32, a32, _ = ref.od_pipeline(host)
    assert np.all(np.isfinite(p))
    assert np.array_equal(p, p32) and np.array_equal(a, a32)
