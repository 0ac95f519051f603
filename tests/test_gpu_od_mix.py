"""GPU: mmla_od_mix against the audioop.add chain bit for bit (host and device pointers, aligned and
unaligned rows, nothing stored outside [0, clip_len) of a row), the plan checks of host-pointer calls,
mmla_od_pipeline_mixed against mmla_od_pipeline on the mixed clips, and the pydub drop-ins
(AudioSegment.overlay, generate_overlap_segment) against the restatement in tests/mix_ref.py."""
import random

import numpy as np
import pytest

import mix_ref
from mmla_audio_amd import _lib, data_augmentation, weights
from mmla_audio_amd.audio_segment import AudioSegment, _read_wav

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a
POOL_LEN = 130001
CANVAS = (24000, 23999, 4001, 3999, 17, 1)
SRC_LENS = (1, 7, 24000, 40000)


def _positions(cl):
    return (0, 1, 7, 8, 1600, cl - 1, cl, cl + 5)


def _plan(clip_len, canvas_lens):
    """every canvas length with 1 .. 8 layers; positions and source lengths cycle through their lists, the
    pool offsets are odd (and even) and the pool is full-scale noise, so most sums saturate"""
    rng = np.random.default_rng(24000 + clip_len)
    clips = []
    for i, (cl, nl) in enumerate((cl, nl) for nl in range(1, 9) for cl in canvas_lens):
        layers = [(int(rng.integers(0, POOL_LEN - cl)) | 1, cl, 0)]
        for l in range(1, nl):
            m = SRC_LENS[(i + l) % 4]
            off = int(rng.integers(0, POOL_LEN - m))
            layers.append((off | 1 if l % 3 else off & ~1, m, _positions(min(cl, clip_len))[(i + 3 * l) % 8]))
        clips.append(layers)
    return _lib.MixPlan.from_layers(clips)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def pool():
    p = np.random.default_rng(77).integers(-32768, 32768, POOL_LEN).astype(np.int16)
    p.setflags(write=False)
    return p


@pytest.fixture(scope='module')
def cases(pool):
    """clip_len -> (plan, out_stride, reference clips by the audioop chain, reference lengths)"""
    out = {}
    for clip_len, stride, canvas_lens in ((24000, 24008, CANVAS), (4801, 4811, (4801, 4800, 5003, 17, 1))):
        plan = _plan(clip_len, canvas_lens)
        want, want_len = mix_ref.mix(pool, plan, clip_len, chain=mix_ref.audioop_chain)
        assert np.array_equal(want, mix_ref.mix(pool, plan, clip_len)[0])
        want.setflags(write=False)
        out[clip_len] = (plan, stride, want, want_len)
    return out


def test_reference_saturates_and_depends_on_order(pool, cases):
    plan, _, want, _ = cases[24000]
    c = 5 * len(CANVAS)          # a clip of 6 layers on a 24000-sample canvas
    assert plan.n_layers[c] == 6 and plan.src_len[c, 0] == 24000
    o = int(plan.src_off[c, 0])
    layers = [(pool[int(plan.src_off[c, l]):int(plan.src_off[c, l]) + int(plan.src_len[c, l])], int(plan.pos[c, l]))
              for l in range(1, 6)]
    tot, clipped = mix_ref.clipped_sum(pool[o:o + 24000], layers)
    assert (np.abs(tot) > 32768).any() and not np.array_equal(clipped, want[c])


def _check_rows(got, got_len, want, want_len, clip_len):
    assert got_len.tolist() == want_len.tolist()
    assert got[:, :clip_len].tobytes() == want.tobytes()
    for c, n in enumerate(want_len):
        assert not got[c, n:clip_len].any(), c                       # zeros behind the canvas
    assert (got[:, clip_len:] == SENTINEL).all()                     # the stride padding is untouched


@pytest.mark.parametrize('clip_len', [24000, 4801])
def test_od_mix_device_pointers(ctx, pool, cases, clip_len):
    """24000 with rows 16 bytes apart from aligned (the 16-byte stores); 4801 with an odd stride, so rows
    start at every alignment and end inside a thread's 8 samples"""
    import torch
    plan, stride, want, want_len = cases[clip_len]
    n = len(plan.n_layers)
    # the pool at an odd sample of its allocation: 2-byte aligned sources and nothing better
    dpool = torch.zeros(POOL_LEN + 1, dtype=torch.int16, device='cuda')
    dpool[1:] = torch.from_numpy(np.array(pool)).cuda()
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in plan.arrays()]
    out = torch.full((n, stride), SENTINEL, dtype=torch.int16, device='cuda')
    out_len = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.od_mix_dev(dpool.data_ptr() + 2, POOL_LEN, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                   d[3].data_ptr(), out.data_ptr(), stride, clip_len, out_len.data_ptr())
    ctx.synchronize()
    _check_rows(out.cpu().numpy(), out_len.cpu().numpy(), want, want_len, clip_len)


@pytest.mark.parametrize('clip_len', [24000, 4801])
def test_od_mix_host_pointers(ctx, pool, cases, clip_len):
    plan, stride, want, want_len = cases[clip_len]
    nl, off, ln, pos = plan.arrays()
    n = nl.size
    out = np.full((n, stride), SENTINEL, np.int16)
    out_len = np.full(n, -7, np.int32)
    rc = ctx.lib.mmla_od_mix(ctx.h, pool.ctypes.data, POOL_LEN, n, nl.ctypes.data, off.ctypes.data, ln.ctypes.data,
                             pos.ctypes.data, clip_len, out.ctypes.data, stride, out_len.ctypes.data, 0)
    assert rc == 0, ctx.lib.mmla_last_error(ctx.h)
    _check_rows(out, out_len, want, want_len, clip_len)
    got, got_len = ctx.od_mix(pool, plan, clip_len)
    assert got.tobytes() == want.tobytes() and got_len.tolist() == want_len.tolist()


def test_a_clip_does_not_depend_on_its_place_in_the_batch(ctx, pool):
    rng = np.random.default_rng(9)
    one = [(4001, 24000, 0)] + [(int(rng.integers(0, 90000)) | 1, 24000, 1600 * l + l) for l in range(1, 8)]
    filler = [[(int(rng.integers(0, 90000)), 20000 + c, 0), (c, 24000, 8 * c)] for c in range(5)]
    out, out_len = ctx.od_mix(pool, _lib.MixPlan.from_layers([one] + filler + [one]))
    assert out[0].tobytes() == out[-1].tobytes() and out_len[0] == out_len[-1] == 24000
    assert out[0].tobytes() == mix_ref.mix(pool, _lib.MixPlan.from_layers([one]), 24000)[0].tobytes()


def test_host_plans_are_checked_before_any_launch(pool):
    c = _lib.Context(0)
    try:
        c.profile_enable(True)
        good = [[(0, 100, 0)], [(10, 100, 0), (300, 50, 20), (500, 60, 30)]]

        def broken(layer, clip=1, at=2):
            clips = [list(x) for x in good]
            clips[clip][at] = layer
            return _lib.MixPlan.from_layers(clips)

        few = _lib.MixPlan.from_layers(good)._replace(n_layers=np.array([1, 0], np.int32))
        many = _lib.MixPlan.from_layers(good)._replace(n_layers=np.array([1, 9], np.int32))
        bad = [(few, 'clip 1', 'layers'), (many, 'clip 1', 'layers'),
               (broken((-1, 60, 30)), 'clip 1 layer 2', 'offset'),
               (broken((500, -60, 30)), 'clip 1 layer 2', 'length'),
               (broken((500, 60, -30)), 'clip 1 layer 2', 'position'),
               (broken((POOL_LEN - 59, 60, 30)), 'clip 1 layer 2', 'pool'),
               (broken((POOL_LEN - 99, 100, 0), clip=0, at=0), 'clip 0 layer 0', 'pool')]
        for plan, where, what in bad:
            for call in (c.od_mix, c.od_pipeline_mixed):      # (the plan is checked before the weights)
                with pytest.raises(_lib.MmlaError) as e:
                    call(pool, plan)
                assert e.value.code == -1 and where in str(e.value) and what in str(e.value), str(e.value)
        assert all(v[1] == 0 for v in c.profile_read().values())      # not one launch so far
        out, out_len = c.od_mix(pool, broken((POOL_LEN - 60, 60, 30)))  # the last samples of the pool
        assert out_len.tolist() == [100, 100]
        assert c.profile_read()['glue'][1] == 1
    finally:
        c.close()


def test_fused_call_equals_od_pipeline_on_the_mixed_clips(pool):
    import torch
    rng = np.random.default_rng(21)
    clips = []
    for i in range(21):         # 21 clips under set_microbatch(od=8): 8 + 8 + 5
        cl = (24000, 24000, 23999, 4001, 3999, 12000, 17)[i % 7]
        layers = [(int(rng.integers(0, 100000)) | 1, cl, 0)]
        for l in range(i % 5):
            layers.append((int(rng.integers(0, 90000)), (24000, 40000, 7, 1600)[(i + l) % 4],
                           int(rng.integers(0, 13)) * 1600))
        clips.append(layers)
    plan = _lib.MixPlan.from_layers(clips)
    quiet = (np.array(pool) // 4).astype(np.int16)      # overlays that do not all saturate
    c = _lib.Context(0)
    try:
        c.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=5)), 2)
        c.set_microbatch(od=8)
        mixed, out_len = c.od_mix(quiet, plan)
        assert mixed.tobytes() == mix_ref.mix(quiet, plan, 24000)[0].tobytes()
        want = c.od_pipeline(mixed, out_len)
        got = c.od_pipeline_mixed(quiet, plan)
        for g, w, name in zip(got, want, ('probs', 'argmax', 'silent')):
            assert g.tobytes() == w.tobytes(), name
        assert got[2].tolist() == (out_len < 4000).tolist() and got[2].any() and not got[2].all()
        assert (got[1][got[2]] == -1).all() and (got[1][~got[2]] >= 0).all()
        # ... and under device pointers
        dpool = torch.from_numpy(quiet).cuda()
        d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in plan.arrays()]
        probs = torch.zeros((21, 2), dtype=torch.float32, device='cuda')
        am = torch.zeros(21, dtype=torch.int32, device='cuda')
        silent = torch.zeros(21, dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()
        c.od_pipeline_mixed_dev(dpool.data_ptr(), POOL_LEN, 21, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                d[3].data_ptr(), probs.data_ptr(), am.data_ptr(), silent.data_ptr())
        c.synchronize()
        assert probs.cpu().numpy().tobytes() == want[0].tobytes()
        assert am.cpu().numpy().tolist() == want[1].tolist()
        assert silent.cpu().numpy().astype(bool).tolist() == want[2].tolist()
    finally:
        c.close()


def test_pool_and_plan_outlive_a_repeated_micro_batch(monkeypatch, pool):
    """MMLA_DEBUG_FAIL_ALLOC=1 fails a context's first workspace allocation, which falls into the first
    micro-batch behind the upload of the pool and the plan.  Only a micro-batch of more than 64 clips is
    halved, so the call has 66 clips (-> 64 + 2): the workspace is released, the micro-batch repeated, and it
    must find the pool and the plan where the call put them.  The hook is spent by the call it fails, so that
    it is live in this path is shown on a second context made under it: 6 clips, too few to halve, report it."""
    rng = np.random.default_rng(66)
    clips = []
    for i in range(66):
        cl = (24000, 23999, 4001, 3999, 12000, 17)[i % 6]
        clips.append([(int(rng.integers(0, 100000)) | 1, cl, 0)] +
                     [(int(rng.integers(0, 90000)), (24000, 40000, 7, 1600)[(i + l) % 4], int(rng.integers(0, 13)) * 1600)
                      for l in range(i % 4)])
    plan = _lib.MixPlan.from_layers(clips)
    quiet = (np.array(pool) // 4).astype(np.int16)
    packed = weights.pack(weights.OD, weights.synthetic(weights.OD, seed=5))
    monkeypatch.setenv('MMLA_DEBUG_FAIL_ALLOC', '1')
    dbg, small = _lib.Context(0), _lib.Context(0)
    monkeypatch.delenv('MMLA_DEBUG_FAIL_ALLOC')
    plain = _lib.Context(0)
    try:
        for c in (dbg, small, plain):
            c.load_weights(weights.OD, packed, 2)
        with pytest.raises(_lib.MmlaError) as e:
            small.od_pipeline_mixed(quiet, _lib.MixPlan.from_layers(clips[:6]))
        assert e.value.code == -4, e.value
        got = dbg.od_pipeline_mixed(quiet, plan)
        want = plain.od_pipeline_mixed(quiet, plan)
        for g, w, name in zip(got, want, ('probs', 'argmax', 'silent')):
            assert g.tobytes() == w.tobytes(), name
        assert np.isfinite(got[0]).all() and got[2].any() and not got[2].all()
    finally:
        for c in (dbg, small, plain):
            c.close()


def test_overlay_drop_in(ctx, pool):
    canvas = np.array(pool[1:5004])               # 5003 frames: 312.6875 ms, pydub's len() is 313
    seg = np.array(pool[20001:21601])
    short = np.array(pool[40001:40301])
    a = AudioSegment(canvas, 16000, ctx=ctx)
    for kw, times in ((dict(), 1), (dict(times=3), 3), (dict(loop=True), -1)):
        got = a.overlay(AudioSegment(seg, 16000, ctx=ctx), position=100, **kw)
        want = mix_ref.overlay(canvas, seg, 100, 16000, times)
        assert got.data.tobytes() == want.tobytes() and got.frame_count == 5008, kw
    # 12 repeats: more layers than one call takes
    got = a.overlay(AudioSegment(short, 16000, ctx=ctx), position=100, loop=True)
    assert got.data.tobytes() == mix_ref.overlay(canvas, short, 100, 16000, -1).tobytes()
    assert not np.array_equal(got.data[1600:5003], canvas[1600:5003])
    # a position at and past the end, times=0, and the gain that is not built
    whole = AudioSegment(np.array(pool[:24000]), 16000, ctx=ctx)
    for position in (1500, 1700):
        assert whole.overlay(AudioSegment(seg, 16000, ctx=ctx), position=position).data.tobytes() == \
            whole.data.tobytes()
    assert whole.overlay(AudioSegment(seg, 16000, ctx=ctx), times=0).data.tobytes() == whole.data.tobytes()
    with pytest.raises(NotImplementedError):
        whole.overlay(AudioSegment(seg, 16000, ctx=ctx), gain_during_overlay=-6)


def test_generate_overlap_segment_drop_in(ctx, pool, tmp_path):
    utterances = [np.array(pool[1:40001]), np.array(pool[50001:80001]), np.array(pool[90000:95003]),
                  np.array(pool[100000:124000])]
    paths = []
    for i, u in enumerate(utterances):
        paths.append(str(tmp_path / f'u{i}.wav'))
        AudioSegment(u, 16000).export(paths[-1])
    out = str(tmp_path / 'overlap.wav')
    random.seed(7)
    data_augmentation.generate_overlap_segment(paths, out, ctx=ctx)
    rate, nch, width, x = _read_wav(out)
    assert (rate, nch, width) == (16000, 1, 2)
    want = mix_ref.overlap_segment(utterances, [500, 200, 600])
    assert len(want) == 24000 and x.tobytes() == want.tobytes()
    assert random.randrange(13) * 100 == 1000       # three draws were taken, as the reference takes them
