"""CPU: the numpy restatement of the layered mix against CPython's audioop.add, pydub's slice arithmetic
at the pinned values, and the plan / scoring helpers of mmla_audio_amd.data_augmentation."""
import audioop
import random

import numpy as np
import pytest

import mix_ref
from mmla_audio_amd import _lib, data_augmentation as da


def audioop_chain(canvas, layers):
    """pydub's overlay body on bytes: seg1[:pos] + audioop.add(seg1[pos : pos + n], seg2[:n], 2) + rest"""
    data = np.asarray(canvas, '<i2').tobytes()
    for src, pos in layers:
        head, tail = data[:2 * pos], data[2 * pos:]
        s2 = np.asarray(src, '<i2').tobytes()[:len(tail)]
        data = head + audioop.add(tail[:len(s2)], s2, 2) + tail[len(s2):]
    return np.frombuffer(data, '<i2')


def grid(seed=20261020, cases=300):
    rng = np.random.default_rng(seed)
    for _ in range(cases):
        n = int(rng.choice([17, 4801, 5003, 24000]))
        amp = int(rng.choice([3000, 20000, 32767]))
        canvas = rng.integers(-amp - 1, amp + 1, n).astype(np.int16)
        layers = []
        for _ in range(int(rng.integers(1, 5))):
            m = int(rng.choice([1, 7, 1600, 24000, 40000]))
            layers.append((rng.integers(-amp - 1, amp + 1, m).astype(np.int16), int(rng.integers(0, n + 3))))
        yield canvas, layers


def test_chain_is_the_audioop_add_chain():
    saturating = order_dependent = 0
    for canvas, layers in grid():
        got = mix_ref.chain(canvas, layers)
        assert np.array_equal(got, audioop_chain(canvas, layers))
        tot, clipped = mix_ref.clipped_sum(canvas, layers)
        saturating += bool((tot > 32767).any() or (tot < -32768).any())
        order_dependent += not np.array_equal(clipped, got)
    # the grid must reach what makes the chain a chain: saturation, and an order that matters
    assert saturating >= 1 and order_dependent >= 1
    assert audioop_chain([-32768, 32767], [([-1, 1], 0)]).tolist() == [-32768, 32767]


def test_mix_of_a_plan_is_the_chain():
    rng = np.random.default_rng(3)
    pool = rng.integers(-32768, 32768, 5000).astype(np.int16)
    plan = _lib.MixPlan.from_layers([[(0, 1000, 0), (1001, 300, 900), (7, 2000, 0)], [(4000, 1000, 0)]])
    out, out_len = mix_ref.mix(pool, plan, 1200)
    assert out_len.tolist() == [1000, 1000]
    assert np.array_equal(out[0, :1000], audioop_chain(pool[:1000], [(pool[1001:1301], 900), (pool[7:2007], 0)]))
    assert np.array_equal(out[1, :1000], pool[4000:]) and not out[:, 1000:].any()


@pytest.mark.parametrize('F,frames', [(17, 16), (3999, 3999), (4001, 4000), (4801, 4800), (5003, 5003),
                                      (23990, 23984), (23999, 23999), (24000, 24000), (40000, 24000)])
def test_canvas_slice_table(F, frames):
    assert mix_ref.canvas_frames(F)[1] == frames
    from mmla_audio_amd.audio_segment import AudioSegment
    seg = AudioSegment(np.arange(F, dtype=np.int16), 16000)
    td = 1.5 if seg.duration_seconds > 1.5 else seg.duration_seconds
    cut = seg[:td * 1000]
    assert cut.frame_count == frames and np.array_equal(cut.data, np.arange(frames, dtype=np.int16))


def test_seeded_position_draws():
    td, _, arg = mix_ref.canvas_frames(24000)
    assert (td, arg) == (1.5, 13)
    random.seed(7)
    assert [random.randrange(arg) * 100 for _ in range(6)] == [500, 200, 600, 1000, 0, 100]
    assert [mix_ref.parse_position(ms, 16000) for ms in (500, 1200)] == [8000, 19200]


def test_short_canvas_raises_value_error(tmp_path):
    assert mix_ref.canvas_frames(4799)[2] == 0      # 0.2999 s: randrange(0)
    from mmla_audio_amd.audio_segment import AudioSegment
    paths = []
    for i, n in enumerate((4799, 24000)):
        paths.append(str(tmp_path / f'u{i}.wav'))
        AudioSegment(np.zeros(n, np.int16), 16000).export(paths[-1])
    with pytest.raises(ValueError):
        da.generate_overlap_segment(paths, str(tmp_path / 'mix.wav'))


def test_overlap_plan():
    lens = [24000 * 5 + 17, 24000 * 3, 100, 24000 * 2, 24000 * 4, 24000, 24000 * 2]
    speaker_of = [0, 1, 2, 3, 4, 5, 0]
    plan, labels, talkers = da.overlap_plan(lens, speaker_of, 200, 60, random.Random(5))
    again = da.overlap_plan(lens, speaker_of, 200, 60, random.Random(5))
    for a, b in zip(plan, again[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(labels, again[1]) and np.array_equal(talkers, again[2])
    other = da.overlap_plan(lens, speaker_of, 200, 60, random.Random(6))[0]
    assert not np.array_equal(plan.src_off, other.src_off)

    assert labels.tolist() == [1] * 200 + [0] * 60
    assert np.array_equal(talkers, plan.n_layers)
    # 50 / 30 / 15 / 5 % of the overlapped clips with 2 / 3 / 4 / 5 talkers, single clips one layer
    assert np.bincount(talkers[:200], minlength=6).tolist() == [0, 0, 100, 60, 30, 10]
    assert (talkers[200:] == 1).all()

    starts = np.concatenate([[0], np.cumsum(lens)])
    owner = {}
    for r, sp in enumerate(speaker_of):
        for w in range(lens[r] // 24000):
            owner[int(starts[r]) + 24000 * w] = sp
    assert 2 not in owner.values()                   # speaker 2 has no whole window
    for c in range(260):
        k = int(plan.n_layers[c])
        offs = plan.src_off[c, :k].tolist()
        assert all(o in owner for o in offs)         # whole windows, inside the pool
        assert (plan.src_len[c, :k] == 24000).all() and offs[-1] + 24000 <= starts[-1]
        assert len({owner[o] for o in offs}) == k    # distinct speakers
        assert plan.pos[c, 0] == 0
        assert all(p % 1600 == 0 and 0 <= p <= 19200 for p in plan.pos[c, 1:k])
    assert len(set(plan.pos[:200, 1].tolist())) == 13


def test_overlap_plan_caps_the_degree_and_needs_two_speakers():
    plan, labels, talkers = da.overlap_plan([48000, 24000, 24000], [0, 1, 2], 40, 0, random.Random(1))
    assert np.bincount(talkers, minlength=4).tolist() == [0, 0, 20, 20]
    with pytest.raises(ValueError, match='speakers'):
        da.overlap_plan([48000, 23999], [0, 1], 4, 4, random.Random(1))
    with pytest.raises(ValueError, match='speakers'):
        da.overlap_plan([48000, 24000], [0, 0], 4, 4, random.Random(1))


def test_confusion_by_hand():
    labels = [1, 1, 1, 1, 0, 0, 0, 1]
    argmax = [1, 1, 0, 1, 0, 1, 0, 1]
    m, recall, precision = da.confusion(labels, argmax)
    assert m.tolist() == [[2, 1], [1, 4]]
    assert recall == 4 / 5 and precision == 4 / 5
    m, recall, precision = da.confusion([0, 0], [0, 0])
    assert m.tolist() == [[2, 0], [0, 0]] and np.isnan(recall) and np.isnan(precision)
    m, recall, precision = da.confusion([1, 1], [0, 0])
    assert recall == 0 and np.isnan(precision)


def test_mix_plan_from_layers_shapes():
    plan = _lib.MixPlan.from_layers([[(5, 6, 0)], [(1, 2, 0), (3, 4, 5)]])
    nl, off, ln, pos = plan.arrays()
    assert nl.dtype == np.int32 and off.dtype == np.int64 and ln.dtype == np.int32 and pos.dtype == np.int32
    assert off.shape == ln.shape == pos.shape == (2, _lib.MIX_MAX_LAYERS)
    assert nl.tolist() == [1, 2] and off[1, :2].tolist() == [1, 3] and pos[1, 1] == 5
    with pytest.raises(ValueError):
        _lib.MixPlan.from_layers([[(0, 1, 0)] * 9])
    with pytest.raises(ValueError):
        _lib.MixPlan.from_layers([[]])
