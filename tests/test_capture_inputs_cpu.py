"""CPU: the capture audio of tests/test_gpu_capture.py exercises both outcomes of the silent rule.

The GPU test compares the fused capture tick with Room.tick on the restatement's converted clips and
asserts ``silent.any() and not silent.all()`` on every tick.  That is a condition on the inputs: here the
CPU oracles (stationary gate, PCM_16, webrtc Vad(3) per stream, carried over the two ticks) run on the
restatement's conversion alone and must give kept lengths on both sides of 4000 samples, with the gate
(each stream against its own noise profile) and without it.
"""
import numpy as np
import pytest

import capture_inputs as ci
import capture_ref
import cond_ref


def test_held_48k_converts_to_the_16k_clips():
    (t0, l0), (t1, l1) = ci.restated('48k_stereo')[0]
    x0, x1 = ci.ticks16k()
    assert np.array_equal(t0, x0) and np.array_equal(t1, x1)
    assert (l0 == cond_ref.L).all() and (l1 == cond_ref.L).all()
    assert capture_ref.out_clip_len(ci.FRAMES_48K, 48000) == cond_ref.L
    assert capture_ref.out_clip_len(ci.FRAMES_441, 44100) == cond_ref.L


@pytest.mark.parametrize('gate', [True, False])
@pytest.mark.parametrize('case', sorted(ci.CASES))
def test_both_outcomes_of_the_silent_rule(case, gate):
    converted, conv = ci.restated(case)
    dets = ci.detectors()
    profiles = np.arange(ci.N) // ci.IPS if gate else None
    for t, (q, lens) in enumerate(converted):
        kept = ci.oracle_kept(q, lens, profiles, dets)
        silent = kept < 4000
        print(case, 'gate' if gate else 'no gate', 'tick', t, 'out_lens', lens.tolist(), 'kept', kept.tolist())
        assert silent.any() and not silent.all(), (case, gate, t, kept)
    for d, _ in conv.states:
        ir, orr = capture_ref.reduced(ci.CASES[case][0][0])
        assert -max(ir, orr) <= d < 0
