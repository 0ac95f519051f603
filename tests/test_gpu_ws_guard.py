"""Out-of-bounds stores: every workspace slot framed by guard bands (MMLA_WS_GUARD=1, context.cpp
ws_get); a call fails if any kernel wrote into one.  Micro-batches and batch sizes that leave
partial tiles at the end of each buffer, OD and SI pipelines, front-ends and the noise gate; the kept
slots of a capture tick and of a host-pointer mix."""
import os

import numpy as np
import pytest

from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gctx():
    from mmla_audio_amd import _lib, weights
    os.environ['MMLA_WS_GUARD'] = '1'
    try:
        c = _lib.Context(0)
        c.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=31)), 2)
        Ws = weights.synthetic(weights.SI, seed=32, n_classes=8)
        c.load_weights(weights.SI, weights.pack(weights.SI, Ws, 8), 8, 1)
        yield c
    finally:
        os.environ.pop('MMLA_WS_GUARD', None)


@pytest.mark.parametrize('mb,n', [(32, 75), (64, 150), (0, 37)])
def test_od_guards(gctx, mb, n):
    pcm = synth.batch(960 + n, n, 40000)
    gctx.set_microbatch(mb, 0)
    try:
        gctx.od_features(pcm)
        p, a, _ = gctx.od_pipeline(pcm)
    finally:
        gctx.set_microbatch(0, 0)
    assert np.isfinite(p).all()


@pytest.mark.parametrize('mb,n', [(16, 41), (0, 23)])
def test_si_guards(gctx, mb, n):
    pcm = synth.batch(970 + n, n, 24000)
    gctx.set_microbatch(0, mb)
    try:
        gctx.si_features(pcm)
        p, a, s = gctx.si_pipeline(pcm)
    finally:
        gctx.set_microbatch(0, 0)
    assert np.isfinite(p).all()


def test_noise_gate_guards(gctx):
    rng = np.random.default_rng(5)
    gctx.nr_set_noise((0.01 * rng.standard_normal(16000)).astype(np.float32))
    ys = (0.1 * rng.standard_normal((3, 40000))).astype(np.float32)
    out = gctx.nr_reduce(ys)
    assert out.shape == ys.shape and np.isfinite(out).all()


def test_capture_and_mix_buffers_are_framed(gctx, monkeypatch):
    """The converted clips of a capture tick and the pool and plan of a host-pointer mix live in kept
    workspace slots, so the bands frame them too: one room tick (4 clips of 2 streams, 48 kHz stereo, 0.5 s
    each) and one mixed call (4 clips of 3 layers) succeed under the guard and give an unguarded context's
    bytes.  While these buffers came from an allocator of their own, without bands, this passed whatever
    the kernels stored behind them: it only pins that the bands now there stay clean."""
    from mmla_audio_amd import _lib, weights
    mono = synth.batch(990, 4, 24000)
    raw = np.empty((4, 48000), np.int16)
    raw[:, 0::2] = mono
    raw[:, 1::2] = mono // 2
    pool = synth.batch(991, 1, 60000).reshape(-1)
    plan = _lib.MixPlan.from_layers([[(1 + 7 * i, 24000 - 1000 * i, 0), (20001 + i, 12000, 1600 * i + 3),
                                      (40000, 20000, 8000 - i)] for i in range(4)])

    def calls(c):
        c.capture_reset(2, 48000, 2, 0)
        c.vad_reset(2, 3)
        tick = c.room_pipeline_capture(raw, None, None, 1, True, 2, return_pcm=True, nonstationary=True)
        return tuple(tick) + tuple(c.od_pipeline_mixed(pool, plan))

    got = calls(gctx)
    monkeypatch.delenv('MMLA_WS_GUARD')      # read at every allocation: this context's slots have no bands
    plain = _lib.Context(0)
    try:
        plain.load_weights(weights.OD, weights.pack(weights.OD, weights.synthetic(weights.OD, seed=31)), 2)
        plain.load_weights(weights.SI, weights.pack(weights.SI, weights.synthetic(weights.SI, seed=32, n_classes=8), 8),
                           8, 1)
        want = calls(plain)
    finally:
        plain.close()
    assert len(got) == len(want) == 10
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), i
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all() and np.isfinite(got[7]).all()
