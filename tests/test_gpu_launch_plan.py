"""The launch plan of the two networks: which kernels run_od_net / run_si_net (csrc/net_runners.cpp)
launch in every A/B configuration, pinned through the profiler -- the exact per-stage launch counts
and the exact per-stage algorithmic work of one host-pointer pipeline call on 3 clips (the network
geometry is fixed, so the clip count is the only free size and the plan does not depend on it).

The bit-identity tests (test_gpu_rbs, test_gpu_odu, test_gpu_siu) compare two contexts' outputs; they
would not notice an A/B switch that selected the same path for both, nor a change of the work the
profiler books per stage, on which bench.py's roofline fraction is built.

The expected work is computed here in closed form from the layer table and never read back from the
library; every term is an integer below 2^53, so the comparison is ==.  Two quirks are part of the
contract: the SI stem is counted with 40 input channels when si_fe writes padded feature rows (the
default) and with 39 otherwise; the OD stem's FLOPs are booked under 'conv' when the stem is fused
into block 1 and under 'glue' when it is its own launch."""
import numpy as np
import pytest

from oracle import synth

pytestmark = pytest.mark.gpu

N = 3
CH = (32, 32, 32, 64, 64, 64, 128, 128, 128)
POOL = (True, False, False, True, False, False, True, False, False)
OD_H, OD_W = 128, 151
OD_STEM = 2 * N * OD_H * OD_W * 3 * 16
SI_T, SI_D = 256, 39
SI_NEED = 160 * 259 + 400


def lstm_flops(t):
    return 2 * N * t * 2 * (256 + 128) * 1024


def od_conv_work(blocks=9):
    """res blocks 1..blocks: Conv2D(3x3) + Conv2D((4,1)) at the block's input size, the 1x1 stride-2
    shortcut of the pool blocks at the pooled size"""
    h, w, cin, work = OD_H, OD_W, 16, 0
    for b in range(blocks):
        c = CH[b]
        work += 2 * N * h * w * (9 * cin * c + 4 * c * c)
        if POOL[b]:
            h, w = (h + 1) // 2, (w + 1) // 2
            work += 2 * N * h * w * cin * c
        cin = c
    return work, h, w


def od_expected(conv_n, glue_n, stem_fused, blocks=9, mean=True, pipeline=True):
    """a run through `blocks` res blocks, then the mean over h, then (pipeline) the front-end before
    and the BiLSTM and the head after"""
    conv, h, w = od_conv_work(blocks)
    glue = 0
    if stem_fused:
        conv += OD_STEM
    else:
        glue += OD_STEM
    if mean:
        glue += N * h * w * 128
    exp = {s: (0, 0) for s in ('od_fe', 'si_fe', 'conv', 'lstm', 'glue', 'head', 'nr')}
    exp['conv'] = (conv_n, conv)
    exp['glue'] = (glue_n, glue)
    if pipeline:
        exp['od_fe'] = (1, N * (24000 * 2 + OD_H * OD_W * 3))   # int16 samples read, uint8 image written
        exp['lstm'] = (1, lstm_flops(w))
        exp['head'] = (1, 2 * N * 512 * 2)
    return exp


def si_expected(k, conv_n, glue_n, stem_cin, final_glue, f32_pools=False):
    t, cin = SI_T, 32
    conv = 2 * N * t * 4 * stem_cin * 32
    glue = 0
    for u in range(9):
        c = CH[u]
        if POOL[u]:
            if f32_pools:
                glue += N * t * cin   # MaxPool1D as its own launch
            t = (t + 1) // 2
            conv += 2 * N * t * cin * c   # shortcut Conv1D(1, stride 2)
        conv += 2 * N * t * (3 * cin * c + 3 * c * c)
        cin = c
    if final_glue:
        glue += 3 * N * t * 128
    exp = {s: (0, 0) for s in ('od_fe', 'si_fe', 'conv', 'lstm', 'glue', 'head', 'nr')}
    exp['si_fe'] = (1, N * (SI_NEED * 2 + SI_T * SI_D * 4 + 1))   # ragged clips: the full reach is booked
    exp['conv'] = (conv_n, conv)
    exp['glue'] = (glue_n, glue)
    exp['lstm'] = (1, lstm_flops(t // 4))
    exp['head'] = (2, 2 * N * 512 * k + 4 * N * k)
    return exp


def _check(c, exp):
    got = c.profile_read()
    plan = {s: (got[s][1], got[s][2]) for s in got}
    print(plan)
    assert plan == {s: (n, float(w)) for s, (n, w) in exp.items()}


def _ctx(monkeypatch, env):
    from mmla_audio_amd import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = _lib.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return c


@pytest.fixture(scope='module')
def od_weights():
    from mmla_audio_amd import weights
    return weights.pack(weights.OD, weights.synthetic(weights.OD, seed=53))


def _od_ctx(monkeypatch, env, packed):
    from mmla_audio_amd import weights
    c = _ctx(monkeypatch, env)
    c.load_weights(weights.OD, packed, 2)
    return c


@pytest.mark.parametrize('env,f32,conv_n,glue_n', [
    ({'MMLA_RB_TILE': '0', 'MMLA_NO_ODU': '0'}, False, 9, 1),
    ({'MMLA_RB_TILE': '1', 'MMLA_NO_ODU': '0'}, False, 9, 1),
    ({'MMLA_RB_TILE': '0', 'MMLA_NO_ODU': '1'}, False, 15, 1),
    ({'MMLA_RB_TILE': '0', 'MMLA_NO_ODU': '0'}, True, 21, 2),
], ids=['default', 'rb_tile', 'no_odu', 'f32'])
def test_od_pipeline_plan(monkeypatch, od_weights, env, f32, conv_n, glue_n):
    from mmla_audio_amd import _lib
    c = _od_ctx(monkeypatch, env, od_weights)
    if f32:
        c.set_precision(_lib.PREC_F32)
    c.profile_enable()
    c.od_pipeline(synth.batch(3300, N, 40000))
    _check(c, od_expected(conv_n, glue_n, stem_fused=not f32))


@pytest.mark.parametrize('stage,conv_n,glue_n', [(0, 0, 1), (1, 1, 0), (5, 5, 0), (10, 9, 1)])
def test_od_trace_plan(monkeypatch, od_weights, stage, conv_n, glue_n):
    """debug_od_trace stops after `stage`; stage 0 forces the stand-alone stem launch"""
    c = _od_ctx(monkeypatch, {'MMLA_RB_TILE': '0', 'MMLA_NO_ODU': '0'}, od_weights)
    x = np.random.default_rng(51).integers(0, 256, size=(N, 128, 151, 3)).astype(np.float32)
    c.profile_enable()
    c.debug_od_trace(x, stage)
    _check(c, od_expected(conv_n, glue_n, stem_fused=stage != 0, blocks=min(stage, 9),
                          mean=stage == 10, pipeline=False))


SI_ON = {'MMLA_NO_SIU': '0', 'MMLA_NO_SIPU': '0', 'MMLA_NO_SIFIN': '0', 'MMLA_NO_SIPAD': '0',
         'MMLA_NO_SIPAIR': '0', 'MMLA_NO_SICHAIN': '0'}
SI_OFF = {k: '1' for k in SI_ON}


@pytest.mark.parametrize('k', [630, 8])
@pytest.mark.parametrize('env,f32,conv_n,glue_n', [
    (SI_ON, False, 4, 0),
    (dict(SI_ON, MMLA_NO_SICHAIN='1'), False, 7, 0),
    (dict(SI_ON, MMLA_NO_SICHAIN='1', MMLA_NO_SIPAIR='1'), False, 10, 0),
    (dict(SI_ON, MMLA_NO_SICHAIN='1', MMLA_NO_SIPAIR='1', MMLA_NO_SIFIN='1'), False, 10, 1),
    (SI_OFF, False, 19, 1),
    (SI_ON, True, 22, 4),
], ids=['all_on', 'no_chain', 'no_pair', 'no_fin', 'all_off', 'f32'])
def test_si_pipeline_plan(monkeypatch, env, f32, conv_n, glue_n, k):
    from mmla_audio_amd import _lib, weights
    c = _ctx(monkeypatch, env)
    W = weights.synthetic(weights.SI, seed=31, n_classes=k)
    c.load_weights(weights.SI, weights.pack(weights.SI, W, k), k, _lib.HEAD_SOFTMAX)
    if f32:
        c.set_precision(_lib.PREC_F32)
    c.profile_enable()
    c.si_pipeline([synth.clip(4000 + i, n) for i, n in enumerate((24000, 3000, 17000))])
    padded = not f32 and env['MMLA_NO_SIPAD'] == '0'
    _check(c, si_expected(k, conv_n, glue_n, SI_D + 1 if padded else SI_D,
                          final_glue=f32 or env['MMLA_NO_SIFIN'] == '1', f32_pools=f32))
