"""The 3xFP16 range guard at every place OD-NET splits an activation (tests/od_range_cases.py: 22
sites), with ONE operand out of range wherever the site can be hit at a single pixel: at the first
row and column of clip 0, in the last row of clip 1's ragged last strip (the second clip of block
1's paired tails) and in clip 2's last strip (the unpaired tail; the second strip of blocks 7-9's last
workgroup is absent).  Every other site stays below half its limit (asserted on the CPU in
tests/test_od_range_cases_cpu.py), so a guard that is missing at one site, or that loses a lane, a
strip of a pair or an absent clip, is not covered for by the next site.

Hot case, host call: exactly one micro-batch is re-run in exact f32 -- the MMLA_PREC_F32 context's
bytes --, within LOGP_TOL of the float64 oracle.  Its control twin (the same construction at a
quarter of the limit) is not re-run, is within LOGP_TOL, and differs from the f32 bytes: it stayed
on 3xFP16.  The layer trace that stops behind the site's block flags too, the one that stops a
stage earlier does not: the flag is that block's own.  A device-pointer call reports MMLA_E_RANGE
once.  The reference kernels that still ship (MMLA_RB_TILE, MMLA_NO_ODU, MMLA_NO_RBS_TAILPAIR,
MMLA_NO_RBS_W1L) are held to the same on the sites they own."""
import functools

import numpy as np
import pytest

import od_range_cases as oc
from oracle import compare

pytestmark = pytest.mark.gpu

build = functools.lru_cache(maxsize=None)(oc.build)


def _context(env=None, prec=None):
    from mmla_audio_amd import _lib
    with pytest.MonkeyPatch.context() as mp:   # every switch set, so the tests hold whatever the environment
        for k in ('MMLA_RB_TILE', 'MMLA_NO_ODU', 'MMLA_NO_RBS_TAILPAIR', 'MMLA_NO_RBS_W1L'):
            mp.setenv(k, '1' if k == env else '0')
        mp.setenv('MMLA_DEBUG_TRACE_GUARD', '1')   # the layer trace as a guarded host micro-batch
        c = _lib.Context(0)
    if prec is not None:
        c.set_precision(prec)
    return c


@pytest.fixture(scope='module')
def f32():
    from mmla_audio_amd import _lib
    return _context(prec=_lib.PREC_F32)


@pytest.fixture(scope='module')
def ctx():
    return _context()


@functools.lru_cache(maxsize=None)
def _env_context(env):
    return _context(env)


def _load(c, W):
    from mmla_audio_amd import weights
    c.load_weights(weights.OD, weights.pack(weights.OD, W), 2)


def _check_host(c, f32, case):
    """the host call's contract; a case with nothing hot (control, b1.sc's odd pixel) must stay on 3xFP16"""
    _load(c, case.W)
    _load(f32, case.W)
    before = c.range_check()
    p = c.od_forward(case.x)
    reruns = c.range_check() - before
    p32 = f32.od_forward(case.x)
    err = compare.logp_err(p, case.probs)
    print(f'{case.site} {case.placement} hot={case.hot}: reruns {reruns}, |dlog p| {err:.3g}')
    assert f32.range_check() == 0
    assert err <= compare.LOGP_TOL
    if len(case.hot_idx):
        assert reruns == 1
        assert np.array_equal(p, p32)
    else:
        assert reruns == 0
        assert not np.array_equal(p, p32)
    # The flag is the site's own kernel's.  The hot operand meets a zero weight, and fp16 inf x 0 is a
    # NaN that a guard further down may report in place of a missing one here; the layer trace stops
    # behind the site's block (behind the BiLSTM for its input), so nothing further down runs, and the
    # trace that stops one stage earlier must not flag
    stage = 11 if case.site == 'lstm' else oc.block_of(case.site)
    t = c.debug_od_trace(case.x, stage)
    assert c.range_check() - before - reruns == (1 if len(case.hot_idx) else 0)
    if len(case.hot_idx):
        assert np.array_equal(t, f32.debug_od_trace(case.x, stage))
        if stage > 1:
            c.debug_od_trace(case.x, stage - 1)
            assert c.range_check() - before - reruns == 1


@pytest.mark.parametrize('hot', [True, False], ids=['hot', 'control'])
@pytest.mark.parametrize('site,placement', oc.case_ids(), ids=lambda v: v)
def test_host_call(ctx, f32, site, placement, hot):
    _check_host(ctx, f32, build(site, placement, hot))


def _one_placement(site):
    return 'channel' if (site, 'channel') in oc.case_ids() else 'lone_tail'


@pytest.mark.parametrize('site', oc.SITES)
def test_device_call_reports_range_once(ctx, site):
    import torch
    from mmla_audio_amd import _lib
    case = build(site, _one_placement(site), True)
    _load(ctx, case.W)
    before = ctx.range_check()
    x = torch.from_numpy(case.x).cuda()
    probs = torch.empty((oc.N, 2), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.od_forward_dev(x.data_ptr(), oc.N, probs.data_ptr())
    with pytest.raises(_lib.MmlaError) as e:
        ctx.range_check()
    assert e.value.code == _lib.MMLA_E_RANGE
    assert ctx.range_check() == before            # reported once, then clear; nothing was re-run


def _block_sites(blocks):
    return [s for s in oc.SITES if oc.block_of(s) in blocks]


# the A/B reference kernels and the blocks they run in place of the default ones
AB = [(env, s) for env, blocks in (('MMLA_RB_TILE', (1, 2, 3)), ('MMLA_NO_ODU', (4, 5, 6, 7, 8, 9)),
                                   ('MMLA_NO_RBS_TAILPAIR', (1,)), ('MMLA_NO_RBS_W1L', (2, 3)))
      for s in _block_sites(blocks)]


@pytest.mark.parametrize('hot', [True, False], ids=['hot', 'control'])
@pytest.mark.parametrize('env,site', AB)
def test_reference_kernels_host_call(f32, env, site, hot):
    placement = 'channel' if (site, 'channel') in oc.case_ids() else 'pair_last_row'
    _check_host(_env_context(env), f32, build(site, placement, hot))
