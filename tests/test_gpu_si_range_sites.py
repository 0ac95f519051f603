"""The 3xFP16 range guard at every place SI-NET splits an activation (tests/si_range_cases.py: 23
sites), with ONE operand out of range wherever the site can be hit at a single row: at the first row
of clip 0, at the last row of clip 1 (the next tap is another clip's row), at the last output row of
the default launch's first workgroup and at the row after it, and at the last row of the batch, in
the tail workgroup whose other rows lie past the batch.  Every other site stays below half its limit
(asserted on the CPU in tests/test_si_range_cases_cpu.py), so a guard that is missing at one site, or
that loses a lane, a halo row or the tail workgroup, is not covered for by the next site.

Hot case, host call: exactly one micro-batch is re-run in exact f32 -- the MMLA_PREC_F32 context's
bytes --, within LOGP_TOL of the float64 oracle.  Its control twin (the same construction at a
quarter of the limit) is not re-run, is within LOGP_TOL, and differs from the f32 bytes: it stayed
on 3xFP16.  The layer trace that stops at the end of the site's launch flags too and equals the f32
trace; the one that stops at the end of the launch before does not: the flag is that launch's own.
A device-pointer call reports MMLA_E_RANGE once.  The other launch plans (a pool unit + pairs, one
unit per launch with and without the fused final pooling, pool units on conv_h3, conv_h3 throughout)
are held to the same at the first and the last row of the batch on the sites they own, and the
unsplit BiLSTM (MMLA_NO_LSTM_SPLIT) on its input.  The opposite case, an operand out of range only in
the rows a tail workgroup computes past the batch, must not flag (past_batch)."""
import functools

import numpy as np
import pytest

import si_range_cases as sc
from oracle import compare

ALL, PATHS, SWITCHES, context = sc.ALL_STAGES, sc.PATHS, sc.SWITCHES, sc.context

pytestmark = pytest.mark.gpu

POOL_STAGES = (0, 1, 3, 4, 6, 7, 10, 11, 12)
# path -> (switches set to 1, the stages it writes to memory, the sites whose launch it changes)
UNIT_SITES = tuple(s for s in sc.SITES if 1 <= sc.unit_of(s) <= 9)
AB = {
    'no_chain': (PATHS['no_chain'][0], PATHS['no_chain'][2], UNIT_SITES),
    'no_pair': (PATHS['no_pair'][0], PATHS['no_pair'][2], UNIT_SITES),
    'no_fin': (PATHS['no_fin'][0], ALL, ('u9.in', 'u9.mid')),
    'no_sipu': (('MMLA_NO_SIPU',), POOL_STAGES, tuple(s for s in UNIT_SITES if sc.unit_of(s) in sc.POOL_UNITS)),
    'conv_h3': (SWITCHES, ALL, UNIT_SITES),
}


@functools.lru_cache(maxsize=None)
def _context(ones=(), f32=False, extra=()):
    return context(ones, f32, k=None, guard=True, extra=extra)   # the layer trace as a guarded host micro-batch


@pytest.fixture(scope='module')
def f32():
    return _context(f32=True)


def _load(c, W):
    from mmla_audio_amd import _lib, weights
    c.load_weights(weights.SI, weights.pack(weights.SI, W, sc.K), sc.K, _lib.HEAD_SIGMOID)


def launch_stages(site, stages):
    """-> (the stage at which the site's launch ends, the stage at which the launch before it ends or
    None) among the stages a path writes to memory"""
    k = {0: 0, 10: 11}.get(sc.unit_of(site), sc.unit_of(site))
    end = min(s for s in stages if s >= k)
    return end, max((s for s in stages if s < end), default=None)


def _check_host(c, f32, case, stages):
    """the host call's contract; a case with nothing hot (control, u1.sc's odd row) must stay on 3xFP16"""
    _load(c, case.W)
    _load(f32, case.W)
    before = c.range_check()
    p = c.si_forward(case.x)
    reruns = c.range_check() - before
    p32 = f32.si_forward(case.x)
    err = compare.logp_err(p, case.probs)
    print(f'{case.site} {case.placement} hot={case.hot}: reruns {reruns}, |dlog p| {err:.3g}')
    assert f32.range_check() == 0
    assert err <= compare.LOGP_TOL
    hot = len(case.hot_idx) > 0
    if hot:
        assert reruns == 1
        assert np.array_equal(p, p32)
    else:
        assert reruns == 0
        assert not np.array_equal(p, p32)
    # The flag is the site's own launch's.  The hot operand meets a zero weight, and fp16 inf x 0 is a
    # NaN that a guard further down may report in place of a missing one here; the layer trace stops
    # at the end of the site's launch, so nothing further down runs, and the trace that stops at the
    # end of the launch before must not flag
    end, prev = launch_stages(case.site, stages)
    t = c.debug_si_trace(case.x, end)
    assert c.range_check() - before - reruns == (1 if hot else 0)
    if hot:
        assert np.array_equal(t, f32.debug_si_trace(case.x, end))
        if prev is not None:
            c.debug_si_trace(case.x, prev)
            assert c.range_check() - before - reruns == 1
    assert f32.range_check() == 0


@pytest.mark.parametrize('hot', [True, False], ids=['hot', 'control'])
@pytest.mark.parametrize('site,placement', sc.case_ids(), ids=lambda v: v)
def test_host_call(f32, site, placement, hot):
    _check_host(_context(), f32, sc.build(site, placement, hot), PATHS['default'][2])


def _one_placement(site):
    return next(p for p in ('channel', 'even', 'first') if (site, p) in sc.case_ids())


@pytest.mark.parametrize('site', sc.SITES)
def test_device_call_reports_range_once(site):
    import torch
    from mmla_audio_amd import _lib
    ctx = _context()
    case = sc.build(site, _one_placement(site), True)
    _load(ctx, case.W)
    before = ctx.range_check()
    x = torch.from_numpy(np.array(case.x)).cuda()
    probs = torch.empty((sc.N, sc.K), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.si_forward_dev(x.data_ptr(), sc.N, probs.data_ptr())
    with pytest.raises(_lib.MmlaError) as e:
        ctx.range_check()
    assert e.value.code == _lib.MMLA_E_RANGE
    assert ctx.range_check() == before            # reported once, then clear; nothing was re-run


def _ab_cases():
    out = []
    for path, (_, _, sites) in AB.items():
        for s in sites:
            ps = ('first', 'batch_end') if s in sc.LOCAL_SITES else (_one_placement(s),)
            out += [(path, s, p) for p in ps]
    return out


@pytest.mark.parametrize('hot', [True, False], ids=['hot', 'control'])
@pytest.mark.parametrize('path,site,placement', _ab_cases(), ids=lambda v: v)
def test_other_launch_plans_host_call(f32, path, site, placement, hot):
    ones, stages, _ = AB[path]
    _check_host(_context(tuple(ones)), f32, sc.build(site, placement, hot), stages)


@pytest.mark.parametrize('hot', [True, False], ids=['hot', 'control'])
def test_unsplit_bilstm_host_call(f32, hot):
    c = _context(extra=(('MMLA_NO_LSTM_SPLIT', '1'),))
    _check_host(c, f32, sc.build('lstm', 'channel', hot), PATHS['default'][2])


# where each unit is the first of its launch: the rows past the batch then hold copies of the last row
PAST = [(path, f'u{u}.mid') for path, units in (('default', (1, 4, 7)), ('no_chain', (1, 2, 4, 5, 7, 8)),
                                                ('no_pair', range(1, 10)), ('no_fin', (9,)))
        for u in units]


@pytest.mark.parametrize('path,site', PAST, ids=lambda v: v)
def test_rows_past_the_batch_do_not_flag(f32, path, site):
    """the tail workgroup's rows past the batch hold an operand of 2.3 and 4.3 x the limit while nothing in
    the batch is above 0.3 x (tests/si_range_cases.py _build_past_batch): no re-run, 3xFP16 bytes"""
    ones, stages = (PATHS[path][0], PATHS[path][2])
    _check_host(_context(tuple(ones)), f32, sc.build(site, 'past_batch', False), stages)
