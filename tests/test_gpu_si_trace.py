"""SI-NET stage by stage (mmla_debug_si_trace) against the float64 oracle walk (tests/si_trace_ref.py),
on every path the context's switches select: the default three 3-unit chains, a pool unit + pairs, one
unit per launch with and without the fused final pooling, the conv_h3 launches, and exact f32.

Bound, per stage: max|got - ref64| <= 16 x max(d32, 2^-24 max|ref64|), d32 = the oracle's own float32
walk against its float64 walk on the same inputs (si_finetune_cases.d32_bound) -- asserted over the
whole tensor and again over the edge rows alone, where the chain geometry can go wrong and a
whole-tensor maximum could be dominated elsewhere: the first and last row of every clip, the last
output row of each workgroup and the first of the next, the last row of the batch.  The workgroup rows
come from the launches' geometry (si_range_cases.chain_rows).

5 clips (three si_golden, two of 10 x standard normal): every default chain launch has more than one
workgroup and the last one has rows past the batch; 1 clip: every row clamped at both ends, fewer
rows than one tile.  Synthetic weights, K = 8 with the sigmoid head; K = 630 softmax for the logits.

Measured (MI355X), worst over paths and n; ratio = err / bound, rel = err / max|ref64| (OD's layer
trace is held to rel <= 1e-5): stages 0-10 ratio 0.07-0.22 (edge rows 0.07-0.17), rel 2.6e-7 - 8.2e-7;
stage 11 ratio 0.13, rel 3.1e-6; stage 12 ratio 0.33 (K = 8, n = 1, exact f32), 0.065 at K = 630.  The
per-stage table is in DESIGN.md, "SI-NET from the inside"."""
import functools

import numpy as np
import pytest

import si_finetune_cases as fc
import si_range_cases as sc
import si_trace_ref as ref
from oracle import compare

pytestmark = pytest.mark.gpu

ALL, PATHS, context = sc.ALL_STAGES, sc.PATHS, sc.context


@functools.lru_cache(maxsize=None)
def walks(n, k=sc.K):
    """the oracle's float64 and float32 walks of the first n clips: computed once, read-only"""
    from mmla_audio_amd import weights
    W = weights.synthetic(weights.SI, seed=sc.SEED, n_classes=k)
    head = 'sigmoid' if k == sc.K else 'softmax'
    x = sc.base_features()[:n]
    out = tuple(ref.walk(x, W, head=head, dtype=d) for d in (np.float64, np.float32))
    for o in out:
        for v in o.values():
            v.setflags(write=False)
    return out


def edge_rows(stage, n, launches):
    """-> the edge rows of a stage tensor as (clip, row) index arrays; None: every row is one (the
    per-clip stages 11 and 12)"""
    if stage >= 11:
        return None
    unit = min(max(stage, 1), 9)                 # whose rows: the stem has unit 1's unpooled rows
    T = 256 if stage == 0 else 8 if stage == 10 else ref.ROWS[unit]
    rows = n * T
    g = {c * T + r for c in range(n) for r in (0, T - 1)} | {rows - 1}
    if stage >= 1:
        per = 4 if stage == 10 else 1            # a row of stage 10 is four rows of unit 9
        for launch in {sc.DEFAULT_LAUNCH[unit], launches.get(unit, sc.DEFAULT_LAUNCH[unit])}:
            ro = sc.chain_rows(*launch)
            for e in range(ro, n * ref.ROWS[unit], ro):
                g |= {(e - 1) // per, e // per}
    g = np.array(sorted(g))
    return g // T, g % T


def check_stage(label, got, r64, r32, edges):
    """the d32 rule over the whole tensor and over the edge rows alone; prints the figures first"""
    assert got.shape == r64.shape and got.dtype == np.float32
    worst = 0.0
    for what, sel in (('all', None), ('edges', edges)):
        g, a, b = (got, r64, r32) if sel is None else (got[sel], r64[sel], r32[sel])
        err = float(np.max(np.abs(g.astype(np.float64) - a)))
        bound = fc.d32_bound(a, b)
        print(f'{label} {what:5s}: |got - ref64| {err:.3e}  bound {bound:.3e}  ratio {err / bound:.3f}  '
              f'rel {err / float(np.max(np.abs(a))):.2e} (OD: 1e-5)')
        assert np.isfinite(g).all() and err <= bound, f'{label} {what}: {err:.3e} > {bound:.3e}'
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize('n', [sc.N, 1])
@pytest.mark.parametrize('path', PATHS)
def test_stages_vs_oracle(path, n):
    ones, f32, stages, launches = PATHS[path]
    c = context(ones, f32)
    r64, r32 = walks(n)
    x = sc.base_features()[:n]
    for s in stages:
        check_stage(f'{path} n={n} stage {s:2d}', c.debug_si_trace(x, s), r64[s], r32[s], edge_rows(s, n, launches))
    assert c.range_check() == 0
    missing = [s for s in ALL if s not in stages]
    from mmla_audio_amd import _lib
    for s in missing:                            # a stage a fused launch keeps on chip: refused, and named
        with pytest.raises(_lib.MmlaError) as e:
            c.debug_si_trace(x, s)
        assert e.value.code == _lib.MMLA_E_INVALID and 'stays on chip' in str(e.value), str(e.value)


def test_default_path_names_the_launch():
    from mmla_audio_amd import _lib
    c = context()
    x = sc.base_features()
    with pytest.raises(_lib.MmlaError) as e:
        c.debug_si_trace(x, 2)
    assert e.value.code == _lib.MMLA_E_INVALID and 'units 1-3' in str(e.value)
    with pytest.raises(_lib.MmlaError) as e:
        c.debug_si_trace(x, 9)
    assert e.value.code == _lib.MMLA_E_INVALID and 'MMLA_NO_SIFIN' in str(e.value)
    for s in (-1, 13):
        with pytest.raises(_lib.MmlaError) as e:
            c.debug_si_trace(x, s)
        assert e.value.code == _lib.MMLA_E_INVALID


def test_logits_630_softmax():
    """stage 12 with padded logit rows in memory (K = 630), and the stages in front of it once more"""
    c = context(k=630)
    r64, r32 = walks(sc.N, 630)
    x = sc.base_features()
    for s in (10, 11, 12):
        check_stage(f'K=630 stage {s}', c.debug_si_trace(x, s), r64[s], r32[s], edge_rows(s, sc.N, {}))
    assert c.debug_si_trace(x, 12).shape == (sc.N, 630)


@pytest.mark.parametrize('stage,conv_n', [(0, 1), (3, 2), (6, 3), (10, 4), (11, 4), (12, 4)])
def test_trace_runs_the_selected_launches(stage, conv_n):
    """the stop stage does not change the plan: the default path up to `stage` is the stem and one
    chain launch per three units, the final pooling inside the last, and nothing behind the stage runs"""
    c = context()
    c.profile_enable(True)
    c.debug_si_trace(sc.base_features(), stage)
    prof = c.profile_read()
    assert prof['conv'][1] == conv_n and prof['glue'][1] == 0
    assert prof['lstm'][1] == (1 if stage >= 11 else 0)
    assert prof['head'][1] == (1 if stage == 12 else 0)           # the Dense; the sigmoid is behind the logits


def test_trace_is_the_forward_pass():
    """what the trace taps is what mmla_si_forward / mmla_si_embed compute"""
    c = context()
    x = sc.base_features()
    assert np.array_equal(c.debug_si_trace(x, 11), c.si_embed(x))
    z = c.debug_si_trace(x, 12).astype(np.float64)
    assert compare.logp_err(c.si_forward(x), 1.0 / (1.0 + np.exp(-z))) <= compare.LOGP_TOL
