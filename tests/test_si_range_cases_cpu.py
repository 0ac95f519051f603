"""The conditions tests/si_range_cases.py promises for every case tests/test_gpu_si_range_sites.py
runs, asserted in the float64 oracle walk: the targeted split site is >= 2 x its limit and every
other one <= 0.5 x its limit; the hot operands are as many as stated, in the stated clip, row and
channel; the control twin stays <= 0.5 x the limit everywhere; the probabilities are finite and the
hot channel's downstream weights are zero; and the walk is the oracle's SI-NET.

Measured: the whole file (101 hot / control pairs, 9 past-batch cases) takes 18 s; the float64 walk of
five clips takes 30 ms, it restarts from the edited unit on the unedited prefix, and a built case is
cached."""
import numpy as np
import pytest

import si_range_cases as sc
import si_trace_ref as ref
from oracle import nets


def test_limits_are_the_kernels():
    """65504 / the activation scale 2^4 (conv operands), 65504 / the BiLSTM's 2^6"""
    assert sc.LIMIT_CONV == 4094.0 and sc.LIMIT_LSTM == 1023.5


@pytest.mark.parametrize('head', ['sigmoid', 'softmax'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_walk_is_the_oracle_forward(head, dtype):
    W, x = sc.base_weights(), sc.base_features()
    out = ref.walk(x, W, head=head, dtype=dtype)
    assert out['probs'].dtype == dtype
    assert np.array_equal(out['probs'], nets.si_forward(x, W, head=head, dtype=dtype))
    assert np.array_equal(out[12], nets.si_forward(x, W, head=head, dtype=dtype, return_logits=True))
    shapes = {0: (256, 32), 10: (8, 128), 11: (512,), 12: (sc.K,)}
    for s in ref.STAGES:
        want = shapes.get(s) or (ref.ROWS[s], nets.CHANNELS[s - 1])
        assert out[s].shape == (sc.N,) + want, s


def test_walk_restarts_on_a_prefix():
    W, x = sc.base_weights(), sc.base_features()
    probs, sites, stages = sc.walk(x, W)
    assert set(sites) == set(sc.SITES)
    peak = {s: v[0] / sc.limit(s) for s, v in sites.items()}
    assert max(peak.values()) < 0.06, peak         # the unedited network is far inside the range
    for first in (2, 4, 9):
        p2, s2, st2 = sc.walk(x, W, first, stages[first - 1])
        assert np.array_equal(p2, probs)
        assert set(s2) == {s for s in sc.SITES if sc.unit_of(s) >= first}
        assert all(np.array_equal(st2[k], stages[k]) for k in st2 if k != 'probs')


def test_workgroup_rows():
    """the rows a default launch's workgroup writes, and what follows for 5 clips: more than one
    workgroup per launch, and a last workgroup with rows past the batch"""
    assert [sc.wg_rows(u) for u in (1, 4, 7)] == [244, 244, 112]
    for u in range(1, 10):
        rows, per = sc.N * sc.ROWS[u], sc.wg_rows(u)
        assert rows > per and rows % per != 0
        for p in ('wg_last', 'wg_first'):
            clip, row = sc.target(f'u{u}.in', p)
            g = clip * sc.ROWS[u] + row
            assert g == per - (p == 'wg_last') and 0 < row < sc.ROWS[u] - 1     # inside a clip


def test_case_list_covers_every_site():
    ids = sc.case_ids()
    assert len(ids) == len(set(ids))
    assert {s for s, _ in ids} == set(sc.SITES)
    for s in sc.LOCAL_SITES:
        assert {p for t, p in ids if t == s} == set(sc.PLACEMENTS)
    assert {p for t, p in ids if t == 'stem'} == set(sc.STEM_PLACEMENTS)


def _downstream_zero(case):
    """every weight that multiplies the hot channel"""
    W, c, u = case.W, case.channel, sc.unit_of(case.site)
    kind = case.site.split('.')[-1]
    if case.site == 'stem':
        ws = [W['layer_with_weights-0/kernel'][:, c, :]]
    elif case.site == 'lstm':
        ws = [W[f'layer_with_weights-41/{d}/kernel'][c, :] for d in ('forward', 'backward')]
    elif kind == 'sc':      # the shortcut conv, and the unit's BN_in (its conv_a then sees ReLU(0))
        ws = [W[f'layer_with_weights-{sc.K_IN[u] + 3}/kernel'][:, c, :], W[f'layer_with_weights-{sc.K_IN[u]}/gamma'][c],
              W[f'layer_with_weights-{sc.K_IN[u]}/beta'][c]]
    elif kind == 'in':
        ws = [W[f'layer_with_weights-{sc.K_IN[u] + 1}/kernel'][:, c, :]]
    else:
        ws = [W[f'layer_with_weights-{sc.K_IN[u] + (4 if u in sc.POOL_UNITS else 3)}/kernel'][:, c, :]]
    return all(not np.any(w) for w in ws)


@pytest.mark.parametrize('site,placement', sc.case_ids(), ids=lambda v: v)
def test_case_conditions(site, placement):
    hot, ctl = sc.build(site, placement, True), sc.build(site, placement, False)
    lim = sc.limit(site)
    for c in (hot, ctl):
        assert set(c.amax) == set(sc.SITES)
        assert np.isfinite(c.probs).all() and c.probs.shape == (sc.N, sc.K)
        assert c.x.dtype == np.float32 and c.x.shape == (sc.N, 256, 39)
        assert _downstream_zero(c)
        for s, v in c.amax.items():
            if c is ctl or s != site:
                assert v <= 0.5 * sc.limit(s), (s, v)
        # the recorded figures are the float64 walk's of these very weights and features
        probs, sites, _ = sc.walk(c.x, c.W)
        assert np.array_equal(probs, c.probs) and {s: v[0] for s, v in sites.items()} == c.amax
    assert len(ctl.hot_idx) == 0 and ctl.amax[site] >= 0.2 * lim or placement == 'odd'
    idx = hot.hot_idx
    if placement == 'odd':          # the strided shortcut never reads an odd row: nothing is hot,
        assert len(idx) == 0 and hot.amax[site] <= 0.5 * lim      # although the stem output there is
        assert float(np.abs(ref.walk(hot.x, hot.W)[0]).max()) >= 2 * lim
        return
    assert hot.amax[site] >= 2 * lim
    assert (idx[:, -1] == hot.channel).all()
    if placement == 'channel':
        assert len(idx) > 1
        return
    assert len(idx) == 1
    n, r = int(idx[0][0]), int(idx[0][1])
    if site == 'u1.sc':
        assert (n, 2 * r) == sc.SC1_ROWS['even'] and sc.SC1_ROWS['odd'][1] % 2 == 1
        return
    assert (n, r) == sc.target(site, placement) and r == hot.row


@pytest.mark.parametrize('site', sc.PAST_SITES)
def test_past_batch_conditions(site):
    """nothing in the batch is above half a limit; the site's channel c holds 0.3 x the limit in the
    last two rows of the batch and exactly 0 elsewhere, and is conv_a's plain three-tap sum of ONE
    nonzero operand -- so a row that saw that operand in two or three taps holds 2.3 or 4.3 x the limit"""
    case = sc.build(site, 'past_batch', False)
    u, c = sc.unit_of(site), case.channel
    assert np.isfinite(case.probs).all() and _downstream_zero(case) and len(case.hot_idx) == 0
    assert set(case.amax) == set(sc.SITES) and all(v <= 0.5 * sc.limit(s) for s, v in case.amax.items())
    sites = {}
    ref.walk(case.x, case.W, sites=sites)
    a, m = sites[f'u{u}.in'], sites[site][:, :, c]
    d = sc.build(f'u{u}.in', 'batch_end', False).channel
    assert np.argwhere(a[:, :, d]).tolist() == [[sc.N - 1, ref.ROWS[u] - 1]]
    A = a[sc.N - 1, -1, d]
    assert abs(A / sc.LIMIT_CONV - sc.CONTROL_SCALE) < 1e-6
    assert np.argwhere(m).tolist() == [[sc.N - 1, ref.ROWS[u] - 2], [sc.N - 1, ref.ROWS[u] - 1]]
    assert np.allclose(m[sc.N - 1, -2:] / sc.LIMIT_CONV, sc.PAST_MID, atol=1e-5)
    k = sc.K_IN[u]
    kern = case.W[f'layer_with_weights-{k + 1}/kernel'][:, :, c]
    assert np.array_equal(kern[:, d], np.ones(3)) and np.count_nonzero(kern) == 3
    copies = lambda t: nets.relu(nets.batchnorm(np.array([[[t * A]]]), {n: v[c:c + 1] for n, v in case.W.items()
                                                                      if n.startswith(f'layer_with_weights-{k + 2}/')}, k + 2))
    assert copies(1) <= 0.5 * sc.LIMIT_CONV and copies(2) >= 2 * sc.LIMIT_CONV and copies(3) >= 4 * sc.LIMIT_CONV
