"""The conditions tests/od_range_cases.py promises for every case tests/test_gpu_od_range_sites.py
runs, asserted in the float64 oracle walk: the targeted split site is >= 2 x its limit and every
other one <= 0.5 x its limit; the hot operands are as many as stated, in the stated clip, region and
channel; the control twin stays <= 0.5 x the limit everywhere; the probabilities are finite; and the
walk is the oracle's OD-NET."""
import numpy as np
import pytest

import od_range_cases as oc
from oracle import nets


def test_limits_are_the_kernels():
    """65504 / the activation scale 2^4 (conv operands), 65504 / the BiLSTM's 2^6"""
    assert oc.LIMIT_CONV == 4094.0 and oc.LIMIT_LSTM == 1023.5


def test_walk_is_the_oracle_forward():
    W = oc.base_weights()
    x = oc.image('lone_tail', 4)
    probs, sites, _ = oc.walk(x, W)
    assert np.array_equal(probs, nets.od_forward(x, W))
    assert set(sites) == set(oc.SITES)
    peak = {s: float(np.abs(v).max()) / oc.limit(s) for s, v in sites.items()}
    assert max(peak.values()) < 0.06, peak         # the unedited network is far inside the range


def test_case_list_covers_every_site():
    ids = oc.case_ids()
    assert len(ids) == len(set(ids))
    assert {s for s, _ in ids} == set(oc.SITES)
    for s in oc.LOCAL_SITES + ('b1.sc',):
        assert {p for t, p in ids if t == s} >= set(oc.PLACEMENTS)


@pytest.mark.parametrize('site,placement', oc.case_ids(), ids=lambda v: v)
def test_case_conditions(site, placement):
    hot, ctl = oc.build(site, placement, True), oc.build(site, placement, False)
    lim = oc.limit(site)
    for c in (hot, ctl):
        assert set(c.amax) == set(oc.SITES)
        assert np.isfinite(c.probs).all() and c.x.dtype == np.float32 and c.x.shape == (oc.N, 128, 151, 3)
        for s, v in c.amax.items():
            if c is ctl or s != site:
                assert v <= 0.5 * oc.limit(s), (s, v)
    assert len(ctl.hot_idx) == 0
    idx = hot.hot_idx
    if placement == 'odd':          # the strided shortcut never reads an odd pixel: nothing is hot
        assert len(idx) == 0 and hot.amax[site] <= 0.5 * lim
        assert float(np.abs(nets._conv(hot.x.astype(np.float64), hot.W, 0)).max()) >= 2 * lim
        return
    assert hot.amax[site] >= 2 * lim
    assert (idx[:, -1] == hot.channel).all()
    if placement == 'channel':
        assert len(idx) > 1
        return
    assert len(idx) == 1
    n, r, q = (int(v) for v in idx[0][:3])
    assert n == oc.PLACE_CLIP[placement]
    if site == 'b1.sc':             # the one bright pixel: (0, 0), the last even row in the paired
        assert (n, 2 * r, 2 * q) == oc.SC1_PIXELS[placement]   # tail's last column, the lone tail
        assert placement == 'first' or 2 * q >= oc.GEOM[1][3]
        return
    h, _, _, last = oc.GEOM[int(site[1])]
    if placement == 'first':
        assert (r, q) == (0, 0)
    else:
        assert q >= last                                   # the kernels' last, ragged column strip
        if placement == 'pair_last_row':
            assert r == h - 1
