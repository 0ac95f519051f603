"""SI-NET inputs that drive exactly one 3xFP16 split site out of range -- TEST INFRASTRUCTURE ONLY.

SI-NET splits an activation into fp16 hi + lo at 23 places (SITES): the raw features the stem conv
reads (``stem``), the two conv operands of each res unit (``u<k>.in`` = ReLU(BN_in(x)), of the
max-pooled x in units 1, 4, 7; ``u<k>.mid`` = ReLU(BN_mid(conv_a))), the raw unit input the strided
shortcut of units 1, 4, 7 reads at even rows (``u<k>.sc``) and the BiLSTM input (``lstm``, the
[n, 8, 128] sequence).  Conv operands are split at 2^4, so the limit is 65504 / 16 = 4094 (f16x3.h
ACT_SCALE, SPLIT_MAX); the BiLSTM input at 2^6, limit 1023.5 (nets.hip LSTM_AS).  The BiLSTM state and
the Dense input are bounded by 1 and are no sites.

``build(site, placement, hot)`` returns weights (synthetic seed 5, K = 8, sigmoid head, edited) and a
5-clip feature batch (three si_golden clips, two of 10 x standard normal) for which, in the float64
oracle walk (tests/si_trace_ref.py),
  * hot: the targeted site is >= 2 x its limit, every other site <= 0.5 x its limit;
  * control (hot=False): the same construction at 0.25 x the limit, every site <= 0.5 x its limit;
  * the probabilities are finite, because the hot channel's downstream weights are zero.
``stem``, ``.in`` and ``.mid`` cases have exactly ONE hot operand in the whole batch, at a row of the
site's own pooled rows (PLACEMENTS): a feature bump over the source rows that map to the target row,
a channel whose extremum lands there, and that channel's BatchNorm set so that ReLU zeroes the
runner-up.  Every case reaches its exact row, the deepest units included (Case.row records it and
tests/test_si_range_cases_cpu.py asserts it).  tests/test_gpu_si_range_sites.py runs the cases.

5 clips: the smallest batch at which every default launch (units 1-3, 4-6, 7-9) has more than one
workgroup; the clips' rows do not divide the workgroups' rows either, so the last workgroup has rows
past the batch.  The workgroup rows come from chain_rows(), the chain kernel's row bookkeeping
restated: a launch of U units computes `tile` rows and each conv narrows the correct ones by one at
each end, so it writes tile - 4 U rows; the launch that ends the net (fused BN + ReLU + AvgPool4)
keeps its first row and its row count multiples of the pool window 4.
"""
import functools
import os
from collections import namedtuple

import numpy as np

import si_trace_ref as ref

N = 5
K = 8
SEED = 5
LIMIT_CONV = 65504.0 / 16.0
LIMIT_LSTM = 65504.0 / 64.0
HOT_SCALE, CONTROL_SCALE = 4.0, 0.25
BUMP = 150.0            # |feature| of the steering bump (the clips' own features reach about 40)
BUMP_TRIES = 12         # sign patterns tried for a channel that peaks on the exact row

K_IN, POOL_UNITS, ROWS = ref.K_IN, ref.POOL_UNITS, ref.ROWS
LOCAL_SITES = tuple(f'u{u}.{k}' for u in range(1, 10) for k in ('in', 'mid'))
SITES = ('stem',) + tuple(s for u in range(1, 10)
                          for s in ([f'u{u}.sc'] if u in POOL_UNITS else []) + [f'u{u}.in', f'u{u}.mid']) + ('lstm',)
assert len(SITES) == 23
PLACEMENTS = ('first', 'clip_end', 'wg_last', 'wg_first', 'batch_end')
STEM_PLACEMENTS = ('first', 'clip_end', 'batch_end')
SC1_ROWS = {'even': (2, 100), 'odd': (2, 101)}      # u1.sc: (clip, source row) of the feature spike

# the default launches: units -> (rows of the kernel's tile, units in the launch, ends the net)
DEFAULT_LAUNCH = {1: (256, 3, False), 2: (256, 3, False), 3: (256, 3, False),
                  4: (256, 3, False), 5: (256, 3, False), 6: (256, 3, False),
                  7: (128, 3, True), 8: (128, 3, True), 9: (128, 3, True)}

Case = namedtuple('Case', 'site placement hot W x probs amax hot_idx channel row')


def chain_rows(tile, units, fin):
    """output rows per workgroup of a chain launch (see the module docstring)"""
    if not fin:
        return tile - 4 * units
    front = (2 * units + 3) // 4 * 4
    return (tile - front - 2 * units) // 4 * 4


def wg_rows(u):
    return chain_rows(*DEFAULT_LAUNCH[u])


def limit(site):
    return LIMIT_LSTM if site == 'lstm' else LIMIT_CONV


def unit_of(site):
    """0 the stem, 1..9 the res units, 10 the BiLSTM's input"""
    return 0 if site == 'stem' else 10 if site == 'lstm' else int(site[1])


def target(site, placement):
    """-> (clip, row) in the site's own rows per clip"""
    T = 256 if site == 'stem' else ROWS[unit_of(site)]
    if placement == 'first':
        return 0, 0
    if placement == 'clip_end':
        return 1, T - 1
    if placement == 'batch_end':
        return N - 1, T - 1
    g = wg_rows(unit_of(site)) - (1 if placement == 'wg_last' else 0)   # global row, first workgroup's end
    return g // T, g % T


def case_ids():
    """every (site, placement) the default path runs, consecutive cases sharing a feature batch"""
    ids = [('stem', p) for p in STEM_PLACEMENTS]
    for p in PLACEMENTS:
        ids += [(s, p) for s in LOCAL_SITES]
    ids += [('u1.sc', p) for p in SC1_ROWS]
    ids += [('u4.sc', 'channel'), ('u7.sc', 'channel'), ('lstm', 'channel')]
    return ids


def base_weights():
    from mmla_audio_amd import weights
    return weights.synthetic(weights.SI, seed=SEED, n_classes=K)


@functools.lru_cache(maxsize=None)
def base_features():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'si_golden.npz'))
    rng = np.random.default_rng(SEED)
    x = np.concatenate([g['feat_0'], g['feat_1'], g['feat_2'], 10.0 * rng.standard_normal((2, 256, 39))])
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


# ---- the oracle walk ------------------------------------------------------------------------------

def _summary(sites):
    """{site: tensor} -> {site: (max |operand|, indices of the operands above 0.5 x the limit)}"""
    out = {}
    for s, v in sites.items():
        a = np.abs(v)
        out[s] = (float(a.max()), np.argwhere(a > 0.5 * limit(s)))
    return out


def walk(x, W, first=1, net=None):
    """float64 SI-NET from unit `first` on (net: its input; default the stem of x)
    -> (probs, {site: summary} of what was walked, {stage: tensor})"""
    sites = {}
    out = ref.walk(x, W, head='sigmoid', first=first, net=net, sites=sites)
    return out['probs'], _summary(sites), out


def _finish(site, placement, hot, W, x, first, net, before, channel):
    """walk the edited network from unit `first`; the sites before it are the unedited ones"""
    amax = {s: v[0] for s, v in before.items() if unit_of(s) < first}
    probs, out, _ = walk(x, W, first, net)
    amax.update({s: v[0] for s, v in out.items()})
    idx = out[site][1]
    row = int(idx[0][1]) if len(idx) == 1 else None
    return Case(site, placement, hot, W, x, probs, amax, idx, channel, row)


def _edit(W, name):
    W[name] = W[name].copy()
    return W[name]


def _bn_z(pre, W, k):
    m = W[f'layer_with_weights-{k}/moving_mean'].astype(np.float64)
    v = W[f'layer_with_weights-{k}/moving_variance'].astype(np.float64)
    return (pre - m) / np.sqrt(v + ref.nets.BN_EPS)


def _pre(net, W, u, kind):
    """what the site's BatchNorm reads: the (max-pooled) unit input, or conv_a's output"""
    inp = ref.nets.maxpool1d_same(net) if u in POOL_UNITS else net
    if kind == 'in':
        return inp
    return ref.nets._conv1(ref.nets.relu(ref.nets.batchnorm(inp, W, K_IN[u])), W, K_IN[u] + 1)


# ---- features -------------------------------------------------------------------------------------

def bumped(clip, row, T, t):
    """the base features with a bump of +-BUMP (sign pattern t) over the 256 / T source rows of the
    clip that pool down to `row` of T"""
    x = base_features().copy()
    ds = 256 // T
    sign = np.where(np.random.default_rng([SEED, t]).integers(0, 2, 39) == 1, 1.0, -1.0)
    x[clip, row * ds:(row + 1) * ds] = (BUMP * sign).astype(np.float32)
    return x


@functools.lru_cache(maxsize=8)
def _base(clip, row, T, t):
    """the unedited network on a bumped batch: every stage and the site summaries"""
    W = base_weights()
    x = bumped(clip, row, T, t)
    _, before, stages = walk(x, W)
    return W, x, stages, before


def _peaks(site, placement, t):
    """the channel of the site's BatchNorm input whose largest normalised value of the whole batch is on
    the target row, with the widest gap to its runner-up -> (c, top, runner-up, W, x, stages, before)"""
    u, kind = unit_of(site), site.split('.')[1]
    clip, row = target(site, placement)
    W, x, stages, before = _base(clip, row, ROWS[u], t)
    k = K_IN[u] + (0 if kind == 'in' else 2)
    z = _bn_z(_pre(stages[u - 1], W, u, kind), W, k)
    flat = z.reshape(-1, z.shape[-1])
    n, r = np.unravel_index(np.argmax(flat, axis=0), z.shape[:2])
    part = np.partition(flat, -2, axis=0)
    gap = part[-1] - part[-2]
    ok = (n == clip) & (r == row)
    if not ok.any():
        return None
    c = int(np.argmax(np.where(ok, gap, -1.0)))
    return c, part[-1, c], part[-2, c], W, x, stages, before


def _build_local(site, placement, hot):
    """one hot operand: BatchNorm channel c maps its largest normalised value to scale x limit and
    everything else below zero (ReLU: exactly 0); the conv that reads the operand ignores channel c"""
    u, kind = unit_of(site), site.split('.')[1]
    found = next((p for p in (_peaks(site, placement, t) for t in range(BUMP_TRIES)) if p), None)
    assert found, f'{site} {placement}: no channel peaks on the target row'
    c, top, second, W0, x, stages, before = found
    W = dict(W0)
    k = K_IN[u] + (0 if kind == 'in' else 2)
    t0 = 0.5 * (top + second)
    G = (HOT_SCALE if hot else CONTROL_SCALE) * LIMIT_CONV / (top - t0)
    _edit(W, f'layer_with_weights-{k}/gamma')[c] = G
    _edit(W, f'layer_with_weights-{k}/beta')[c] = -G * t0
    reader = k + 1 if kind == 'in' or u not in POOL_UNITS else k + 2     # conv_a; conv_b behind the shortcut
    _edit(W, f'layer_with_weights-{reader}/kernel')[:, c, :] = 0.0
    return _finish(site, placement, hot, W, x, u, stages[u - 1], before, c)


def _build_stem(placement, hot):
    """one feature of one row x scale x limit; the stem ignores that feature"""
    clip, row = target('stem', placement)
    W = dict(base_weights())
    x = base_features().copy()
    d = 7
    x[clip, row, d] = (HOT_SCALE if hot else CONTROL_SCALE) * LIMIT_CONV
    _edit(W, 'layer_with_weights-0/kernel')[:, d, :] = 0.0
    return _finish('stem', placement, hot, W, x, 1, None, {}, d)


def _build_sc1(placement, hot):
    """u1.sc: stem channel c = F x feature d of the same row (one tap), a feature spike of 0.45 x the
    limit in one row; BN_in of unit 1 and the shortcut ignore channel c.  An even row is one hot
    shortcut operand; an odd row none, although the stem output there is as large."""
    clip, row = SC1_ROWS[placement]
    W = dict(base_weights())
    x = base_features().copy()
    c, d = 3, 7
    spike = 0.45 * LIMIT_CONV
    x[clip, row, d] = spike
    kern = _edit(W, 'layer_with_weights-0/kernel')
    kern[:, :, c] = 0.0
    kern[1, d, c] = (HOT_SCALE if hot else CONTROL_SCALE) * LIMIT_CONV / spike    # tap 1 reads the row itself
    _edit(W, 'layer_with_weights-0/bias')[c] = 0.0
    _edit(W, 'layer_with_weights-1/gamma')[c] = 0.0
    _edit(W, 'layer_with_weights-1/beta')[c] = 0.0
    _edit(W, f'layer_with_weights-{K_IN[1] + 3}/kernel')[:, c, :] = 0.0
    return _finish('u1.sc', placement, hot, W, x, 1, None, {}, c)


def _build_channel(site, hot):
    """u4.sc, u7.sc: the bias of the conv that ends the unit before puts channel c of the unit's raw
    input at scale x limit in every row; the unit's BN_in and its shortcut ignore channel c.
    lstm: the final BatchNorm's channel c is the constant scale x limit; the BiLSTM ignores it."""
    W = dict(base_weights())
    x = base_features()
    _, before, stages = walk(x, W)
    c = 0
    B = (HOT_SCALE if hot else CONTROL_SCALE) * limit(site)
    if site == 'lstm':
        _edit(W, 'layer_with_weights-40/gamma')[c] = 0.0
        _edit(W, 'layer_with_weights-40/beta')[c] = B
        for d in ('forward', 'backward'):
            _edit(W, f'layer_with_weights-41/{d}/kernel')[c, :] = 0.0
        return _finish(site, 'channel', hot, W, x, 9, stages[8], before, c)
    u = unit_of(site)
    _edit(W, f'layer_with_weights-{K_IN[u - 1] + 3}/bias')[c] += B
    _edit(W, f'layer_with_weights-{K_IN[u]}/gamma')[c] = 0.0
    _edit(W, f'layer_with_weights-{K_IN[u]}/beta')[c] = 0.0
    _edit(W, f'layer_with_weights-{K_IN[u] + 3}/kernel')[:, c, :] = 0.0
    return _finish(site, 'channel', hot, W, x, u - 1, stages[u - 2], before, c)


PAST_SITES = tuple(f'u{u}.mid' for u in range(1, 10))
PAST_MID, PAST_GAIN = 0.3, 2.0     # the real operand and one copy more of it, in units of the limit


def _build_past_batch(site):
    """u<k>.mid, nothing hot in the batch, but out of range in the rows a tail workgroup computes past
    the batch.  Those rows stage copies of the batch's last row, so where unit k is the first of its
    launch their conv_a sees the last row's BN_in + ReLU output in every tap.  The u<k>.in control case
    at the batch's last row leaves ONE nonzero operand A = 0.25 x the limit in channel d; conv_a's
    channel c becomes the plain sum of channel d over its three taps (A in the last two rows of the
    batch, 0 elsewhere; 2 A and 3 A in the rows past it) and BN_mid's channel c maps A to 0.3 x the limit
    and each further A to 2 x the limit more; conv_b ignores channel c."""
    u = unit_of(site)
    base = build(f'u{u}.in', 'batch_end', False)
    W, d, c = dict(base.W), base.channel, 0
    k = K_IN[u]
    A = CONTROL_SCALE * LIMIT_CONV
    kern = _edit(W, f'layer_with_weights-{k + 1}/kernel')
    kern[:, :, c] = 0.0
    kern[:, d, c] = 1.0
    _edit(W, f'layer_with_weights-{k + 1}/bias')[c] = 0.0
    p = f'layer_with_weights-{k + 2}/'
    _edit(W, p + 'moving_mean')[c] = 0.0
    _edit(W, p + 'moving_variance')[c] = 1.0 - ref.nets.BN_EPS
    _edit(W, p + 'gamma')[c] = PAST_GAIN * LIMIT_CONV / A
    _edit(W, p + 'beta')[c] = (PAST_MID - PAST_GAIN) * LIMIT_CONV
    _edit(W, f'layer_with_weights-{k + (4 if u in POOL_UNITS else 3)}/kernel')[:, c, :] = 0.0
    return _finish(site, 'past_batch', False, W, base.x, 1, None, {}, c)


@functools.lru_cache(maxsize=None)
def build(site, placement, hot):
    """-> Case(site, placement, hot, W, x [5, 256, 39] float32, oracle probs [5, 8], amax {site:
    max |operand|}, hot_idx [k, 3] = (clip, row, channel) of the site's operands above 0.5 x its limit,
    channel, row = the one hot operand's row or None)"""
    if placement == 'past_batch':
        assert not hot
        return _build_past_batch(site)
    if site == 'stem':
        return _build_stem(placement, hot)
    if site == 'u1.sc':
        return _build_sc1(placement, hot)
    if placement == 'channel':
        return _build_channel(site, hot)
    return _build_local(site, placement, hot)


# ---- the launch plans the GPU tests run (tests/test_gpu_si_trace.py, test_gpu_si_range_sites.py) ----

SWITCHES = ('MMLA_NO_SIU', 'MMLA_NO_SIPU', 'MMLA_NO_SIFIN', 'MMLA_NO_SIPAD', 'MMLA_NO_SIPAIR', 'MMLA_NO_SICHAIN')
ALL_STAGES = tuple(range(13))
# path -> (switches set to 1, exact f32, the stages it writes to memory,
#          its siu launches: last unit -> (tile rows, units, ends the net with the fused pooling))
PATHS = {
    'default': ((), False, (0, 3, 6, 10, 11, 12), dict((u, DEFAULT_LAUNCH[u]) for u in (3, 6, 9))),
    'no_chain': (('MMLA_NO_SICHAIN',), False, (0, 1, 3, 4, 6, 7, 10, 11, 12),
                 {1: (256, 1, False), 3: (256, 2, False), 4: (128, 1, False), 6: (256, 2, False),
                  7: (64, 1, False), 9: (128, 2, True)}),
    'no_pair': (('MMLA_NO_SICHAIN', 'MMLA_NO_SIPAIR'), False, (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12),
                {1: (256, 1, False), 2: (256, 1, False), 3: (256, 1, False), 4: (128, 1, False),
                 5: (256, 1, False), 6: (256, 1, False), 7: (64, 1, False), 8: (128, 1, False), 9: (128, 1, True)}),
    'no_fin': (('MMLA_NO_SICHAIN', 'MMLA_NO_SIPAIR', 'MMLA_NO_SIFIN'), False, ALL_STAGES,
               {1: (256, 1, False), 2: (256, 1, False), 3: (256, 1, False), 4: (128, 1, False),
                5: (256, 1, False), 6: (256, 1, False), 7: (64, 1, False), 8: (128, 1, False), 9: (128, 1, False)}),
    'conv_h3': (SWITCHES, False, ALL_STAGES, {}),
    'f32': ((), True, ALL_STAGES, {}),
}


def context(ones=(), f32=False, k=K, guard=False, extra=()):
    """a context with every SI switch set explicitly, so the tests hold whatever the environment"""
    import pytest
    from mmla_audio_amd import _lib, weights
    with pytest.MonkeyPatch.context() as mp:
        for s in SWITCHES:
            mp.setenv(s, '1' if s in ones else '0')
        mp.setenv('MMLA_DEBUG_TRACE_GUARD', '1' if guard else '0')
        for s, v in extra:
            mp.setenv(s, v)
        c = _lib.Context(0)
    if f32:
        c.set_precision(_lib.PREC_F32)
    if k is not None:
        W = weights.synthetic(weights.SI, seed=SEED, n_classes=k)
        c.load_weights(weights.SI, weights.pack(weights.SI, W, k), k, _lib.HEAD_SIGMOID if k == K else _lib.HEAD_SOFTMAX)
    return c
