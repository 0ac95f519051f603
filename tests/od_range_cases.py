"""OD-NET inputs that drive exactly one 3xFP16 split site out of range -- TEST INFRASTRUCTURE ONLY.

OD-NET splits an activation into fp16 hi + lo at 22 places (SITES): the two conv operands of each
res_block (``b<k>.in`` = ELU(BN_in(x)), ``b<k>.mid`` = ELU(BN_mid(conv1))), the raw block input the
strided shortcut of blocks 1, 4, 7 reads at ``[::2, ::2]`` (``b<k>.sc``) and the BiLSTM input
(``lstm``, the mean over H of block 9's output).  Conv operands are split at 2^4, so the limit is
65504 / 16 = 4094 (f16x3.h ACT_SCALE, SPLIT_MAX; conv_h3.hip / resblk.hip ACT_RANGE); the BiLSTM
input at 2^6, limit 1023.5 (nets.hip LSTM_AS).

``build(site, placement, hot)`` returns weights (synthetic seed 5, edited) and a 3-clip float image
for which, in the float64 oracle walk below,
  * hot: the targeted site is >= 2 x its limit, every other site <= 0.5 x its limit;
  * control (hot=False): the same construction at 0.25 x the limit, every site <= 0.5 x its limit;
  * the probabilities are finite, because the hot channel's downstream weights are zero.
For ``.in`` / ``.mid`` sites exactly ONE operand of the whole batch is hot, at a pixel steered by a
bright patch into a chosen clip and region (PLACEMENTS), so a range fold that loses a lane, a strip
of a pair or an absent pair clip shows.  tests/test_od_range_cases_cpu.py asserts these conditions;
tests/test_gpu_od_range_sites.py runs the cases.

3 clips: block 1's ragged last strips (image columns 144-150) are paired per two clips, so clips
0 and 1 share a workgroup and clip 2's tail is the unpaired one; blocks 7-9 run two strips per
workgroup and 3 x 19 / 3 x 5 strips are odd, so the last workgroup's second strip is absent.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import nets

N = 3
SEED = 5
LIMIT_CONV = 65504.0 / 16.0
LIMIT_LSTM = 65504.0 / 64.0
HOT_SCALE, CONTROL_SCALE = 4.0, 0.25

# block -> index of its BN_in (then conv1, BN_mid, conv2[, shortcut]), input height / width, the
# downsampling of its input against the image, first column of the kernels' last column strip
K_IN = {1: 1, 2: 6, 3: 10, 4: 14, 5: 19, 6: 23, 7: 27, 8: 32, 9: 36}
GEOM = {1: (128, 151, 1, 144), 2: (64, 76, 2, 64), 3: (64, 76, 2, 64), 4: (64, 76, 2, 74),
        5: (32, 38, 4, 36), 6: (32, 38, 4, 36), 7: (32, 38, 4, 36), 8: (16, 19, 8, 16), 9: (16, 19, 8, 16)}
POOL_BLOCKS = (1, 4, 7)
SITES = tuple(s for b in range(1, 10)
              for s in ([f'b{b}.sc'] if b in POOL_BLOCKS else []) + [f'b{b}.in', f'b{b}.mid']) + ('lstm',)
assert len(SITES) == 22
LOCAL_SITES = tuple(s for s in SITES if s.endswith(('.in', '.mid')))
# where the one hot operand goes: clip, and the region of the site's [H, W] it must lie in
PLACEMENTS = ('first', 'pair_last_row', 'lone_tail')
PLACE_CLIP = {'first': 0, 'pair_last_row': 1, 'lone_tail': 2}
# b1.sc on a black image with one 255 pixel: (clip, row, col); the odd pixel is never read
SC1_PIXELS = {'first': (0, 0, 0), 'pair_last_row': (1, 126, 150), 'lone_tail': (2, 64, 146), 'odd': (1, 65, 77)}

Case = namedtuple('Case', 'site placement hot W x probs amax hot_idx channel')


def limit(site):
    return LIMIT_LSTM if site == 'lstm' else LIMIT_CONV


def block_of(site):
    return 10 if site == 'lstm' else int(site[1])


def case_ids():
    """every (site, placement) the GPU tests run, grouped so that consecutive cases share an image"""
    ids = []
    for ds in (1, 2, 4, 8):
        for p in PLACEMENTS:
            ids += [(s, p) for s in LOCAL_SITES if GEOM[int(s[1])][2] == ds]
    ids += [('b1.sc', p) for p in SC1_PIXELS]
    ids += [('b4.sc', 'channel'), ('b7.sc', 'channel'), ('lstm', 'channel')]
    return ids


def base_weights():
    from mmla_audio_amd import weights
    return weights.synthetic(weights.OD, seed=SEED)


# ---- the oracle walk ------------------------------------------------------------------------------

def _block(net, W, b, sites):
    """res_block b on its input; records its split operands; -> (output, conv1's raw output)"""
    k = K_IN[b]
    pool = b in POOL_BLOCKS
    if pool:
        sites[f'b{b}.sc'] = net[:, ::2, ::2]
    a = nets.elu(nets.batchnorm(net, W, k))
    sites[f'b{b}.in'] = a
    t = nets._conv(a, W, k + 1)
    m = nets.elu(nets.batchnorm(t, W, k + 2))
    sites[f'b{b}.mid'] = m
    o = nets._conv(m, W, k + 3)
    if pool:
        res = nets._conv(net, W, k + 4, stride=2)
        o = nets.maxpool2d_same(o)
    else:
        res = net
    return res + o, t


def _tail(net, W, sites):
    seq = net.mean(axis=nets.MEAN_AXIS)
    sites['lstm'] = seq
    h = nets.bilstm(seq, W, 40)
    h = np.where(h > 0, h, h * np.float64(nets.LEAKY_ALPHA))
    z = h @ W['layer_with_weights-41/kernel'].astype(np.float64) + W['layer_with_weights-41/bias'].astype(np.float64)
    return nets.softmax(z)


def walk(x, W, first=1, net=None, keep=None):
    """float64 OD-NET from block `first` on (net: that block's input; default the stem of image x)
    -> (probs, {site: operand tensor}, [the input of every block walked]).  keep: called with the
    dict of sites after every block to drop tensors that are no longer needed"""
    if net is None:
        net = nets._conv(np.asarray(x, np.float64), W, 0)
    sites, inputs = {}, []
    for b in range(first, 10):
        inputs.append(net)
        net, _ = _block(net, W, b, sites)
        if keep:
            keep(sites)
    probs = _tail(net, W, sites)
    if keep:
        keep(sites)
    return probs, sites, inputs


def _summary(sites, out):
    """site tensors -> {site: (max |operand|, indices of the operands above 0.5 x the limit)}"""
    for s in list(sites):
        v = sites[s]
        if isinstance(v, tuple):
            continue
        a = np.abs(v)
        out[s] = (float(a.max()), np.argwhere(a > 0.5 * limit(s)))
        sites[s] = out[s]


# ---- images ---------------------------------------------------------------------------------------

def image(placement, ds, value=255.0):
    """dim noise (0..32) with a 255-valued patch, 2 ds pixels square (ds = 1: one pixel), in the
    placement's clip: top-left corner, bottom-right corner or the last columns at row 64"""
    x = np.random.default_rng(1000 + ds).integers(0, 33, size=(N, 128, 151, 3)).astype(np.float32)
    s = 1 if ds == 1 else 2 * ds
    r0, c0 = {'first': (0, 0), 'pair_last_row': (128 - s, 151 - s), 'lone_tail': (64, 151 - s)}[placement]
    x[PLACE_CLIP[placement], r0:r0 + s, c0:c0 + s] = value
    return x


def _region(site, placement):
    """mask over the site's [H, W]: where the placement wants the hot operand"""
    h, w, _, last = GEOM[int(site[1])]
    m = np.zeros((h, w), bool)
    if placement == 'first':
        m[0, 0] = True
    elif placement == 'pair_last_row':
        m[h - 1, last:] = True
    else:
        m[:, last:] = True
    return m


@functools.lru_cache(maxsize=4)
def _base(placement, ds):
    """the unedited network on a placement's image: every block's input and the site summaries"""
    W = base_weights()
    x = image(placement, ds)
    out = {}
    probs, _, inputs = walk(x, W, keep=lambda s: _summary(s, out))
    return W, x, inputs, out


@functools.lru_cache(maxsize=4)
def _base_sc1(placement):
    W = base_weights()
    x = np.zeros((N, 128, 151, 3), np.float32)
    c, r, q = SC1_PIXELS[placement]
    x[c, r, q] = 255.0
    return W, x


def _finish(site, placement, hot, W, x, first, net, before, channel):
    """walk the edited network from block `first`; the sites before it are the unedited ones"""
    amax = {s: v[0] for s, v in before.items() if block_of(s) < first}
    out = {}
    probs, _, _ = walk(x, W, first, net, keep=lambda s: _summary(s, out))
    amax.update({s: v[0] for s, v in out.items()})
    return Case(site, placement, hot, W, x, probs, amax, out[site][1], channel)


def _bn_z(pre, W, k):
    m = W[f'layer_with_weights-{k}/moving_mean'].astype(np.float64)
    v = W[f'layer_with_weights-{k}/moving_variance'].astype(np.float64)
    return (pre - m) / np.sqrt(v + nets.BN_EPS)


def _build_local(site, placement, hot):
    """one hot operand: BatchNorm channel c maps its largest normalised value to scale x limit and
    everything else below zero (ELU then gives (-1, 0)); conv k + 1 ignores channel c"""
    b, kind = int(site[1]), site.split('.')[1]
    ds = GEOM[b][2]
    W0, x, inputs, before = _base(placement, ds)
    W = dict(W0)
    net = inputs[b - 1]
    k = K_IN[b] + (0 if kind == 'in' else 2)
    pre = net if kind == 'in' else nets._conv(nets.elu(nets.batchnorm(net, W, K_IN[b])), W, K_IN[b] + 1)
    z = _bn_z(pre, W, k)
    flat = z.reshape(-1, z.shape[-1])
    top = np.argmax(flat, axis=0)
    n, hh, ww = np.unravel_index(top, z.shape[:3])
    ok = (n == PLACE_CLIP[placement]) & _region(site, placement)[hh, ww]
    assert ok.any(), f'{site} {placement}: no channel peaks in the region'
    part = np.partition(flat, -2, axis=0)
    gap = np.where(ok, part[-1] - part[-2], -1.0)
    c = int(np.argmax(gap))
    t = 0.5 * (part[-1, c] + part[-2, c])
    G = (HOT_SCALE if hot else CONTROL_SCALE) * LIMIT_CONV / (part[-1, c] - t)
    p = f'layer_with_weights-{k}/'
    W[p + 'gamma'] = W[p + 'gamma'].copy()
    W[p + 'beta'] = W[p + 'beta'].copy()
    W[p + 'gamma'][c] = G
    W[p + 'beta'][c] = -G * t
    kn = f'layer_with_weights-{k + 1}/kernel'
    W[kn] = W[kn].copy()
    W[kn][:, :, c, :] = 0.0
    return _finish(site, placement, hot, W, x, b, net, before, c)


def _scale_conv_channel(W, k, c, f):
    for v in ('kernel', 'bias'):
        name = f'layer_with_weights-{k}/{v}'
        W[name] = W[name].copy()
        W[name][..., c] *= f


def _renorm_bn(W, k, c, f):
    for v, g in (('moving_mean', f), ('moving_variance', f * f)):
        name = f'layer_with_weights-{k}/{v}'
        W[name] = W[name].copy()
        W[name][c] *= g


def _zero_row(W, name, c):
    W[name] = W[name].copy()
    W[name][..., c, :] = 0.0


def _build_sc1(placement, hot):
    """b1.sc: the stem's channel c x F on a black image with one 255 pixel; BN-1 renormalised; the
    shortcut ignores channel c.  An even pixel is one hot shortcut operand, an odd one none."""
    W0, x = _base_sc1(placement)
    W = dict(W0)
    k0 = W['layer_with_weights-0/kernel']
    resp = 255.0 * k0[0, 0].sum(axis=0).astype(np.float64)
    c = int(np.argmax(np.abs(resp)))
    F = (HOT_SCALE if hot else CONTROL_SCALE) * LIMIT_CONV / abs(resp[c])
    _scale_conv_channel(W, 0, c, F)
    W['layer_with_weights-0/bias'][c] = 0.0
    _renorm_bn(W, 1, c, F)
    _zero_row(W, 'layer_with_weights-5/kernel', c)
    return _finish('b1.sc', placement, hot, W, x, 1, None, {}, c)


def _build_channel(site, hot):
    """b4.sc, b7.sc, lstm: channel c of the conv that produces the operand x F (the whole channel is
    hot; the residual part of it is not scaled), the next BN_in renormalised, the reader's row c zero"""
    prod = {'b4.sc': 3, 'b7.sc': 6, 'lstm': 9}[site]
    W0, x, inputs, before = _base('first', 2)
    W = dict(W0)
    net = inputs[prod - 1]
    kc = K_IN[prod] + 3
    c = 0
    sites = {}
    out, _ = _block(net, W, prod, sites)
    o = out - net                                   # the conv's share of channel c, bias included
    o = o.mean(axis=1)[..., c] if site == 'lstm' else o[:, ::2, ::2, c]
    F = (HOT_SCALE if hot else CONTROL_SCALE) * limit(site) / float(np.abs(o).max())
    _scale_conv_channel(W, kc, c, F)
    if site == 'lstm':
        _zero_row(W, 'layer_with_weights-40/forward/kernel', c)
        _zero_row(W, 'layer_with_weights-40/backward/kernel', c)
    else:
        _renorm_bn(W, kc + 1, c, F)
        _zero_row(W, f'layer_with_weights-{kc + 5}/kernel', c)
    return _finish(site, 'channel', hot, W, x, prod, net, before, c)


def build(site, placement, hot):
    """-> Case(site, placement, hot, W, x [3, 128, 151, 3] float32, oracle probs [3, 2], amax {site:
    max |operand|}, hot_idx [k, 4] = (clip, row, col, channel) of the site's operands above 0.5 x its
    limit, channel)"""
    if site == 'b1.sc':
        return _build_sc1(placement, hot)
    if placement == 'channel':
        return _build_channel(site, hot)
    return _build_local(site, placement, hot)
