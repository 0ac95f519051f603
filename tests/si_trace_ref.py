"""SI-NET stage by stage in the oracle's own layer functions -- TEST INFRASTRUCTURE ONLY.

``walk`` calls oracle/nets.py's layers in the order of ``nets.si_forward`` (tests/
test_si_range_cases_cpu.py asserts that its last stage is si_forward's output bit for bit) and keeps
what mmla_debug_si_trace taps:

  stage 0       stem Conv1D(32, 4)                      [n, 256, 32]
  stage 1..9    output of res unit 1..9                 [n, 128, 32] x 3, [n, 64, 64] x 3, [n, 32, 128] x 3
  stage 10      final BN + ReLU + AveragePooling1D(4)   [n, 8, 128]
  stage 11      BiLSTM output                           [n, 512]
  stage 12      the logits                              [n, K]
  'probs'       softmax / sigmoid of stage 12

and, on request, the operands the 3xFP16 kernels split (tests/si_range_cases.py SITES): the raw
features (``stem``), per unit ``u<k>.in`` = ReLU(BN_in(x)) (units 1, 4, 7: of the max-pooled x) and
``u<k>.mid`` = ReLU(BN_mid(conv_a)), the raw input of units 1, 4, 7 at even rows (``u<k>.sc``) and the
BiLSTM's input sequence (``lstm``).
"""
import numpy as np

from oracle import nets

# unit -> index of its BN_in; then conv_a, BN_mid, [shortcut,] conv_b
K_IN = {1: 1, 2: 6, 3: 10, 4: 14, 5: 19, 6: 23, 7: 27, 8: 32, 9: 36}
POOL_UNITS = tuple(u for u in range(1, 10) if nets.POOL[u - 1])
ROWS = {u: 256 >> (1 + (u - 1) // 3) for u in range(1, 10)}     # a unit's (pooled) rows per clip
STAGES = tuple(range(13))


def unit(net, W, u, sites=None):
    """res unit u (1-based) on its input, nets.si_forward's loop body; records its split operands"""
    k = K_IN[u]
    pool = u in POOL_UNITS
    inp = nets.maxpool1d_same(net) if pool else net
    a = nets.relu(nets.batchnorm(inp, W, k))
    t = nets._conv1(a, W, k + 1)
    m = nets.relu(nets.batchnorm(t, W, k + 2))
    if pool:
        res = nets._conv1(net, W, k + 3, stride=2)
        out = nets._conv1(m, W, k + 4)
    else:
        res = net
        out = nets._conv1(m, W, k + 3)
    if sites is not None:
        if pool:
            sites[f'u{u}.sc'] = net[:, ::2]
        sites[f'u{u}.in'] = a
        sites[f'u{u}.mid'] = m
    return res + out


def walk(x, W, head='sigmoid', dtype=np.float64, first=1, net=None, sites=None):
    """-> {stage: tensor, 'probs': [n, K]} from unit `first` on (net: that unit's input, i.e. stage
    first - 1; default: the stem of the features x, then stage 0 is returned too).  sites: a dict that
    receives the split operands of what was walked"""
    out = {}
    if net is None:
        assert first == 1
        x = np.asarray(x, dtype=dtype)
        if sites is not None:
            sites['stem'] = x
        net = nets._conv1(x, W, 0)
        out[0] = net
    net = np.asarray(net, dtype=dtype)
    for u in range(first, 10):
        net = unit(net, W, u, sites)
        out[u] = net
    net = nets.relu(nets.batchnorm(net, W, 40))
    n, t, c = net.shape
    seq = net[:, :t // 4 * 4].reshape(n, t // 4, 4, c).mean(axis=2)
    if sites is not None:
        sites['lstm'] = seq
    out[10] = seq
    out[11] = nets.bilstm(seq, W, 41)
    out[12] = out[11] @ W['layer_with_weights-42/kernel'].astype(dtype) + W['layer_with_weights-42/bias'].astype(dtype)
    out['probs'] = nets.softmax(out[12]) if head == 'softmax' else nets.sigmoid(out[12])
    return out
