"""TEST INFRASTRUCTURE: torch-CPU restatement, with autograd on, of what ``mmla_si_loss_grad`` and
``mmla_si_finetune`` (include/mmla.h) compute -- stage 2 of the reference's ``transfer_learning``
(speaker_identification.py:438-454) as Keras 2.6's published source defines it.  TensorFlow is not
available; parity with TF itself is unpinned.

The graph is ``oracle.nets_torch.Nets``'s building blocks (conv1d with Keras 'same' padding, BN on the
moving statistics with eps 1e-3) in the order of ``Nets.si_forward``; the BiLSTM is restated as an
explicit 8-step loop because ``Nets.bilstm`` copies its weights out of the graph.

  loss      mean_b[-log(clip(s_c / sum_k s_k, 1e-7, 1 - 1e-7))] + R
  R         0.1 sum w^2 over the kernels of layer_with_weights-20, 22, 24, 26
            + 0.2 sum w^2 over those of layer_with_weights-33, 35, 37, 39
  RMSprop   rms <- 0.9 rms + 0.1 g^2; v <- v - lr g / (sqrt(rms) + 1e-7), every accumulator from 0
  frozen    moving_mean, moving_variance (gradient reported as 0, value never updated)

Every function takes ``dtype`` (torch.float64: the reference; torch.float32: the arithmetic the kernels
are held to, with torch's summation orders).
"""
import numpy as np
import torch
import torch.nn.functional as F

from mmla_audio_amd import weights
from oracle.nets_torch import POOL, Nets

L2 = {20: 0.1, 22: 0.1, 24: 0.1, 26: 0.1, 33: 0.2, 35: 0.2, 37: 0.2, 39: 0.2}
L2_NAMES = {f'layer_with_weights-{k}/kernel': lam for k, lam in L2.items()}


def is_frozen(role):
    return role in ('bn_mean', 'bn_var')


class _Net(Nets):
    """Nets with the tensors of W as autograd leaves and a BiLSTM inside the graph."""

    def __init__(self, W, dtype):
        super().__init__(W, dtype)
        self.relu_min = np.inf      # filled by logits(): the margins of the last forward
        self.pool_min = np.inf

    def bilstm(self, seq, k):
        p = f'layer_with_weights-{k}'
        outs = []
        for side in ('forward', 'backward'):
            wk, wr, b = (self.W[f'{p}/{side}/{v}'] for v in ('kernel', 'recurrent_kernel', 'bias'))
            h = seq.new_zeros(seq.shape[0], 256)
            c = seq.new_zeros(seq.shape[0], 256)
            steps = range(seq.shape[1]) if side == 'forward' else range(seq.shape[1] - 1, -1, -1)
            for t in steps:
                z = seq[:, t] @ wk + h @ wr + b
                i, f, g, o = z[:, :256], z[:, 256:512], z[:, 512:768], z[:, 768:]
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        return torch.cat(outs, dim=1)

    def _relu_bn(self, x, k):
        pre = self.bn(x, k)
        self.relu_min = min(self.relu_min, float(pre.detach().abs().min()))
        return F.relu(pre)

    def _pool(self, x):
        assert x.shape[2] % 2 == 0                     # T = 256 / 128 / 64: 'same' pads nothing
        d = x.detach()
        self.pool_min = min(self.pool_min, float((d[:, :, 0::2] - d[:, :, 1::2]).abs().min()))
        return F.max_pool1d(x, 2)

    def embed(self, x):
        """x [N,256,39] -> the BiLSTM output [N,512] (the graph of Nets.si_forward)"""
        self.relu_min = self.pool_min = np.inf
        x = torch.as_tensor(np.asarray(x)).to(self.dtype).permute(0, 2, 1)
        net = self.conv1d(x, 0)
        k = 1
        for pool in POOL:
            inp = self._pool(net) if pool else net
            out = self.conv1d(self._relu_bn(inp, k), k + 1)
            out = self._relu_bn(out, k + 2)
            if pool:
                res = self.conv1d(net, k + 3, 2)
                out = self.conv1d(out, k + 4)
                k += 5
            else:
                res = net
                out = self.conv1d(out, k + 3)
                k += 4
            net = res + out
        net = self._relu_bn(net, 40)
        net = F.avg_pool1d(net, 4)
        return self.bilstm(net.permute(0, 2, 1), 41)

    def sigmoids(self, x):
        z = self.embed(x) @ self.W['layer_with_weights-42/kernel'] + self.W['layer_with_weights-42/bias']
        return torch.sigmoid(z)

    def penalty(self):
        r = None
        for name, lam in L2_NAMES.items():
            t = lam * (self.W[name] ** 2).sum()
            r = t if r is None else r + t
        return r


def _data_terms(s, labels, dtype):
    """-> (per-sample loss tensor, hits, smallest top-two gap)"""
    one = torch.ones((), dtype=dtype)
    lo = torch.tensor(1e-7, dtype=dtype)
    hi = one - lo
    idx = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    p = s[torch.arange(len(idx)), idx] / s.sum(dim=1)
    loss = -torch.log(torch.clamp(p, lo, hi))         # clamp passes the gradient inside [lo, hi] only
    d = s.detach()
    hits = int((d.argmax(dim=1) == idx).sum())        # first index wins a tie
    gap = np.inf
    if d.shape[1] > 1:
        top = torch.sort(d, dim=1).values
        gap = float((top[:, -1] - top[:, -2]).min())
    return loss, hits, gap


def forward(W, x, dtype=torch.float64):
    """sigmoid-head outputs [N,K] (numpy), no graph kept"""
    with torch.no_grad():
        return _Net(W, dtype).sigmoids(x).numpy()


def loss_and_grad(W, K, x, labels, dtype=torch.float64):
    """One batch -> (data term, R, {name: gradient of data + R}) with 0 for the moving statistics."""
    net = _Net(W, dtype)
    spec = weights.si_spec(K)
    for name, _, role in spec:
        net.W[name].requires_grad_(not is_frozen(role))
    loss, _, _ = _data_terms(net.sigmoids(x), labels, dtype)
    data, r = loss.mean(), net.penalty()
    (data + r).backward()
    g = {name: (np.zeros(shape, np.float64) if is_frozen(role) else net.W[name].grad.numpy().astype(np.float64))
         for name, shape, role in spec}
    return float(data.detach()), float(r.detach()), g


def margins(W, K, x, labels=None, dtype=torch.float64):
    """-> (smallest |pre-activation| at any ReLU, smallest gap inside any max-pool pair, smallest
    top-two sigmoid gap) over the batch"""
    with torch.no_grad():
        net = _Net(W, dtype)
        s = net.sigmoids(x)
        _, _, gap = _data_terms(s, np.zeros(len(s), np.int64) if labels is None else labels, dtype)
    return net.relu_min, net.pool_min, gap


def fit(W, K, x, labels, val_x, val_labels, perm, epochs, batch=8, lr=1e-6, dtype=torch.float64,
        frozen_base=False, penalty=True):
    """The arguments of mmla_si_finetune (perm [epochs, n]).  frozen_base: only the head is trainable;
    penalty=False drops R (together: stage 1 restated, see the CPU tests).
    -> ({name: float64 array} fine-tuned, history [epochs,4] float64, dict(relu, pool, gap) = the
    smallest margins met in any forward of the fit)"""
    net = _Net(W, dtype)
    spec = weights.si_spec(K)
    head = {spec[-2][0], spec[-1][0]}
    train = [n for n, _, role in spec if not is_frozen(role) and (not frozen_base or n in head)]
    for n in train:
        net.W[n].requires_grad_(True)
    rms = {n: torch.zeros_like(net.W[n]) for n in train}
    labels = np.asarray(labels)
    x = np.asarray(x)
    n = len(labels)
    nv = 0 if val_labels is None else len(val_labels)
    lr_t = torch.tensor(float(np.float32(lr)), dtype=dtype)      # the ABI's lr argument is a float
    rho, rest, eps = (torch.tensor(v, dtype=dtype) for v in (0.9, 0.1, 1e-7))
    hist = np.full((epochs, 4), np.nan, np.float64)
    m = dict(relu=np.inf, pool=np.inf, gap=np.inf)

    def note(gap):
        m['relu'] = min(m['relu'], net.relu_min)
        m['pool'] = min(m['pool'], net.pool_min)
        m['gap'] = min(m['gap'], gap)

    zero = torch.zeros((), dtype=dtype)
    for ep in range(epochs):
        tot, hits = 0.0, 0
        for i0 in range(0, n, batch):
            idx = np.asarray(perm[ep, i0:i0 + batch])
            for t in train:
                net.W[t].grad = None
            loss, h, gap = _data_terms(net.sigmoids(x[idx]), labels[idx], dtype)
            note(gap)
            r = net.penalty() if penalty else zero
            total = loss.mean() + r
            total.backward()
            tot += float(total.detach()) * len(idx)
            hits += h
            with torch.no_grad():
                for t in train:
                    g = net.W[t].grad
                    rms[t].mul_(rho).add_(rest * g * g)
                    net.W[t].sub_(lr_t * g / (torch.sqrt(rms[t]) + eps))
        hist[ep, 0] = tot / n
        hist[ep, 1] = hits / n
        if nv:
            with torch.no_grad():
                loss, h, gap = _data_terms(net.sigmoids(val_x), val_labels, dtype)
                note(gap)
                r = net.penalty() if penalty else zero
                hist[ep, 2] = float(loss.mean() + r)
                hist[ep, 3] = h / nv
    return {k: v.detach().numpy().astype(np.float64) for k, v in net.W.items()}, hist, m
