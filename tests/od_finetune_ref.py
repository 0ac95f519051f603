"""TEST INFRASTRUCTURE: torch-CPU restatement, with autograd on, of what ``mmla_od_loss_grad`` and
``mmla_od_finetune`` (include/mmla.h) compute -- ``OverlapDetector.continue_train_model``
(OverlapDetection/scripts/overlap_detector.py:480-509) as Keras 2.6's published source defines it.
TensorFlow is not available; parity with TF itself is unpinned.

The graph is ``oracle.nets_torch.Nets``'s building blocks (conv2d with Keras 'same' padding, BN eps 1e-3) in
the order of ``Nets.od_forward``; the BiLSTM is restated as an explicit loop because ``Nets.bilstm`` copies
its weights out of the graph.

  training  BatchNorm on batch statistics (biased variance); moving <- 0.99 moving + 0.01 batch with the
            Bessel-corrected variance (x N / max(N - 1, 1)); dropout = x * float32(1 / 0.75) * mask with
            the given masks (None: all kept)
  inference moving statistics, no dropout (the validation passes; equals Nets.od_forward)
  loss      p <- p / sum p; clip(p, 1e-7, 1 - 1e-7); mean_b[-w_c log p_c]
  Adadelta  a <- rho a + (1 - rho) g^2; u = sqrt(d + eps) / sqrt(a + eps) g; v <- v - lr u;
            d <- rho d + (1 - rho) u^2; rho 0.95, eps 1e-7, every accumulator from 0
  frozen    moving_mean, moving_variance (gradient reported as 0; only the BN update moves them)

Every function takes ``dtype`` (torch.float64: the reference; torch.float32: the arithmetic the kernels are
held to, with torch's summation orders).
"""
import numpy as np
import torch
import torch.nn.functional as F

from mmla_audio_amd import weights
from oracle.nets_torch import LEAKY_ALPHA, POOL, Nets

SPEC = weights.od_spec()
KEEP_SCALE = float(np.float32(1.0) / np.float32(0.75))
CLIP_LO = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))
HEAD = 'layer_with_weights-41'


def is_frozen(role):
    return role in ('bn_mean', 'bn_var')


class _Net(Nets):
    """Nets with the tensors of W as autograd leaves, training-mode BN and a BiLSTM inside the graph."""

    def __init__(self, W, dtype):
        super().__init__(W, dtype)
        self.pool_min = np.inf      # the margins of the last forward
        self.leaky_min = np.inf

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

    def bn_train(self, x, k):
        """batch statistics over N, H, W; the moving statistics advance in place"""
        mean = x.mean(dim=(0, 2, 3))
        var = ((x - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
        n = x.shape[0] * x.shape[2] * x.shape[3]
        with torch.no_grad():
            mm, mv = self._w(k, 'moving_mean'), self._w(k, 'moving_variance')
            mm.mul_(0.99).add_(0.01 * mean)
            mv.mul_(0.99).add_(0.01 * var * (n / max(n - 1, 1)))
        xh = (x - mean[None, :, None, None]) / torch.sqrt(var + 1e-3)[None, :, None, None]
        return xh * self._w(k, 'gamma')[None, :, None, None] + self._w(k, 'beta')[None, :, None, None]

    def _pool(self, x):
        h, w = x.shape[2], x.shape[3]
        xp = F.pad(x, (0, w % 2, 0, h % 2), value=-np.inf)
        d = xp.detach()
        cand = torch.stack([d[:, :, 0::2, 0::2], d[:, :, 0::2, 1::2], d[:, :, 1::2, 0::2], d[:, :, 1::2, 1::2]])
        top = torch.sort(cand, dim=0).values
        gap = top[3] - top[2]                       # inf where only one candidate is inside
        self.pool_min = min(self.pool_min, float(gap.min()))
        return F.max_pool2d(xp, 2)

    def logits(self, x, mask=None, train=False):
        """x uint8 [N,h,w,3] -> the Dense(2) outputs [N,2]; mask [N,512] (train only, None = keep all)"""
        self.pool_min = self.leaky_min = np.inf
        bn = self.bn_train if train else self.bn
        x = torch.as_tensor(np.asarray(x, np.float64)).to(self.dtype).permute(0, 3, 1, 2)
        net = self.conv2d(x, 0)
        k = 1
        for pool in POOL:
            out = self.conv2d(F.elu(bn(net, k)), k + 1)
            out = self.conv2d(F.elu(bn(out, k + 2)), k + 3)
            if pool:
                res = self.conv2d(net, k + 4, 2)
                out = self._pool(out)
                k += 5
            else:
                res = net
                k += 4
            net = res + out
        seq = net.mean(dim=2).permute(0, 2, 1)
        h = self.bilstm(seq, 40)
        if train:
            h = h * torch.tensor(KEEP_SCALE, dtype=self.dtype)
            if mask is not None:
                h = h * torch.as_tensor(np.asarray(mask) != 0).to(self.dtype)
        live = h.detach()[h.detach() != 0]
        self.leaky_min = float(live.abs().min()) if live.numel() else np.inf
        h = F.leaky_relu(h, LEAKY_ALPHA)
        return h @ self.W[HEAD + '/kernel'] + self.W[HEAD + '/bias']


def _loss_terms(z, labels, class_w, dtype):
    """-> (per-sample weighted loss tensor, hits)"""
    idx = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    p = torch.softmax(z, 1)
    p = p / p.sum(dim=1, keepdim=True)
    pc = p[torch.arange(len(idx)), idx]
    lo, hi = torch.tensor(CLIP_LO, dtype=dtype), torch.tensor(CLIP_HI, dtype=dtype)
    w = torch.as_tensor(np.asarray(class_w, np.float32).astype(np.float64)).to(dtype)[idx]
    loss = -w * torch.log(torch.clamp(pc, lo, hi))     # clamp passes the gradient inside [lo, hi] only
    hits = int((p.detach().argmax(dim=1) == idx).sum())   # first index wins a tie
    return loss, hits


def forward(W, x, dtype=torch.float64):
    """inference-mode softmax outputs [N,2] (numpy), no graph kept"""
    with torch.no_grad():
        return torch.softmax(_Net(W, dtype).logits(x), 1).numpy()


def _numpy(net):
    return {k: v.detach().numpy().astype(np.float64) for k, v in net.W.items()}


def loss_and_grad(W, x, labels, class_w=(1.0, 1.0), mask=None, dtype=torch.float64):
    """One training-mode batch -> (loss, {name: gradient} with 0 for the moving statistics, {name: value}
    after the step's moving-statistics update, dict(pool, leaky) = the margins of the forward)"""
    net = _Net(W, dtype)
    for name, _, role in SPEC:
        net.W[name].requires_grad_(not is_frozen(role))
    loss, _ = _loss_terms(net.logits(x, mask, True), labels, class_w, dtype)
    total = loss.mean()
    total.backward()
    g = {name: (np.zeros(shape, np.float64) if is_frozen(role) else net.W[name].grad.numpy().astype(np.float64))
         for name, shape, role in SPEC}
    return float(total.detach()), g, _numpy(net), dict(pool=net.pool_min, leaky=net.leaky_min)


def loss_only(W, x, labels, class_w, mask, dtype=torch.float64):
    with torch.no_grad():
        net = _Net(W, dtype)
        loss, _ = _loss_terms(net.logits(x, mask, True), labels, class_w, dtype)
        return float(loss.mean())


def fit(W, x, labels, val_x, val_labels, class_w, lr, perm, masks, epochs, batch, patience=0,
        dtype=torch.float64):
    """The arguments of mmla_od_finetune (lr [epochs], perm [epochs, n], masks [epochs, n, 512] or None).
    -> ({name: float64 array}, history [epochs,5] float64 (NaN rows after an early stop), epochs_run,
    dict(pool, leaky) = the smallest margins met in any forward of the fit)"""
    net = _Net(W, dtype)
    train = [n for n, _, role in SPEC if not is_frozen(role)]
    for n in train:
        net.W[n].requires_grad_(True)
    acc_g = {n: torch.zeros_like(net.W[n]) for n in train}
    acc_d = {n: torch.zeros_like(net.W[n]) for n in train}
    labels = np.asarray(labels)
    x = np.asarray(x)
    n = len(labels)
    nv = 0 if val_labels is None else len(val_labels)
    rho, eps = torch.tensor(0.95, dtype=dtype), torch.tensor(1e-7, dtype=dtype)
    rest = 1 - rho
    hist = np.full((epochs, 5), np.nan, np.float64)
    m = dict(pool=np.inf, leaky=np.inf)

    def note():
        m['pool'] = min(m['pool'], net.pool_min)
        m['leaky'] = min(m['leaky'], net.leaky_min)

    best, wait, ran = np.inf, 0, 0
    for ep in range(epochs):
        lr_t = torch.tensor(float(np.float32(lr[ep])), dtype=dtype)
        tot, hits = 0.0, 0
        for i0 in range(0, n, batch):
            idx = np.asarray(perm[ep, i0:i0 + batch])
            for t in train:
                net.W[t].grad = None
            mk = None if masks is None else np.asarray(masks)[ep][idx]
            loss, h = _loss_terms(net.logits(x[idx], mk, True), labels[idx], class_w, dtype)
            note()
            total = loss.mean()
            total.backward()
            tot += float(total.detach()) * len(idx)
            hits += h
            with torch.no_grad():
                for t in train:
                    g = net.W[t].grad
                    acc_g[t].mul_(rho).add_(rest * g * g)
                    u = torch.sqrt(acc_d[t] + eps) / torch.sqrt(acc_g[t] + eps) * g
                    net.W[t].sub_(lr_t * u)
                    acc_d[t].mul_(rho).add_(rest * u * u)
        hist[ep] = (tot / n, hits / n, np.nan, np.nan, float(np.float32(lr[ep])))
        if nv:
            with torch.no_grad():
                loss, h = _loss_terms(net.logits(val_x), val_labels, class_w, dtype)
                hist[ep, 2] = float(loss.mean())
                hist[ep, 3] = h / nv
        ran = ep + 1
        if patience > 0 and nv:
            if hist[ep, 2] < best:
                best, wait = hist[ep, 2], 0
            else:
                wait += 1
                if wait >= patience:
                    break
    return _numpy(net), hist, ran, m
