"""GPU: speaker registration -- the embedding tap (mmla_si_embed), the persistent head trainer
(mmla_si_head_fit) against the float64 numpy restatement (tests/si_head_ref.py), and the drop-in
transfer_learning_on_experiment end to end.

The trainer's pass bound is measured inside each test: d32 = max-abs deviation of the restatement's
own float32 run from its float64 run on the same inputs, per quantity (W, b, loss, val_loss); the
kernel must lie within 16 x d32 of the float64 run (different summation order over 512 and over the
batch, hardware exp / log: each step adds error of the order of one f32 rounding)."""
import json
import os

import numpy as np
import pytest

import si_head_ref
from mmla_audio_amd import _lib, weights
from oracle import compare, nets, synth

pytestmark = pytest.mark.gpu

KMAX = _lib.SI_TRAIN_MAX_CLASSES
GAP = 1e-5      # no evaluated sample of the float64 run may have its top two sigmoids closer
FACTOR = 16.0


@pytest.fixture(scope='module')
def ctx():
    return _lib.Context(0)


@pytest.fixture(scope='module')
def base_w():
    return weights.synthetic(weights.SI, seed=2, n_classes=8)


def _load(ctx, W, k, head):
    ctx.load_weights(weights.SI, weights.pack(weights.SI, W, k), k, head)


@pytest.fixture(scope='module')
def emb64(ctx, base_w):
    """embeddings of 64 random windows, computed once and shared (read-only) by the trainer tests"""
    _load(ctx, base_w, 8, _lib.HEAD_SIGMOID)
    x = np.random.default_rng(21).standard_normal((64, 256, 39)) * 10
    e = ctx.si_embed(x.astype(np.float32))
    e.setflags(write=False)
    return e


def fit_inputs(emb, k, n_train, n_val, epochs, seed, restarts=1):
    """labels, Glorot initial heads and per-epoch orders of a trainer case, from `seed`"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, k, n_train + n_val).astype(np.int32)
    lim = np.sqrt(6.0 / (512 + k))
    w0 = rng.uniform(-lim, lim, (restarts, 512, k)).astype(np.float32)
    b0 = rng.uniform(-0.05, 0.05, (restarts, k)).astype(np.float32)
    perm = np.stack([[rng.permutation(n_train) for _ in range(epochs)] for _ in range(restarts)]).astype(np.int32)
    tr, va = slice(0, n_train), slice(n_train, n_train + n_val)
    return dict(emb=emb[tr], labels=lab[tr], val_emb=emb[va] if n_val else None,
                val_labels=lab[va] if n_val else None, w0=w0, b0=b0, perm=perm, epochs=epochs)


# ---- 1. si_embed ------------------------------------------------------------------------------------

@pytest.mark.parametrize('prec', [_lib.PREC_F16X3, _lib.PREC_F32])
def test_si_embed_vs_oracle(ctx, base_w, si_golden, prec):
    import torch
    x = np.stack([si_golden[f'feat_{i}'][0] for i in range(len(si_golden['names']))])
    x = np.concatenate([x, np.random.default_rng(5).standard_normal((9, 256, 39)) * 10]).astype(np.float32)
    Wi = dict(base_w)     # the oracle's Dense as a 512 x 512 identity: its logits are the BiLSTM output
    Wi['layer_with_weights-42/kernel'] = np.eye(512, dtype=np.float32)
    Wi['layer_with_weights-42/bias'] = np.zeros(512, np.float32)
    want = nets.si_forward(x, Wi, return_logits=True)
    ctx.set_precision(prec)
    try:
        _load(ctx, base_w, 8, _lib.HEAD_SIGMOID)
        got = ctx.si_embed(x)
        assert got.shape == (len(x), 512) and got.dtype == np.float32
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f'si_embed prec {prec}: max|got - want| / max|want| = {err:.3e}')
        assert err < 1e-5
        xt = torch.from_numpy(x).cuda()
        et = torch.zeros((len(x), 512), dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        ctx.si_embed_dev(xt.data_ptr(), len(x), et.data_ptr())
        ctx.synchronize()
        assert np.array_equal(et.cpu().numpy(), got), 'device-pointer call differs from the host call'
        W630 = weights.synthetic(weights.SI, seed=9, n_classes=630)     # another head, same base
        W630.update({n: base_w[n] for n, _, _ in weights.si_spec(8)[:-2]})
        _load(ctx, W630, 630, _lib.HEAD_SOFTMAX)
        assert np.array_equal(ctx.si_embed(x), got), 'the loaded head changed the embedding'
    finally:
        ctx.set_precision(_lib.PREC_F16X3)


# ---- 2. fit_head against the float64 restatement ----------------------------------------------------

CASES = [   # (K, n_train, n_val, epochs, seed) -- seeds chosen so that the float64 run has no near tie
    pytest.param(3, 37, 11, 30, 105, id='short-last-batch'),
    pytest.param(2, 9, 4, 30, 101, id='one-partial-batch'),
    pytest.param(KMAX, 48, 16, 3, 100, id='capacity'),
    pytest.param(3, 37, 0, 2, 101, id='no-validation'),
]


@pytest.mark.parametrize('k,n_train,n_val,epochs,seed', CASES)
def test_fit_head_vs_float64_reference(ctx, emb64, k, n_train, n_val, epochs, seed):
    from mmla_audio_amd import speaker_identification as si
    a = fit_inputs(emb64, k, n_train, n_val, epochs, seed)
    w, b, hist = si.fit_head(a['emb'], a['labels'], a['val_emb'], a['val_labels'], a['w0'], a['b0'],
                             a['perm'], epochs, device=ctx)
    assert w.shape == (1, 512, k) and b.shape == (1, k) and hist.shape == (1, epochs, 4)
    ref = {}
    for dt in (np.float64, np.float32):
        ref[dt] = si_head_ref.fit(a['emb'], a['labels'], a['val_emb'], a['val_labels'], a['w0'][0],
                                  a['b0'][0], a['perm'][0], epochs, dtype=dt)
    w64, b64, h64, gap = ref[np.float64]
    w32, b32, h32, _ = ref[np.float32]
    assert gap >= GAP, f'unlucky seed: top-two sigmoid gap {gap:.3e} in the float64 run'
    cols = [('W', w[0], w64, w32), ('b', b[0], b64, b32), ('loss', hist[0, :, 0], h64[:, 0], h32[:, 0])]
    if n_val:
        cols.append(('val_loss', hist[0, :, 2], h64[:, 2], h32[:, 2]))
    failures = []
    for name, got, r64, r32 in cols:
        d32 = float(np.abs(r32.astype(np.float64) - r64).max())
        dev = float(np.abs(got.astype(np.float64) - r64).max())
        print(f'K={k} n={n_train}/{n_val} epochs={epochs} {name}: d32 {d32:.3e}  kernel {dev:.3e}  '
              f'ratio {dev / d32 if d32 else float("inf"):.2f}')
        if not dev <= FACTOR * d32:
            failures.append((name, dev, d32))
    print(f'  most any weight moved: {np.abs(w64 - a["w0"][0]).max():.3e}; min top-two gap {gap:.3e}')
    assert not failures, failures
    assert np.array_equal(hist[0, :, 1], h64[:, 1].astype(np.float32)), 'per-epoch accuracy'
    if n_val:
        assert np.array_equal(hist[0, :, 3], h64[:, 3].astype(np.float32)), 'per-epoch val accuracy'
    else:
        assert np.isnan(hist[0, :, 2:]).all() and not np.isnan(hist[0, :, :2]).any()


# ---- 3. one registered speaker ----------------------------------------------------------------------

def test_fit_head_single_class_is_a_fixed_point(ctx, emb64):
    a = fit_inputs(emb64, 1, 21, 6, 4, seed=3)
    w, b, hist = ctx.si_head_fit(a['emb'], a['labels'], a['val_emb'], a['val_labels'], a['w0'], a['b0'],
                                 a['perm'], 4)
    assert w.tobytes() == a['w0'].tobytes() and b.tobytes() == a['b0'].tobytes()
    want = -np.log(np.float32(1) - np.float32(1e-7))
    assert want.dtype == np.float32
    assert (hist[0, :, [0, 2]] == want).all(), hist[0]
    assert (hist[0, :, [1, 3]] == 1).all()


# ---- 4. determinism, restart independence -----------------------------------------------------------

def test_fit_head_is_deterministic_and_restarts_are_independent(ctx, emb64):
    a = fit_inputs(emb64, 5, 37, 11, 6, seed=4, restarts=3)
    args = (a['emb'], a['labels'], a['val_emb'], a['val_labels'])
    one = ctx.si_head_fit(*args, a['w0'], a['b0'], a['perm'], 6)
    two = ctx.si_head_fit(*args, a['w0'], a['b0'], a['perm'], 6)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(one[0][0], one[0][1])
    for r in range(3):
        solo = ctx.si_head_fit(*args, a['w0'][r:r + 1], a['b0'][r:r + 1], a['perm'][r:r + 1], 6)
        for x, y in zip(one, solo):
            assert x[r].tobytes() == y[0].tobytes(), f'restart {r} depends on n_restarts'


def test_fit_head_device_pointers_match_host_call(ctx, emb64):
    import torch
    k, nt, nv, ep, R = 5, 37, 11, 6, 2
    a = fit_inputs(emb64, k, nt, nv, ep, seed=4, restarts=R)
    host = ctx.si_head_fit(a['emb'], a['labels'], a['val_emb'], a['val_labels'], a['w0'], a['b0'],
                           a['perm'], ep)
    dev = {n: torch.from_numpy(np.array(a[n])).cuda()
           for n in ('emb', 'labels', 'val_emb', 'val_labels', 'w0', 'b0', 'perm')}
    w = torch.zeros((R, 512, k), dtype=torch.float32, device='cuda')
    b = torch.zeros((R, k), dtype=torch.float32, device='cuda')
    h = torch.zeros((R, ep, 4), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.si_head_fit_dev(dev['emb'].data_ptr(), dev['labels'].data_ptr(), nt, dev['val_emb'].data_ptr(),
                        dev['val_labels'].data_ptr(), nv, k, R, ep, 16, 1e-4, dev['w0'].data_ptr(),
                        dev['b0'].data_ptr(), dev['perm'].data_ptr(), w.data_ptr(), b.data_ptr(),
                        h.data_ptr())
    ctx.synchronize()
    for got, want in zip((w, b, h), host):
        assert got.cpu().numpy().tobytes() == want.tobytes()


# ---- 5. one launch ----------------------------------------------------------------------------------

def test_fit_head_is_one_launch(ctx, emb64):
    ctx.profile_enable(True)
    try:
        for epochs in (2, 40):
            a = fit_inputs(emb64, 3, 37, 11, epochs, seed=5)
            ctx.profile_read(reset=True)
            ctx.si_head_fit(a['emb'], a['labels'], a['val_emb'], a['val_labels'], a['w0'], a['b0'],
                            a['perm'], epochs)
            prof = ctx.profile_read(reset=True)
            assert prof['head'][1] == 1, prof
            assert sum(v[1] for v in prof.values()) == 1, prof
    finally:
        ctx.profile_enable(False)


# ---- 6. argument checks -----------------------------------------------------------------------------

def _bad_classes(a, k):
    a['w0'] = np.zeros((1, 512, k), np.float32)
    a['b0'] = np.zeros((1, k), np.float32)


def _bad_label(a):
    a['labels'] = a['labels'].copy()
    a['labels'][5] = 3


def _bad_perm(a):
    a['perm'] = a['perm'].copy()
    a['perm'][0, 1, 7] = a['perm'][0, 1, 8]


@pytest.mark.parametrize('spoil', [lambda a: _bad_classes(a, 0), lambda a: _bad_classes(a, KMAX + 1),
                                   _bad_label, _bad_perm],
                         ids=['K=0', 'K=MAX+1', 'label=K', 'perm-repeats'])
def test_fit_head_argument_checks(ctx, emb64, spoil):
    a = fit_inputs(emb64, 3, 37, 11, 2, seed=6)
    spoil(a)
    ctx.profile_enable(True)
    try:
        ctx.profile_read(reset=True)
        with pytest.raises(_lib.MmlaError) as ei:
            ctx.si_head_fit(a['emb'], a['labels'], a['val_emb'], a['val_labels'], a['w0'], a['b0'],
                            a['perm'], 2)
        assert ei.value.code == -1 and 'MMLA_E_INVALID: ' in str(ei.value)
        assert len(str(ei.value).split('MMLA_E_INVALID: ')[1]) > 5, 'no message'
        assert sum(v[1] for v in ctx.profile_read(reset=True).values()) == 0, 'something was launched'
    finally:
        ctx.profile_enable(False)


# ---- 7. end to end ----------------------------------------------------------------------------------

def _voiced_wav(path, f0, seed, seconds=8.0):
    import scipy.io.wavfile
    rng = np.random.default_rng(seed)
    n = int(seconds * synth.SR)
    t = np.arange(n) / synth.SR
    k = np.arange(1, 21)[:, None]
    x = np.sum(np.sin(2 * np.pi * k * f0 * t[None] + rng.uniform(0, 2 * np.pi, (20, 1))) / k, axis=0)
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.01 * rng.standard_normal(n)
    x = 0.5 * x / np.abs(x).max()
    scipy.io.wavfile.write(path, synth.SR, np.round(x * 32767).astype(np.int16))


def test_transfer_learning_on_experiment_end_to_end(tmp_path):
    import warnings
    from mmla_audio_amd import speaker_identification as si
    from mmla_audio_amd import load_model, tfbundle
    os.makedirs(tmp_path / 'experiment' / 'corpus')
    names = ['reg_anna', 'reg_bo', 'reg_chen']
    for i, (name, f0) in enumerate(zip(names, (110.0, 165.0, 230.0))):
        _voiced_wav(str(tmp_path / 'experiment' / 'corpus' / f'{name}.wav'), f0, 40 + i)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # synthetic base weights
        acc = si.transfer_learning_on_experiment(str(tmp_path), allow_synthetic=True, epochs=40)
        base = load_model(str(tmp_path / 'timit' / 'model'), kind=weights.SI, allow_synthetic=True)
    ids = json.load(open(tmp_path / 'experiment' / 'speaker_id_dict.json'))
    assert sorted(ids.values()) == names and len(ids) == 3
    feats = np.load(tmp_path / 'experiment' / 'experiment_feature.npz')
    x, y = feats['arr_0'], feats['arr_1']
    model = load_model(str(tmp_path / 'experiment' / 'model'))
    assert model.n_classes == 3 and model.head == _lib.HEAD_SIGMOID and not model.synthetic
    saved = tfbundle.load_bundle(str(tmp_path / 'experiment' / 'model'))
    for n, _, _ in weights.si_spec(3)[:-2]:
        assert saved[n].tobytes() == base.W[n].tobytes(), f'{n}: the frozen base changed'
    wk, wb = saved['layer_with_weights-42/kernel'], saved['layer_with_weights-42/bias']
    emb = model.ctx.si_embed(x)
    want = 1.0 / (1.0 + np.exp(-(emb.astype(np.float64) @ wk.astype(np.float64) + wb)))
    err = compare.logp_err(model.predict(x), want)
    assert err <= compare.LOGP_TOL, err
    # the same plan through the float64 restatement reaches the accuracy returned
    labels = y.argmax(axis=1)
    plan = si._fit_plan(labels, 3, 1, 0, 40, 1)
    tr, va = plan['train'], plan['val']
    assert len(va) >= 3
    w64, b64, h64, gap = si_head_ref.fit(emb[tr], labels[tr], emb[va], labels[va], plan['w0'][0],
                                         plan['b0'][0], plan['perm'][0], 40)
    assert gap >= GAP, f'near tie in the float64 run: {gap:.3e}'
    assert acc == np.float32(h64[-1, 3]), (acc, h64[-1, 3])
