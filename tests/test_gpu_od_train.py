"""GPU: training OD-NET from scratch -- mmla_od_train, mmla_od_drop_mask, mmla_od_auc (od_bwd.hip, od_finetune.cpp)
and overlap_detector.train_model.

No new tolerance for the fit: mmla_od_train must equal, bit for bit, mmla_od_finetune fed the keep-bits that
mmla_od_drop_mask writes, so every bound of tests/test_gpu_od_finetune.py carries over.  The AUC values are held
to 1.2e-7 of the restatement (tests/od_train_ref.py): both sides round one double to float32, and that is
1 ulp at 1.  An AUC comparison is made only where the CPU shows that the probabilities decide every count:
none within 1e-5 of a threshold inside (0, 1) -- float32 and float64 forwards differ by far less -- and all
inside [0, 1], which decides the two outer thresholds float32(-1e-7) and float32(1 + 1e-7) whatever the rounding.
"""
import hashlib

import numpy as np
import pytest
import torch

import od_finetune_ref as ref
import od_train_ref as tr
import si_base_ref
from mmla_audio_amd import _lib, metrics, models, overlap_detector, weights

pytestmark = pytest.mark.gpu

AUC_TOL = 1.2e-7
MARGIN = 1e-5
H, W_, N, NV, BATCH, EPOCHS = 16, 17, 11, 5, 4, 3
CLASS_W = (0.3, 0.7)
SEED = 0x5EED0D0D17


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _case():
    rng = np.random.default_rng([21, 93])
    img = rng.integers(0, 256, (N + NV, H, W_, 3)).astype(np.uint8)
    labels = rng.integers(0, 2, N + NV).astype(np.int32)
    labels[:2] = (0, 1)
    labels[N:N + 2] = (0, 1)
    perm = np.stack([rng.permutation(N) for _ in range(EPOCHS)]).astype(np.int32)
    W0 = weights.initial_od(1)
    return dict(W=W0, blob=weights.pack(weights.OD, W0), img=img[:N], labels=labels[:N], val_img=img[N:],
                val_labels=labels[N:], perm=perm, lr=overlap_detector.cosine_lr(EPOCHS).astype(np.float32))


@pytest.fixture(scope='module')
def case():
    return _case()


def _train(ctx, c, epochs=EPOCHS, batch=BATCH, val=True, ckpt=1, patience=0):
    return ctx.od_train(c['blob'], c['img'], c['labels'], c['val_img'] if val else None,
                        c['val_labels'] if val else None, CLASS_W, c['lr'][:epochs], c['perm'][:epochs], epochs,
                        batch, SEED, patience, ckpt)


def _masks(ctx, epochs):
    return np.stack([ctx.od_drop_mask(SEED, ep, None, N) for ep in range(epochs)])


def _finetune(ctx, c, epochs, batch=BATCH):
    return ctx.od_finetune(c['blob'], c['img'], c['labels'], c['val_img'], c['val_labels'], CLASS_W,
                           c['lr'][:epochs], c['perm'][:epochs], _masks(ctx, epochs), epochs, batch, 0)


@pytest.fixture(scope='module')
def trained(ctx, case):
    r = _train(ctx, case)
    for a in r[:3]:
        if a is not None:
            a.setflags(write=False)
    return r


def _decided(probs):
    p = np.asarray(probs, np.float64).ravel()
    inner = tr.thresholds().astype(np.float64)[1:-1]
    return bool(((p >= 0) & (p <= 1)).all()) and float(np.abs(p[:, None] - inner[None]).min()) > MARGIN


# ---- 1. keep-bits ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 5])
def test_drop_mask_equals_the_philox_restatement(ctx, n):
    ids = np.array([7, 0, 123456, 3, 3], np.int32)[:n]
    for epoch in (0, 3):
        assert ctx.od_drop_mask(SEED, epoch, None, n).tobytes() == tr.drop_mask(SEED, epoch, np.arange(n)).tobytes()
        got = ctx.od_drop_mask(SEED, epoch, ids)
        assert got.shape == (n, 512) and got.tobytes() == tr.drop_mask(SEED, epoch, ids).tobytes()
    assert (ctx.od_drop_mask(SEED, 0, None, n) != ctx.od_drop_mask(SEED, 3, None, n)).any()
    d_ids = torch.from_numpy(ids).cuda()
    out = torch.zeros((n, 512), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.od_drop_mask_dev(SEED, 3, d_ids.data_ptr(), n, out.data_ptr())
    ctx.synchronize()
    assert out.cpu().numpy().tobytes() == tr.drop_mask(SEED, 3, ids).tobytes()


def test_drop_mask_keep_rate_and_the_si_bits_are_unchanged(ctx):
    m = ctx.od_drop_mask(SEED, 1, None, 64)
    assert abs(m.mean() - 0.75) <= 4 * np.sqrt(0.75 * 0.25 / m.size)
    # the SI sites' bits for one fixed seed, as the generator gave them before it moved into philox.h (the
    # values of the restatement tests/si_base_ref.py, which tests/test_gpu_si_base.py holds the kernel to)
    a, b = ctx.si_base_drop_mask(0x1234567089ABCDEF, 2, [0, 7])
    assert np.packbits(a[0].ravel()[:64]).tobytes().hex() == '7d8fadeffebf9fbd'
    assert np.packbits(b[1][:64]).tobytes().hex() == 'ffff5f9edea7acbf'
    assert hashlib.sha256(a.tobytes()).hexdigest() == \
        '0296a153181e6c868f295881261c44874d0f5114c96107d1ebad5e48fb094549'
    assert hashlib.sha256(b.tobytes()).hexdigest() == \
        'f24386ebbc978a32f37063f9e62f82959d9f3e062436a64545b9b09f1e718d1e'
    # site 2 is a stream of its own
    assert np.packbits(ctx.od_drop_mask(0x1234567089ABCDEF, 2, [0, 7])[1][:64]).tobytes().hex() == '1f7bf7ffff678fe5'
    ra, rb = si_base_ref.drop_masks(0x1234567089ABCDEF, 2, [0, 7])
    assert a.tobytes() == ra.tobytes() and b.tobytes() == rb.tobytes()
    with pytest.raises(_lib.MmlaError, match='sample_ids'):
        ctx.od_drop_mask(SEED, 0, [0, -1])
    with pytest.raises(_lib.MmlaError, match='epoch'):
        ctx.od_drop_mask(SEED, -1, None, 2)
    with pytest.raises(_lib.MmlaError, match='n 0'):
        ctx.od_drop_mask(SEED, 0, None, 0)


# ---- 2. AUC ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 64, 65, 1000])
def test_auc_equals_the_restatement(ctx, n):
    rng = np.random.default_rng([31, n])
    p1 = rng.random(n).astype(np.float32)
    probs = np.stack([np.float32(1) - p1, p1], axis=1)
    labels = (rng.random(n) < p1).astype(np.int32)           # informative predictions
    for lab in (labels, np.zeros(n, np.int32), np.ones(n, np.int32)):     # ... and one class alone
        got, want = ctx.od_auc(probs, lab), tr.auc(probs, lab)
        print(n, float(got), float(want))
        assert got.dtype == np.float32 and abs(float(got) - float(want)) <= AUC_TOL
    on, nudged = tr.on_threshold_case()
    pad = np.repeat(np.array([[0.9, 0.1]], np.float32), n - 1, axis=0)    # class-0 samples, well decided
    for first, known in ((on, 0.5), (nudged, 1.0)):
        p, lab = np.vstack([first, pad]), np.zeros(n, np.int32)
        got, want = ctx.od_auc(p, lab), tr.auc(p, lab)
        assert abs(float(got) - float(want)) <= AUC_TOL
        if n == 1:
            assert float(got) == known
    d_p = torch.from_numpy(probs).cuda()
    d_l = torch.from_numpy(labels).cuda()
    out = torch.zeros(1, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ctx.od_auc_dev(d_p.data_ptr(), d_l.data_ptr(), n, out.data_ptr())
    ctx.synchronize()
    assert out.cpu().numpy()[0] == ctx.od_auc(probs, labels)


def test_auc_wrapper_and_arguments(ctx):
    probs = np.array([[0.9, 0.1], [0.2, 0.8], [0.6, 0.4]], np.float32)
    labels = np.array([0, 1, 1])
    assert metrics.auc(probs, labels) == float(tr.auc(probs, labels))
    assert metrics.auc(probs, np.eye(2)[labels]) == float(tr.auc(probs, labels))
    with pytest.raises(_lib.MmlaError, match='labels'):
        ctx.od_auc(probs, [0, 1, 2])
    with pytest.raises(ValueError):
        ctx.od_auc(probs, [0, 1])
    out = np.empty(1, np.float32)
    lab = labels.astype(np.int32)
    assert ctx.lib.mmla_od_auc(ctx.h, probs.ctypes.data, lab.ctypes.data, 0, out.ctypes.data, 0) == -1
    assert ctx.lib.mmla_od_auc(ctx.h, None, lab.ctypes.data, 3, out.ctypes.data, 0) == -1
    assert ctx.lib.mmla_od_auc(ctx.h, probs.ctypes.data, lab.ctypes.data, 3, None, 0) == -1


# ---- 3. the fit -----------------------------------------------------------------------------------------

def test_train_equals_finetune_on_the_masks_of_the_seed(ctx, case, trained):
    out, best, hist, ran, best_ep = trained
    out2, hist2, ran2 = _finetune(ctx, case, EPOCHS)
    print('history', hist.tolist())
    assert ran == ran2 == EPOCHS and hist.shape == (EPOCHS, 7) and np.isfinite(hist).all()
    assert out.tobytes() == out2.tobytes()
    assert hist[:, :5].tobytes() == np.ascontiguousarray(hist2).tobytes()
    assert (out != case['blob']).any()
    assert ((hist[:, 5:] >= 0) & (hist[:, 5:] <= 1)).all()


def test_val_auc_column(ctx, case, trained):
    hist = trained[2]
    for e in range(EPOCHS):
        blob = _finetune(ctx, case, e + 1)[0]
        probs = ref.forward(weights.unpack(weights.OD, blob), case['val_img'])      # inference mode, float64
        assert _decided(probs), f'epoch {e}: a validation prob is too close to a threshold; change the seed'
        want = tr.auc(probs.astype(np.float32), case['val_labels'])
        print('val_auc', e, float(hist[e, 6]), float(want))
        assert abs(float(hist[e, 6]) - float(want)) <= AUC_TOL


def test_training_auc_column_of_a_one_batch_epoch(ctx, case):
    out, _, hist, _, _ = _train(ctx, case, epochs=1, batch=16)
    order = case['perm'][0]
    mask = ctx.od_drop_mask(SEED, 0, order)                       # by row of the training set
    assert mask.tobytes() == _masks(ctx, 1)[0][order].tobytes()
    with torch.no_grad():
        z = ref._Net(case['W'], torch.float64).logits(case['img'][order], mask, True)
        probs = torch.softmax(z, 1).numpy()
    assert _decided(probs), 'a training prob is too close to a threshold; change the seed'
    want = tr.auc(probs.astype(np.float32), case['labels'][order])
    print('auc', float(hist[0, 5]), float(want))
    assert abs(float(hist[0, 5]) - float(want)) <= AUC_TOL


# ---- 4. callbacks ---------------------------------------------------------------------------------------

def _raw_train(ctx, c, **over):
    a = dict(blob=c['blob'], img=np.ascontiguousarray(c['img']), labels=c['labels'],
             vi=np.ascontiguousarray(c['val_img']), vl=c['val_labels'], nv=NV, epochs=EPOCHS, ckpt=1,
             cw=np.array(CLASS_W, np.float32), lr=c['lr'], perm=c['perm'])
    a.update(over)
    out = np.empty_like(c['blob'])
    best = np.full_like(c['blob'], 12345.0)
    hist = np.empty((max(a['epochs'], 1), 7), np.float32)
    ran, best_ep = np.zeros(1, np.int32), np.full(1, 99, np.int32)
    p = lambda x: None if x is None else x.ctypes.data                       # noqa: E731
    rc = ctx.lib.mmla_od_train(ctx.h, p(a['blob']), a['blob'].size, p(a['img']), p(a['labels']), N, p(a['vi']),
                               p(a['vl']), a['nv'], H, W_, p(a['cw']), a['epochs'], BATCH, p(a['lr']), p(a['perm']),
                               _lib._seed64(SEED), 0, a['ckpt'], p(out), p(best), p(hist), p(ran), p(best_ep), 0)
    return rc, out, best, hist, int(ran[0]), int(best_ep[0])


def test_checkpoint_is_the_first_best_epoch(ctx, case, trained):
    out, best, hist, ran, best_ep = trained
    assert best_ep == int(np.argmax(hist[:, 3])) and best is not None
    shorter = _train(ctx, case, epochs=best_ep + 1)[0]
    assert best.tobytes() == shorter.tobytes()
    for over in (dict(ckpt=0), dict(nv=0, vi=None, vl=None)):
        rc, out2, best2, hist2, ran2, ep2 = _raw_train(ctx, case, **over)
        assert rc == 0 and ran2 == EPOCHS and ep2 == -1
        assert (best2 == 12345.0).all(), 'best_out was written without a checkpoint'
        if 'nv' in over:
            assert np.isnan(hist2[:, [2, 3, 6]]).all() and np.isfinite(hist2[:, [0, 1, 4, 5]]).all()
        else:
            assert out2.tobytes() == out.tobytes() and hist2.tobytes() == hist.tobytes()
    assert _raw_train(ctx, case, ckpt=-1)[0] == -1
    assert 'ckpt_period' in ctx.lib.mmla_last_error(ctx.h).decode()


def test_zero_epochs_is_the_identity_and_fits_repeat_bit_for_bit(ctx, case, trained):
    same, best, h0, ran0, ep0 = _train(ctx, case, epochs=0)
    assert same.tobytes() == case['blob'].tobytes() and best is None and h0.shape == (0, 7) and (ran0, ep0) == (0, -1)
    again = _train(ctx, case)
    assert again[0].tobytes() == trained[0].tobytes() and again[1].tobytes() == trained[1].tobytes()
    assert again[2].tobytes() == trained[2].tobytes() and again[3:] == trained[3:]


def test_device_pointers_match_the_host_call(ctx, case, trained):
    c = case
    dev = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda()
           for k in ('blob', 'img', 'labels', 'val_img', 'val_labels', 'perm')}
    n_floats = c['blob'].size
    out = torch.zeros(n_floats, dtype=torch.float32, device='cuda')
    best = torch.zeros(n_floats, dtype=torch.float32, device='cuda')
    hist = torch.zeros((EPOCHS, 7), dtype=torch.float32, device='cuda')
    ran = torch.zeros(1, dtype=torch.int32, device='cuda')
    best_ep = torch.zeros(1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.od_train_dev(dev['blob'].data_ptr(), n_floats, dev['img'].data_ptr(), dev['labels'].data_ptr(), N,
                     dev['val_img'].data_ptr(), dev['val_labels'].data_ptr(), NV, H, W_, CLASS_W, EPOCHS, BATCH,
                     c['lr'], dev['perm'].data_ptr(), SEED, 0, 1, out.data_ptr(), best.data_ptr(), hist.data_ptr(),
                     ran.data_ptr(), best_ep.data_ptr())
    ctx.synchronize()
    assert out.cpu().numpy().tobytes() == trained[0].tobytes()
    assert best.cpu().numpy().tobytes() == trained[1].tobytes()
    assert hist.cpu().numpy().tobytes() == trained[2].tobytes()
    assert (int(ran.cpu()[0]), int(best_ep.cpu()[0])) == trained[3:]
    assert dev['blob'].cpu().numpy().tobytes() == c['blob'].tobytes(), 'the input blob was written'


# ---- 5. Python ------------------------------------------------------------------------------------------

def test_train_model_augments_weights_saves_and_predicts(ctx, tmp_path, monkeypatch):
    rng = np.random.default_rng([41, 94])
    labels = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.int32)            # 9 : 3
    img = rng.integers(0, 256, (12, 16, 17, 3)).astype(np.uint8)
    val_img = rng.integers(0, 256, (4, 16, 17, 3)).astype(np.uint8)
    val_y = np.eye(2)[[0, 1, 1, 0]]                                              # one-hot, as labels_loader
    seen = {}
    real = _lib.Context.od_train

    def spy(self, packed, x, y, *a, **k):
        seen.update(x=np.array(x), y=np.array(y), cw=np.array(a[2]), packed=np.array(packed))
        return real(self, packed, x, y, *a, **k)

    monkeypatch.setattr(_lib.Context, 'od_train', spy)
    save, ckpt = str(tmp_path / 'model'), str(tmp_path / 'ckpt')
    model, history = overlap_detector.train_model(img, labels, val_img, val_y, epochs=2, batch_size=8, weighted=True,
                                                  augmented=True, seed=5, patience=10, checkpoint_path=ckpt,
                                                  save_path=save, device=ctx)
    src, levels, new = overlap_detector.augment_plan(labels, 2)
    assert len(seen['y']) == 9 + 3 + 6 and sorted(levels[new == 1].tolist()) == [0] * 3 + [1] * 3 + [2] * 3
    assert (seen['y'] == new).all() and seen['x'].tobytes() == ctx.od_augment(img, src, levels).tobytes()
    assert seen['cw'].tolist() == overlap_detector.cal_weighted_penalty(np.eye(2)[new]).tolist() == [0.5, 0.5]
    assert seen['packed'].tobytes() == weights.pack(weights.OD, weights.initial_od(5)).tobytes()
    assert isinstance(model, models.OverlapDetectionModel)
    assert list(history.history) == list(overlap_detector.HISTORY_KEYS) and history.epochs_run == 2
    assert all(len(v) == 2 and np.isfinite(v).all() for v in history.history.values())
    assert history.history['lr'] == [float(v) for v in overlap_detector.cosine_lr(2).astype(np.float32)]
    back = models.load_model(save, device=ctx)
    assert weights.pack(weights.OD, back.W).tobytes() == weights.pack(weights.OD, model.W).tobytes()
    assert history.best_epoch is not None
    best = models.load_model(ckpt, kind=weights.OD, device=ctx)
    assert set(best.W) == set(model.W)
    probs = back.predict(rng.integers(0, 256, (2, 128, 151, 3)).astype(np.uint8))
    assert probs.shape == (2, 2) and np.isfinite(probs).all() and np.allclose(probs.sum(axis=1), 1, atol=1e-5)


def test_train_model_full_size_step(ctx):
    rng = np.random.default_rng([42, 95])
    img = rng.integers(0, 256, (2, 128, 151, 3)).astype(np.uint8)
    model, history = overlap_detector.train_model(img, np.array([0, 1]), None, None, epochs=1, batch_size=2,
                                                  device=ctx)
    assert history.epochs_run == 1 and history.best_epoch is None
    for k in ('loss', 'categorical_accuracy', 'lr', 'auc'):
        assert np.isfinite(history.history[k]).all(), k
    assert np.isnan(history.history['val_auc'][0]) and np.isnan(history.history['val_loss'][0])
    assert np.isfinite(weights.pack(weights.OD, model.W)).all()
