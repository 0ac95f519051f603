"""GPU: Room.overlap_adapt -- the enrolled speakers' conditioned recordings mixed into labelled training and
validation clips, OD-NET fitted further on them (mmla_od_finetune) and installed -- recomputed by hand from
od_mix, od_features and overlap_detector.continue_train, and the room left as it was when asked to.  The
weights are synthetic: the scores carry no meaning here, only consistency is tested."""
import random
import warnings

import numpy as np
import pytest

import cond_ref
import enrol_inputs
from mmla_audio_amd import _lib, data_augmentation, models, noisereduce, overlap_detector, room, tfbundle, weights

pytestmark = pytest.mark.gpu

MIC = [0, 1, 0]
N = 8 * 16000
ARGS = dict(mic=MIC, n_overlapped=6, n_single=6, epochs=1, batch=4, patience=0, seed=3)


@pytest.fixture(scope='module')
def recordings():
    recs = [enrol_inputs.voiced(110.0, 80, N, [(30000, 50000)]),
            enrol_inputs.voiced(165.0, 81, N, [(64000, 90000)]),
            enrol_inputs.voiced(230.0, 82, N, [(5000, 12000), (100000, 115000)])]
    for r in recs:
        r.setflags(write=False)
    return recs


def _noises():
    return [cond_ref.noise(0), cond_ref.noise(1)]


def _room(base_dir, od_dir=None):
    c = _lib.Context(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # synthetic base weights
        od = (models.OverlapDetectionModel(weights.synthetic(weights.OD, seed=81), device=c) if od_dir is None
              else models.load_model(od_dir, device=c))
        si = models.load_model(base_dir, kind=weights.SI, allow_synthetic=True, device=c)
    return room.Room(od, si, _noises())


def _same(a, b):
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), name


def test_overlap_adapt_recomputed_by_hand_and_installed(tmp_path, recordings):
    base = str(tmp_path / 'timit' / 'model')
    save_to = str(tmp_path / 'adapted')
    r, twin = _room(base), None
    try:
        W0 = r.od.W
        got = r.overlap_adapt(recordings, save_to=save_to, **ARGS)
        # by hand
        noisereduce._set_noise_bank(r.ctx, _noises(), 16000)
        _, _, kept, pcm = r.ctx.si_enrol_embed(recordings, profile=MIC, passes=1, silence_remove=True,
                                               vad_mode=r.vad_mode, return_pcm=True)
        nw = kept.astype(np.int64) // 24000
        ntr = nw * 4 // 5
        print('windows', nw.tolist(), 'training', ntr.tolist())
        assert got.n_windows.tolist() == nw.tolist() and ntr.min() >= 1 and (nw - ntr).min() >= 1
        pool_tr = np.concatenate([pcm[k, :ntr[k] * 24000] for k in range(3)])
        pool_va = np.concatenate([pcm[k, ntr[k] * 24000:nw[k] * 24000] for k in range(3)])
        rng = random.Random(3)
        plan_tr, lab_tr, _ = data_augmentation.overlap_plan(ntr * 24000, range(3), 6, 6, rng)
        plan_va, lab_va, _ = data_augmentation.overlap_plan((nw - ntr) * 24000, range(3), 1, 1, rng)
        img = []
        for pool, plan in ((pool_tr, plan_tr), (pool_va, plan_va)):
            clips, lens = r.ctx.od_mix(pool, plan)
            img.append(r.ctx.od_features(clips, lens=lens, db=False, norm=False, zcr=False)['img'])
        plan = overlap_detector.fit_plan(lab_tr, 3, 1, val_ratio=0)
        plan['train'], plan['val'] = np.arange(12), 12 + np.arange(2)
        W1, hist, ran = overlap_detector.continue_train(W0, np.concatenate(img), np.concatenate([lab_tr, lab_va]),
                                                        plan, 1, 4, weighted=True, patience=0, device=r.ctx)
        assert ran == got.epochs_run == 1 and hist.tobytes() == got.history.tobytes() and hist.shape == (1, 5)
        assert np.isfinite(hist).all()
        for name in W1:
            assert r.od.W[name].tobytes() == W1[name].tobytes(), name
        assert any((W1[name] != W0[name]).any() for name in W1)
        for (m, rec, pre), W in ((got.before, W0), (got.after, W1)):
            r.ctx.load_weights(weights.OD, weights.pack(weights.OD, W), 2)
            want = data_augmentation.confusion(lab_va, r.ctx.od_forward(img[1]).argmax(axis=1))
            assert m.tolist() == want[0].tolist() and m.sum() == 2
        # the saved bundle is the installed model, bit for bit, and a fresh room on it ticks the same
        saved = tfbundle.load_bundle(save_to)
        for name in W1:
            assert saved[name].tobytes() == W1[name].tobytes(), name
        twin = _room(base, save_to)
        x = cond_ref.clips()
        mic = np.array([0, 1, 0, 1, 0, 1], np.int32)
        _same(r.tick(x, mic=mic), twin.tick(x, mic=mic))
        # set_weights then predict = load_model(save_to) on a fresh context
        assert r.od.predict(img[1]).tobytes() == twin.od.predict(img[1]).tobytes()
    finally:
        r.ctx.close()
        if twin is not None:
            twin.ctx.close()


def test_overlap_adapt_without_install_leaves_the_room_as_it_was(tmp_path, recordings):
    base = str(tmp_path / 'timit' / 'model')
    a, b = _room(base), _room(base)
    try:
        x = cond_ref.clips()
        mic = np.array([0, 1, 0, 1, 0, 1], np.int32)
        first = [rm.tick(x, mic=mic, return_pcm=True) for rm in (a, b)]
        out = a.overlap_adapt(recordings, install=False, **ARGS)
        assert out.epochs_run == 1
        # a speaker with one window has none for the validation pool: named, and nothing changes
        with pytest.raises(ValueError, match='speaker 1'):
            a.overlap_adapt([recordings[0], recordings[1][:9000], recordings[2]], **ARGS)
        second = [rm.tick(x[::-1].copy(), mic=mic, return_pcm=True) for rm in (a, b)]
        for got, want in (first, second):
            _same(got, want)
        for name in a.od.W:
            assert a.od.W[name].tobytes() == b.od.W[name].tobytes(), name
    finally:
        a.ctx.close()
        b.ctx.close()
