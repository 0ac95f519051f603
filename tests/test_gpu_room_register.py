"""GPU: Room.register -- recordings to a live SI head on the room's context -- against the file path the
library had before: the conditioned recordings written as WAV files, make_feature_experiment,
transfer_learning on a context of its own, load_model of the bundle it saved.  The head, the accuracy, the
saved bundle and the next tick must be equal bit for bit (SI-NET's result for a window does not depend on
its position in the batch, tests/test_gpu_batching.py, so the padded enrol batch changes nothing)."""
import json
import os
import warnings

import numpy as np
import pytest

import cond_ref
import enrol_inputs
from mmla_audio_amd import _lib, models, room, tfbundle, weights

pytestmark = pytest.mark.gpu

NAMES = ['reg_anna', 'reg_bo', 'reg_chen']
MIC = [0, 1, 0]
EPOCHS = 40
N = 8 * 16000
HEAD = 'layer_with_weights-42'


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


def _room(base_dir, si_dir=None):
    """a room on a context of its own around the synthetic base (or the bundle under si_dir)"""
    c = _lib.Context(0)
    od = models.OverlapDetectionModel(weights.synthetic(weights.OD, seed=81), device=c)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # synthetic base weights
        si = (models.load_model(base_dir, kind=weights.SI, allow_synthetic=True, device=c) if si_dir is None
              else models.load_model(si_dir, device=c))
    return room.Room(od, si, _noises())


def _file_path(tmp, monkeypatch, recordings, r, restarts):
    """the conditioned recordings through files, make_feature_experiment and transfer_learning on the
    process-wide default context -> (accuracy, the bundle's directory)"""
    import scipy.io.wavfile
    from mmla_audio_amd import noisereduce
    from mmla_audio_amd import speaker_identification as si
    noisereduce._set_noise_bank(r.ctx, _noises(), 16000)          # the room's bank, as its ticks build it
    _, nw, kept, pcm = r.ctx.si_enrol_embed(recordings, profile=MIC, passes=1, silence_remove=True,
                                            vad_mode=r.vad_mode, return_pcm=True)
    os.makedirs(tmp / 'corpus', exist_ok=True)
    files = []
    for k, name in enumerate(NAMES):
        files.append(str(tmp / 'corpus' / f'{name}.wav'))
        scipy.io.wavfile.write(files[-1], 16000, pcm[k, :kept[k]])
    monkeypatch.setattr(si.binarizer, '__defaults__', ({},))      # a label dict of its own
    x, y, ids = si.make_feature_experiment(files)
    assert ids == {str(k): n for k, n in enumerate(NAMES)}
    assert [int((y.argmax(axis=1) == k).sum()) for k in range(3)] == nw.tolist()
    final = str(tmp / f'file_model_{restarts}')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        acc = si.transfer_learning(x, y, 1, 0, str(tmp / 'timit' / 'model'), final, epochs=EPOCHS,
                                   restarts=restarts, allow_synthetic=True)
    return acc, final, kept, nw


@pytest.mark.parametrize('restarts', [1, 2])
def test_register_equals_the_file_path(tmp_path, monkeypatch, recordings, restarts):
    base_dir = str(tmp_path / 'timit' / 'model')
    r = _room(base_dir)
    twin = None
    try:
        assert (r.si.n_classes, r.si.head) == (630, _lib.HEAD_SOFTMAX)
        acc, final, kept, nw = _file_path(tmp_path, monkeypatch, recordings, r, restarts)
        save_to = str(tmp_path / 'room_model')
        reg = r.register(recordings, NAMES, mic=MIC, seed=1, epochs=EPOCHS, restarts=restarts, save_to=save_to)
        print('kept_len', reg.kept_len.tolist(), 'n_windows', reg.n_windows.tolist(), 'accuracy', reg.accuracy, acc)
        assert reg.speaker_id_dict == {'0': 'reg_anna', '1': 'reg_bo', '2': 'reg_chen'}
        assert reg.kept_len.tolist() == kept.tolist() and reg.n_windows.tolist() == nw.tolist()
        assert (reg.kept_len >= 4000).all() and (reg.kept_len <= N - 480).all() and reg.n_windows.min() >= 2
        assert reg.history.shape == (restarts, EPOCHS, 4)
        assert reg.accuracy == acc
        deployed = models.load_model(final)
        assert (deployed.n_classes, deployed.head) == (3, _lib.HEAD_SIGMOID)
        assert (r.si.n_classes, r.si.head, r.ctx.si_classes) == (3, _lib.HEAD_SIGMOID, 3)
        for t in ('/kernel', '/bias'):
            assert r.si.W[HEAD + t].tobytes() == deployed.W[HEAD + t].tobytes(), t
        # the bundle under save_to loads to the same tensors, and its dictionary is the registration's
        a, b = tfbundle.load_bundle(save_to), tfbundle.load_bundle(final)
        assert sorted(a) == sorted(b)
        for n in a:
            assert a[n].dtype == b[n].dtype and a[n].tobytes() == b[n].tobytes(), n
        assert json.load(open(os.path.join(save_to, 'speaker_id_dict.json'))) == reg.speaker_id_dict
        # the next tick answers with the new speakers, as a room built around the loaded bundle does
        twin = _room(base_dir, final)
        x = cond_ref.clips()
        mic = np.array([0, 1, 0, 1, 0, 1], np.int32)
        got, want = r.tick(x, mic=mic, return_pcm=True), twin.tick(x, mic=mic, return_pcm=True)
        assert got.si_probs.shape == (6, 3)
        for name in got._fields:
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
        assert (got.si_argmax >= 0).any() and got.silent.any()
    finally:
        r.ctx.close()
        if twin is not None:
            twin.ctx.close()


def test_an_empty_recording_raises_and_leaves_the_room(tmp_path, recordings):
    r = _room(str(tmp_path / 'timit' / 'model'))
    try:
        kernel = r.si.W[HEAD + '/kernel']
        x = (np.random.default_rng(90).standard_normal((2, 256, 39)) * 10).astype(np.float32)
        before = r.si.predict(x)
        recs = [recordings[0], np.zeros(N, np.int16), recordings[2]]
        with pytest.raises(ValueError, match='reg_bo'):
            r.register(recs, NAMES, mic=MIC, epochs=2, save_to=str(tmp_path / 'never'))
        assert not os.path.exists(tmp_path / 'never')
        assert (r.si.n_classes, r.si.head, r.ctx.si_classes) == (630, _lib.HEAD_SOFTMAX, 630)
        assert r.si.W[HEAD + '/kernel'] is kernel
        assert r.si.predict(x).tobytes() == before.tobytes()
    finally:
        r.ctx.close()
