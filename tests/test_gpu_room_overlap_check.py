"""GPU: Room.overlap_check -- the enrolled speakers' conditioned recordings mixed into labelled clips and
scored by OD-NET in one call -- recomputed by hand (the conditioned PCM of mmla_si_enrol_embed, the plan
of overlap_plan, the mix by tests/mix_ref.py on the host, mmla_od_pipeline), and the room left as it was.
The weights are synthetic: recall and precision carry no meaning here, only consistency is tested."""
import random
import warnings

import numpy as np
import pytest

import cond_ref
import enrol_inputs
import mix_ref
from mmla_audio_amd import _lib, data_augmentation, models, noisereduce, room, weights

pytestmark = pytest.mark.gpu

MIC = [0, 1, 0]
N = 8 * 16000


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


def _room(base_dir):
    c = _lib.Context(0)
    od = models.OverlapDetectionModel(weights.synthetic(weights.OD, seed=81), device=c)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # synthetic base weights
        si = models.load_model(base_dir, kind=weights.SI, allow_synthetic=True, device=c)
    return room.Room(od, si, _noises())


def test_overlap_check_recomputed_by_hand(tmp_path, recordings):
    r = _room(str(tmp_path / 'timit' / 'model'))
    try:
        got = r.overlap_check(recordings, mic=MIC, n_overlapped=24, n_single=16, seed=3)
        noisereduce._set_noise_bank(r.ctx, _noises(), 16000)
        _, _, kept, pcm = r.ctx.si_enrol_embed(recordings, profile=MIC, passes=1, silence_remove=True,
                                               vad_mode=r.vad_mode, return_pcm=True)
        nw = kept // 24000
        print('kept_len', kept.tolist(), 'windows', nw.tolist())
        assert nw.min() >= 2 and got.n_windows.tolist() == nw.tolist()
        pool = np.concatenate([pcm[k, :nw[k] * 24000] for k in range(3)])
        plan, labels, talkers = data_augmentation.overlap_plan(nw * 24000, range(3), 24, 16, random.Random(3))
        mixed, out_len = mix_ref.mix(pool, plan, 24000)
        assert (out_len == 24000).all() and not np.array_equal(mixed[0], pool[int(plan.src_off[0, 0]):][:24000])
        probs, argmax, silent = r.ctx.od_pipeline(mixed, out_len)
        assert not silent.any()
        assert got.probs.tobytes() == probs.tobytes() and got.argmax.tobytes() == argmax.tobytes()
        assert got.labels.tolist() == labels.tolist() == [1] * 24 + [0] * 16
        assert got.talkers.tolist() == talkers.tolist() and set(talkers[:24].tolist()) == {2, 3}
        matrix, recall, precision = data_augmentation.confusion(labels, argmax)
        assert got.confusion.tolist() == matrix.tolist() and got.confusion.sum() == 40
        assert got.confusion.sum(axis=1).tolist() == [16, 24]
        for a, b in ((got.recall, recall), (got.precision, precision)):
            assert a == b or (np.isnan(a) and np.isnan(b))
        # the same seed gives the same check, another seed another plan
        again = r.overlap_check(recordings, mic=MIC, n_overlapped=24, n_single=16, seed=3)
        assert again.probs.tobytes() == got.probs.tobytes()
        assert r.overlap_check(recordings, mic=MIC, n_overlapped=24, n_single=16, seed=4).probs.tobytes() != \
            got.probs.tobytes()
    finally:
        r.ctx.close()


def test_overlap_check_leaves_the_room_as_it_was(tmp_path, recordings):
    a, b = _room(str(tmp_path / 'timit' / 'model')), _room(str(tmp_path / 'timit' / 'model'))
    try:
        x = cond_ref.clips()
        mic = np.array([0, 1, 0, 1, 0, 1], np.int32)
        first = [rm.tick(x, mic=mic, return_pcm=True) for rm in (a, b)]
        a.overlap_check(recordings, mic=MIC, n_overlapped=8, n_single=8)
        # one speaker with a window is not enough; the check names the others and changes nothing
        with pytest.raises(ValueError, match=r'speakers \[1, 2\]'):
            a.overlap_check([recordings[0], recordings[1][:9000], recordings[2][:300]], mic=MIC)
        second = [rm.tick(x[::-1].copy(), mic=mic, return_pcm=True) for rm in (a, b)]
        for got, want in (first, second):
            for name in got._fields:
                assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
        assert (second[0].si_argmax >= 0).any()
        assert (a.si.n_classes, a.ctx.si_classes, a.ctx.od_classes) == (b.si.n_classes, b.ctx.si_classes, 2)
    finally:
        a.ctx.close()
        b.ctx.close()
