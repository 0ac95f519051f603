"""CPU: the arithmetic of the batched sequence front-end's windows, the enrolment tests' inputs under the
CPU oracles (so that no GPU run is spent on inputs that exercise nothing), and Room.register's argument
validation, which must come before the context is touched."""
import numpy as np
import pytest

import enrol_inputs
from mmla_audio_amd import _lib, room


def test_frame_and_window_counts():
    T, W = _lib.si_seq_frames, _lib.si_seq_windows
    assert [T(n) for n in (1, 400, 401, 560, 561, 41200, 41201, 82160, 82161)] == [1, 1, 2, 2, 3, 256, 257, 512, 513]
    assert [W(n) for n in (0, 1, 400, 401, 561, 41200, 41201, 82160, 82161)] == [0, 1, 1, 1, 1, 1, 2, 2, 3]
    assert W(82161) == 3 and W(48000) == 2 and W(30000) == 1 and W(610000) == 15
    # the longest recording: 4096 detector frames of 480 samples, 48 windows
    assert _lib.ENROL_MAX_SAMPLES == 4096 * 480 and T(_lib.ENROL_MAX_SAMPLES) == 12287
    assert W(_lib.ENROL_MAX_SAMPLES) == 48
    # the tests' own helper agrees with the library's
    for n in (0, 1, 400, 401, 41200, 41201, 610000):
        assert enrol_inputs.windows(n) == W(n)
        if n:
            assert enrol_inputs.frames(n) == T(n)
    # T(n) is the number of 400-sample frames at step 160 that cover n samples
    for n in (401, 560, 561, 720, 721, 48000):
        assert 400 + 160 * (T(n) - 1) >= n > 400 + 160 * (T(n) - 2)


def test_the_enrol_inputs_lose_and_keep_audio():
    x = enrol_inputs.recordings()
    kept = np.array(enrol_inputs.oracle_kept(x, enrol_inputs.LENS, enrol_inputs.PROFILE, enrol_inputs.noises()))
    lost = enrol_inputs.LENS - kept
    assert (lost >= 480).any() and (kept >= 4000).any() and kept[2] == 0, kept
    assert (kept % 480 == 0).all()


class _StubContext:
    """a context that must not be reached: every attribute access fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f'Room.register touched the context ({name}) before validating its arguments')


class _StubModel:
    def __init__(self, ctx):
        self.ctx = ctx

    def _ensure_loaded(self):
        raise AssertionError('Room.register loaded the model before validating its arguments')


def _stub_room(noises):
    c = _StubContext()
    return room.Room(_StubModel(c), _StubModel(c), noises)


def test_register_validates_before_it_touches_the_context():
    noises = [np.zeros(16000, np.float32), np.ones(16000, np.float32)]
    rec = [np.zeros(16000, np.int16)] * 3
    r = _stub_room(noises)
    with pytest.raises(ValueError, match='unique'):
        r.register(rec, ['ann', 'bo', 'ann'])
    with pytest.raises(ValueError, match='one recording per speaker'):
        r.register(rec, ['ann', 'bo'])
    with pytest.raises(ValueError, match='one recording per speaker'):
        r.register([], [])
    with pytest.raises(ValueError, match='noise clips'):
        r.register(rec, ['ann', 'bo', 'cy'], mic=[0, 2, 1])
    with pytest.raises(ValueError, match='noise clips'):
        r.register(rec, ['ann', 'bo', 'cy'], mic=[0, -1, 1])
    with pytest.raises(ValueError, match='one entry per speaker'):
        r.register(rec, ['ann', 'bo', 'cy'], mic=[0, 1])
    with pytest.raises(ValueError, match='epochs'):
        r.register(rec, ['ann', 'bo', 'cy'], epochs=0)
    with pytest.raises(ValueError, match='at most'):
        r.register([rec[0]] * 33, [f's{i}' for i in range(33)])
    with pytest.raises(ValueError, match='exceeds'):
        r.register([np.zeros(_lib.ENROL_MAX_SAMPLES + 1, np.int16)], ['ann'])
    # a room without noise clips checks the shape of mic only
    with pytest.raises(ValueError, match='one entry per speaker'):
        _stub_room(None).register(rec, ['ann', 'bo', 'cy'], mic=[0])
