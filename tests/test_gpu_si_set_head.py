"""GPU: mmla_si_set_head -- the Dense head of the loaded SI model replaced in place.

After every installation si_forward must equal, bit for bit, a second context that loaded the full blob
carrying that head through mmla_load_weights, and si_embed must not move.  Synthetic model, 5 windows."""
import numpy as np
import pytest

from mmla_audio_amd import _lib, models, weights

pytestmark = pytest.mark.gpu

HEAD_NAME = 'layer_with_weights-42'
HEADS = [(8, _lib.HEAD_SIGMOID), (3, _lib.HEAD_SIGMOID), (33, _lib.HEAD_SOFTMAX)]


@pytest.fixture(scope='module')
def base_w():
    return weights.synthetic(weights.SI, seed=31, n_classes=630)


@pytest.fixture(scope='module')
def x():
    a = (np.random.default_rng(32).standard_normal((5, 256, 39)) * 10).astype(np.float32)
    a.setflags(write=False)
    return a


def _head(k):
    """a head of its own for every K: kernel [512, K], bias [K]"""
    W = weights.synthetic(weights.SI, seed=40 + k, n_classes=k)
    return W[HEAD_NAME + '/kernel'].astype(np.float32), W[HEAD_NAME + '/bias'].astype(np.float32)


def _with_head(base_w, w, b):
    W = {n: base_w[n] for n, _, _ in weights.si_spec(w.shape[1])[:-2]}
    W[HEAD_NAME + '/kernel'] = w
    W[HEAD_NAME + '/bias'] = b
    return W


@pytest.mark.parametrize('prec', [_lib.PREC_F16X3, _lib.PREC_F32], ids=['f16x3', 'f32'])
def test_set_head_equals_a_full_load(base_w, x, prec):
    a, ref = _lib.Context(0), _lib.Context(0)
    try:
        for c in (a, ref):
            c.set_precision(prec)
        a.load_weights(weights.SI, weights.pack(weights.SI, base_w, 630), 630, _lib.HEAD_SOFTMAX)
        emb = a.si_embed(x)
        for k, head in HEADS:
            w, b = _head(k)
            a.si_set_head(w, b, head)
            assert a.si_classes == k
            ref.load_weights(weights.SI, weights.pack(weights.SI, _with_head(base_w, w, b), k), k, head)
            got, want = a.si_forward(x), ref.si_forward(x)
            assert got.shape == (5, k) and got.tobytes() == want.tobytes(), (k, head)
            assert np.isfinite(got).all() and np.ptp(got) > 0
            assert a.si_embed(x).tobytes() == emb.tobytes(), 'the head moved the embedding'
            assert ref.si_embed(x).tobytes() == emb.tobytes()
    finally:
        a.close()
        ref.close()


def test_model_set_head_survives_a_reload(base_w, x):
    c, ref = _lib.Context(0), _lib.Context(0)
    try:
        m = models.SpeakerIdModel(base_w, 630, _lib.HEAD_SOFTMAX, device=c)
        w, b = _head(3)
        m.set_head(w, b)
        assert (m.n_classes, m.head, c.si_classes) == (3, _lib.HEAD_SIGMOID, 3)
        first = m.predict(x)
        ref.load_weights(weights.SI, weights.pack(weights.SI, _with_head(base_w, w, b), 3), 3, _lib.HEAD_SIGMOID)
        assert first.tobytes() == ref.si_forward(x).tobytes()
        other = models.SpeakerIdModel(weights.synthetic(weights.SI, seed=33, n_classes=8), 8,
                                      _lib.HEAD_SIGMOID, device=c)     # takes the context
        assert other.predict(x).shape == (5, 8)
        assert m.predict(x).tobytes() == first.tobytes(), 'the re-load did not bring the installed head back'
        assert c.si_classes == 3
    finally:
        c.close()
        ref.close()


def test_argument_checks(base_w):
    c = _lib.Context(0)
    try:
        w, b = _head(3)
        with pytest.raises(_lib.MmlaError) as e:          # no model loaded
            c.si_set_head(w, b, _lib.HEAD_SIGMOID)
        assert e.value.code == -3, e.value
        c.load_weights(weights.SI, weights.pack(weights.SI, base_w, 630), 630, _lib.HEAD_SOFTMAX)
        with pytest.raises(_lib.MmlaError) as e:          # K = 0
            c.si_set_head(np.zeros((512, 0), np.float32), np.zeros(0, np.float32), _lib.HEAD_SIGMOID)
        assert e.value.code == -1, e.value
        rc = c.lib.mmla_si_set_head(c.h, w.ctypes.data, b.ctypes.data, 0, _lib.HEAD_SIGMOID)
        assert rc == -1
        with pytest.raises(_lib.MmlaError) as e:          # an unknown head
            c.si_set_head(w, b, 2)
        assert e.value.code == -1, e.value
        assert c.lib.mmla_si_set_head(c.h, None, b.ctypes.data, 3, _lib.HEAD_SIGMOID) == -1
        assert c.lib.mmla_si_set_head(c.h, w.ctypes.data, None, 3, _lib.HEAD_SIGMOID) == -1
        assert c.si_classes == 630                       # and the model is the one loaded
        assert c.si_forward(np.zeros((1, 256, 39), np.float32)).shape == (1, 630)
    finally:
        c.close()
