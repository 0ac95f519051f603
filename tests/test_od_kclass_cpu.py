"""CPU: the K-class OD layers that need no device -- the weight layouts, the bundle, the label and evaluation
helpers, the K-class AUC restatement -- and the conditions the bounds of tests/test_gpu_od_kclass.py rest on
(tests/od_kclass_cases.py)."""
import numpy as np
import pytest

import od_finetune_cases as C
import od_kclass_cases as KC
import od_train_ref as tr
from mmla_audio_amd import _lib, overlap_detector, weights
from mmla_audio_amd import overlap_detection_post_processing as odpp
from oracle import compare, nets

HEAD = KC.HEAD


# ---- weights ----------------------------------------------------------------------------------------------

def test_two_class_defaults_are_unchanged():
    assert weights.od_spec() == weights.od_spec(2) == weights.spec(weights.OD)
    assert weights.od_spec()[-2][1] == (512, 2) and weights.n_params(weights.OD) == 1548706
    a, b = weights.initial_od(3), weights.initial_od(3, 2)
    assert all(a[n].tobytes() == b[n].tobytes() for n in a)
    a, b = weights.synthetic(weights.OD, 3), weights.synthetic(weights.OD, 3, n_classes=2)
    assert all(a[n].tobytes() == b[n].tobytes() for n in a)


@pytest.mark.parametrize('K', KC.KS)
def test_round_trips_and_sizes(K):
    W = weights.synthetic(weights.OD, seed=4, n_classes=K)
    assert weights.od_spec(K)[-2:] == [(HEAD + '/kernel', (512, K), 'kernel'), (HEAD + '/bias', (K,), 'bias')]
    assert weights.od_spec(K)[:-2] == weights.od_spec()[:-2]
    weights.check(weights.OD, W, K)
    blob = weights.pack(weights.OD, W, K)
    assert blob.size == weights.n_params(weights.OD, K) == weights.n_params(weights.OD) + 513 * (K - 2)
    assert weights.od_classes_of(blob.size) == K and weights.od_classes(W) == K
    back = weights.unpack(weights.OD, blob, K)
    assert set(back) == set(W) and all(back[n].tobytes() == W[n].tobytes() for n in W)
    with pytest.raises(ValueError):
        weights.pack(weights.OD, W)                       # a K-class dict is not the two-class spec
    with pytest.raises(ValueError):
        weights.unpack(weights.OD, blob)
    with pytest.raises(ValueError):
        weights.od_classes_of(blob.size + 1)


@pytest.mark.parametrize('K', KC.KS)
def test_every_tensor_but_the_head_is_the_two_class_draw(K):
    for two, many in ((weights.initial_od(6), weights.initial_od(6, K)),
                      (weights.synthetic(weights.OD, 6), weights.synthetic(weights.OD, 6, n_classes=K))):
        assert set(two) == set(many)
        for n in two:
            if not n.startswith(HEAD):
                assert two[n].tobytes() == many[n].tobytes(), n
    W0 = weights.initial_od(6, K)
    lim = np.sqrt(6.0 / (512 + K))                       # Glorot uniform, zero bias
    assert W0[HEAD + '/kernel'].shape == (512, K) and np.abs(W0[HEAD + '/kernel']).max() <= lim
    assert np.abs(W0[HEAD + '/kernel']).max() > 0.9 * lim and not W0[HEAD + '/bias'].any()


def test_classes_outside_the_range_are_refused():
    for K in (1, 9):
        with pytest.raises(ValueError):
            weights.od_spec(K)
        with pytest.raises(ValueError):
            weights.initial_od(0, K)


def test_save_overlap_round_trip_three_classes(tmp_path):
    from mmla_audio_amd import tfbundle
    W = KC.synthetic(2, 3)
    tfbundle.save_overlap(str(tmp_path), W)
    got, (kind, k, head) = tfbundle.load_bundle(str(tmp_path), with_layout=True)
    assert (kind, k, head) == (weights.OD, 3, _lib.HEAD_SOFTMAX) and set(got) == set(W)
    for name in W:
        assert got[name].dtype == np.float32 and got[name].tobytes() == W[name].tobytes(), name


# ---- labels, evaluation, log text ---------------------------------------------------------------------------

def test_class_labels_accept_one_hot_rows_of_k_classes():
    y = np.eye(3)[[2, 0, 1, 2]]
    assert overlap_detector._class_labels(y, 'y').tolist() == [2, 0, 1, 2]
    assert overlap_detector._class_labels(np.eye(2)[[1, 0]], 'y').tolist() == [1, 0]
    for bad in (np.eye(9)[[0]], np.ones((2, 3)), np.eye(3)[[0]] * 2, np.zeros((2, 1))):
        with pytest.raises(ValueError):
            overlap_detector._class_labels(bad, 'y')
    n = overlap_detector._n_classes
    assert n(None, y, None) == 3 and n(None, np.array([0, 2, 1]), None) == 3 and n(None, np.array([0, 0])) == 2
    assert n(None, np.array([0, 1]), np.array([2])) == 3 and n(4, y) == 4


class _Fixed:
    """a model whose predict returns given rows"""

    def __init__(self, probs):
        self.probs = np.asarray(probs, np.float32)
        self.n_classes = self.probs.shape[1]

    def predict(self, x):
        return self.probs


@pytest.mark.parametrize('K', (2, 3, 5))
def test_evaluation_matrix_is_sklearns(K, capsys):
    rng = np.random.default_rng([51, K])
    n = 40
    probs = rng.random((n, K)).astype(np.float32)
    truth = rng.integers(0, K, n)
    m, recall, precision = overlap_detector.evaluation(_Fixed(probs), np.zeros((n, 1)), np.eye(K)[truth])
    pred = probs.argmax(1)
    assert m.shape == (K, K) and m.sum() == n
    try:
        from sklearn.metrics import confusion_matrix
    except ImportError:
        confusion_matrix = None
    if confusion_matrix is not None:
        assert np.array_equal(m, confusion_matrix(truth, pred, labels=list(range(K))))
    tp = int(((truth == K - 1) & (pred == K - 1)).sum())
    assert recall == tp / int((truth == K - 1).sum()) and precision == tp / int((pred == K - 1).sum())
    m2, _, _ = overlap_detector.evaluation(_Fixed(probs), np.zeros((n, 1)), truth)       # integer labels too
    assert np.array_equal(m, m2)
    out = capsys.readouterr().out
    assert 'Overlapped recall: ' in out and ' precision: ' in out and str(m) in out
    with pytest.raises(ValueError):
        overlap_detector.evaluation(_Fixed(probs), np.zeros((n, 1)), np.full(n, K))


def test_log_text_of_a_k_class_model():
    assert [odpp.class_label(k) for k in (0, 1, -1)] == ['non-overlapped', 'overlapped', 'silent']
    assert [odpp.class_label(k, 3) for k in (0, 1, 2, -1)] == ['0', '1', '2', 'silent']


# ---- AUC --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', (1, 65, 1000))
def test_auc_restatement_equals_the_two_class_one(n):
    probs, labels = KC.auc_inputs(n, 2)
    for lab in (labels, np.zeros(n, np.int32), np.ones(n, np.int32)):
        assert KC.auc(probs, lab).tobytes() == tr.auc(probs, lab).tobytes()
    on, nudged = tr.on_threshold_case()
    for p in (on, nudged):
        assert KC.auc(p, [0]).tobytes() == tr.auc(p, [0]).tobytes()


def test_auc_restatement_at_three_classes_by_hand():
    # one sample of class 2: TP entry 0.7, FP entries 0.2 and 0.1.  recall steps 1 -> 0 at 0.7; fpr 1 -> 0.5 at
    # 0.1 -> 0 at 0.2: the area is 1 (every drop of fpr happens at recall 1)
    assert float(KC.auc(np.array([[0.1, 0.2, 0.7]], np.float32), [2])) == 1.0
    # ... and labelled 0 the true entry is the lowest: the area is 0
    assert float(KC.auc(np.array([[0.1, 0.2, 0.7]], np.float32), [0])) == 0.0
    # the pooled binary view (od_train_ref.auc_binary over the n K entries) is the same number
    probs, labels = KC.auc_inputs(65, 3)
    pooled = tr.auc_binary(probs.ravel(), np.eye(3, dtype=bool)[labels].ravel())
    assert KC.auc(probs, labels).tobytes() == pooled.tobytes()


# ---- the conditions of the GPU cases ------------------------------------------------------------------------

@pytest.mark.parametrize('K', KC.KS)
@pytest.mark.parametrize('h,w,B', KC.GRAD_SHAPES)
def test_gradient_cases_have_their_margins_and_no_clipped_sample(h, w, B, K):
    W, img, labels, mask = KC.grad_case(h, w, B, K)
    assert labels[-1] == K - 1 and labels.max() < K
    m = KC.grad_ref(h, w, B, K)['f64'][3]
    q = KC.q_true(W, img, labels, mask)
    print(h, w, B, K, m, q)
    assert m['pool'] >= C.MARGIN and m['leaky'] >= C.MARGIN, m
    assert (q > KC.CLIP_LO).all() and (q < KC.CLIP_HI).all()


def test_clip_case_clips():
    W, img, labels, mask = KC.clip_case()
    q = KC.q_true(W, img, labels, mask)
    print(q)
    assert (q < KC.CLIP_LO).all()


@pytest.mark.parametrize('K', KC.KS)
def test_forward_inputs_are_decided(K):
    W = KC.synthetic(1, K)
    ref = nets.od_forward(KC.forward_inputs().astype(np.float32), W)
    assert ref.shape == (5, K) and np.allclose(ref.sum(axis=1), 1)
    assert compare.near_ties(ref).mean() < 0.05


def test_fit_case_has_every_class_and_its_margins():
    c = KC.fit_case()
    assert set(c['labels']) == set(c['val_labels']) == {0, 1, 2}
    r = KC.fit_ref()
    assert r['f64'][2] == r['f32'][2] == KC.FIT['epochs']
    print(r['f64'][3], r['f64'][1])
    C.check_updates(c['W'], r['f32'][0], r['f64'][0], C.fit_lr_sum(c, KC.FIT), 'float32 restatement')


def test_fit_case_probs_are_far_from_the_auc_thresholds():
    # the GPU test wants 1e-5 of the fitted model's float64 probs; the restatement's own fit has five times that
    val, train = KC.auc_margins()
    print(val, train)
    assert min(val) > 5e-5 and train > 1e-5
