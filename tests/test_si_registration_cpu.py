"""CPU: the host side of speaker registration -- the deployed-model writer, the split / initial-head
/ shuffle plan, the argument check of transfer_learning, the C ABI additions, and the numpy
restatement of the trainer (tests/si_head_ref.py) against finite differences."""
import ctypes
import os

import numpy as np
import pytest

import si_head_ref
from mmla_audio_amd import _lib, speaker_identification as si, tfbundle, weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _deployed_weights(k, seed=11):
    return weights.synthetic(weights.SI, seed=seed, n_classes=k)


@pytest.mark.parametrize('k', [1, 4, 33])
def test_save_deployed_round_trips_bit_exactly(tmp_path, k):
    W = _deployed_weights(k)
    tfbundle.save_deployed(str(tmp_path), W, k)
    shapes = tfbundle.variable_shapes(str(tmp_path / 'variables' / 'variables.index'))
    kind, n_classes, head, mapping = tfbundle.layout(shapes)
    assert (kind, n_classes, head) == (weights.SI, k, _lib.HEAD_SIGMOID)
    assert mapping['layer_with_weights-1/kernel'] == 'layer_with_weights-42/kernel'
    got, lay = tfbundle.load_bundle(str(tmp_path), with_layout=True)
    assert lay == (weights.SI, k, _lib.HEAD_SIGMOID)
    assert set(got) == set(W)
    for name, want in W.items():
        assert got[name].dtype == np.float32 and got[name].shape == want.shape, name
        assert got[name].tobytes() == want.tobytes(), name


def test_save_deployed_flipped_byte_fails_checksum(tmp_path):
    W = _deployed_weights(4)
    tfbundle.save_deployed(str(tmp_path), W, 4)
    shard = tmp_path / 'variables' / 'variables.data-00000-of-00001'
    raw = bytearray(shard.read_bytes())
    raw[len(raw) // 2] ^= 0x01
    shard.write_bytes(bytes(raw))
    with pytest.raises(ValueError, match='checksum'):
        tfbundle.load_bundle(str(tmp_path))


def test_save_deployed_rejects_wrong_shapes(tmp_path):
    with pytest.raises(ValueError):
        tfbundle.save_deployed(str(tmp_path), _deployed_weights(4), 5)


def test_reference_gradient_matches_central_differences():
    rng = np.random.default_rng(0)
    n, d, k = 5, 7, 4
    e = rng.standard_normal((n, d))
    y = rng.integers(0, k, n)
    w = rng.standard_normal((d, k)) * 0.5
    b = rng.standard_normal(k) * 0.1
    _, gw, gb = si_head_ref.loss_and_grad(w, b, e, y)
    h = 1e-6
    for (i, j) in [(i, j) for i in range(d) for j in range(k)]:
        wp, wm = w.copy(), w.copy()
        wp[i, j] += h
        wm[i, j] -= h
        fd = (si_head_ref.loss_and_grad(wp, b, e, y)[0] - si_head_ref.loss_and_grad(wm, b, e, y)[0]) / (2 * h)
        assert abs(fd - gw[i, j]) < 1e-8, (i, j, fd, gw[i, j])
    for j in range(k):
        bp, bm = b.copy(), b.copy()
        bp[j] += h
        bm[j] -= h
        fd = (si_head_ref.loss_and_grad(w, bp, e, y)[0] - si_head_ref.loss_and_grad(w, bm, e, y)[0]) / (2 * h)
        assert abs(fd - gb[j]) < 1e-8, (j, fd, gb[j])


def test_reference_clipped_sample_has_zero_gradient():
    """K = 1: p = 1 is above the upper clip bound, clip_by_value passes no gradient"""
    rng = np.random.default_rng(1)
    e = rng.standard_normal((6, 7))
    loss, gw, gb = si_head_ref.loss_and_grad(rng.standard_normal((7, 1)), np.zeros(1), e, np.zeros(6, int),
                                             np.float32)
    assert not gw.any() and not gb.any()
    assert loss == -np.log(np.float32(1) - np.float32(1e-7))


def test_fit_plan_invariants():
    labels = np.array([0] * 9 + [1] * 5 + [2] * 2 + [3] * 1 + [4] * 13)
    for ratio in (0, 0.2):
        p = si._fit_plan(labels, 5, 7, ratio, 3, 2)
        q = si._fit_plan(labels, 5, 7, ratio, 3, 2)
        for key in p:
            assert np.array_equal(p[key], q[key]), key
        parts = [p['train'], p['val'], p['test']]
        allidx = np.concatenate(parts)
        assert len(allidx) == len(labels) and np.array_equal(np.sort(allidx), np.arange(len(labels)))
        assert (len(p['test']) > 0) == (ratio > 0)
        rest = np.sort(np.concatenate([p['train'], p['val']]))
        for c in range(5):
            n_c = (labels == c).sum()
            if ratio > 0 and n_c >= 2:
                assert (labels[p['test']] == c).any() and (labels[rest] == c).any(), c
            if (labels[rest] == c).sum() >= 2:
                assert (labels[p['train']] == c).any() and (labels[p['val']] == c).any(), c
        assert p['w0'].shape == (2, 512, 5) and p['w0'].dtype == np.float32
        assert np.abs(p['w0']).max() <= np.sqrt(6.0 / 517) and p['w0'].std() > 0.03
        assert not p['b0'].any() and p['b0'].shape == (2, 5)
        assert p['perm'].shape == (2, 3, len(p['train'])) and p['perm'].dtype == np.int32
        assert (np.sort(p['perm'], axis=2) == np.arange(len(p['train']))).all()
    assert not np.array_equal(si._fit_plan(labels, 5, 8, 0, 3, 2)['perm'], p['perm'])
    # restart r's head and order do not depend on how many restarts are drawn
    one = si._fit_plan(labels, 5, 7, 0.2, 3, 1)
    assert np.array_equal(one['w0'][0], p['w0'][0]) and np.array_equal(one['perm'][0], p['perm'][0])


def test_transfer_learning_rejects_rows_that_are_not_one_hot(tmp_path):
    x = np.zeros((4, 256, 39))
    for bad_row in ([1, 1, 0], [0, 0, 0], [0.5, 0.5, 0], [2, 0, 0]):
        y = np.eye(3)[[0, 1, 2, 0]]
        y[2] = bad_row
        with pytest.raises(ValueError, match='one-hot'):
            si.transfer_learning(x, y, 1, 0, str(tmp_path / 'base'), str(tmp_path / 'out'),
                                 allow_synthetic=True)


def test_registration_entry_points_in_abi():
    import test_capi_cpu
    declared = test_capi_cpu.declared_symbols()
    for name in ('mmla_si_embed', 'mmla_si_head_fit'):
        assert name in declared and name in _lib.SIGNATURES
    lib_path = os.path.join(REPO, 'mmla_audio_amd', 'libmmla.so')
    if os.path.exists(lib_path):
        lib = ctypes.CDLL(lib_path)
        assert hasattr(lib, 'mmla_si_embed') and hasattr(lib, 'mmla_si_head_fit')
        assert lib.mmla_abi_version() == 2
        # argument checks come before any device work: a null context is refused
        assert lib.mmla_si_embed(None, None, 0, None, 0) == -1
    header = open(os.path.join(REPO, 'include', 'mmla.h')).read()
    assert '#define MMLA_SI_EMBED 512' in header
    assert f'#define MMLA_SI_TRAIN_MAX_CLASSES {_lib.SI_TRAIN_MAX_CLASSES}' in header
    assert _lib.SI_TRAIN_MAX_CLASSES >= 32 and _lib.NSTAGES == 7


def test_package_exports_registration_names():
    import mmla_audio_amd
    assert mmla_audio_amd.transfer_learning is si.transfer_learning
    assert mmla_audio_amd.transfer_learning_on_experiment is si.transfer_learning_on_experiment
