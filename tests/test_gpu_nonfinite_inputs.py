"""A NaN or an inf in a caller's float input is never silently dropped: the contract is the float64
oracle's, which returns NaN for that clip and leaves the others untouched.

The 3xFP16 range folds are built on fmaxf (which returns its non-NaN argument), the ELU is a median
(NaN -> 0) and the max-pools are fmaxf, so a NaN pixel at an odd row or column of an OD image -- the
stem is a 1 x 1 conv and block 1's strided shortcut reads even pixels only -- used to be staged as
0, never flagged, and the call returned finite probabilities.  The kernels that read a caller's
floats (block 1's staging in the strips and in the tiles, conv_h3's raw-operand staging that
SI-NET's features enter through) now test them; the exact-f32 re-run keeps NaN through its ReLU and
max-pools.

Host call: the bad clip's result is NaN, the other clips are the MMLA_PREC_F32 context's bytes and
within the bar of the oracle.  Device-pointer call: MMLA_E_RANGE is reported, or the bad clip is NaN.
Explicit MMLA_PREC_F32: the bad clip is NaN.  mmla_od_forward_u8 cannot carry a NaN and is unaffected."""
import functools

import numpy as np
import pytest

from oracle import compare, nets

pytestmark = pytest.mark.gpu

N, BAD = 3, 1
VALUES = {'nan': np.nan, '+inf': np.inf, '-inf': -np.inf}
# (row, col) of the image [128, 151]: every parity (the shortcut reads even / even only), the last
# column (block 1's ragged strip, the max-pool's cut window) and the last row
PIXELS = {'odd_odd': (65, 77), 'odd_even': (65, 78), 'even_odd': (64, 77), 'even_even': (64, 78),
          'col150': (33, 150), 'row127': (127, 41)}
OD_SWITCHES = ('MMLA_RB_TILE', 'MMLA_NO_ODU')
# (frame, coefficient) of the SI features [256, 39]: MaxPool1D pairs frames (2 t, 2 t + 1)
CELLS = {'even': (100, 5), 'odd': (101, 20), 'last': (255, 38)}
SI_SWITCHES = ('MMLA_NO_SICHAIN',)
SI_K = 8


def _context(switches, on=None, prec=None):
    from mmla_audio_amd import _lib
    with pytest.MonkeyPatch.context() as mp:
        for k in switches:
            mp.setenv(k, '1' if k == on else '0')
        c = _lib.Context(0)
    if prec is not None:
        c.set_precision(prec)
    return c


def _others(a):
    return np.delete(np.asarray(a), BAD, axis=0)


# ---- OD ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _od_inputs():
    from mmla_audio_amd import weights
    W = weights.synthetic(weights.OD, seed=5)
    x = np.random.default_rng(77).integers(0, 256, size=(N, 128, 151, 3)).astype(np.float32)
    x.setflags(write=False)
    return W, x, nets.od_forward(x, W)


def _od_bad(value, pixel):
    W, x, _ = _od_inputs()
    r, c = PIXELS[pixel]
    bad = x.copy()
    bad[BAD, r, c, (r + c) % 3] = VALUES[value]
    return bad


@functools.lru_cache(maxsize=None)
def _od_oracle_is_nan(value, pixel):
    W = _od_inputs()[0]
    with np.errstate(all='ignore'):
        return bool(np.isnan(nets.od_forward(_od_bad(value, pixel)[BAD:BAD + 1], W)).all())


@functools.lru_cache(maxsize=None)
def _od_ctx(mode):
    from mmla_audio_amd import _lib, weights
    c = _context(OD_SWITCHES, mode, _lib.PREC_F32 if mode == 'f32' else None)
    c.load_weights(weights.OD, weights.pack(weights.OD, _od_inputs()[0]), 2)
    return c


@pytest.mark.parametrize('pixel', PIXELS)
@pytest.mark.parametrize('value', VALUES)
@pytest.mark.parametrize('mode', ('strips',) + OD_SWITCHES)
def test_od_float_image(mode, value, pixel):
    import torch
    from mmla_audio_amd import _lib
    _, _, ref = _od_inputs()
    assert _od_oracle_is_nan(value, pixel)
    bad = _od_bad(value, pixel)
    c, f32 = _od_ctx(mode), _od_ctx('f32')
    p = c.od_forward(bad)
    p32 = f32.od_forward(bad)
    print(f'{mode} {value} {pixel}: bad clip {p[BAD]}, f32 {p32[BAD]}')
    assert np.isnan(p32[BAD]).all()                              # explicit MMLA_PREC_F32
    assert np.isnan(p[BAD]).all()                                # host call
    assert np.array_equal(_others(p), _others(p32))
    assert compare.logp_err(_others(p), _others(ref)) <= compare.LOGP_TOL
    before = c.range_check()
    x = torch.from_numpy(bad).cuda()
    probs = torch.zeros((N, 2), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    c.od_forward_dev(x.data_ptr(), N, probs.data_ptr())
    try:
        c.range_check()
    except _lib.MmlaError as e:
        assert e.code == _lib.MMLA_E_RANGE
    else:
        assert np.isnan(probs.cpu().numpy()[BAD]).all()
    assert c.range_check() == before


def test_od_u8_image_unaffected():
    """the u8 entry cannot carry a NaN: nothing is flagged, and it gives the float entry's bits"""
    W, x, ref = _od_inputs()
    c = _od_ctx('strips')
    before = c.range_check()
    p = c.od_forward(x.astype(np.uint8))
    assert c.range_check() == before
    assert np.array_equal(p, c.od_forward(x)) and c.range_check() == before
    assert compare.logp_err(p, ref) <= compare.LOGP_TOL


# ---- SI ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _si_inputs():
    from mmla_audio_amd import weights
    W = weights.synthetic(weights.SI, seed=7, n_classes=SI_K)
    x = (np.random.default_rng(78).standard_normal((N, 256, 39)) * 10).astype(np.float32)
    x.setflags(write=False)
    Wi = dict(W)     # the oracle's Dense as a 512 x 512 identity: its logits are the BiLSTM output
    Wi['layer_with_weights-42/kernel'] = np.eye(512, dtype=np.float32)
    Wi['layer_with_weights-42/bias'] = np.zeros(512, np.float32)
    return W, Wi, x, nets.si_forward(x, W, head='sigmoid'), nets.si_forward(x, Wi, return_logits=True)


def _si_bad(value, cell):
    x = _si_inputs()[2]
    t, d = CELLS[cell]
    bad = x.copy()
    bad[BAD, t, d] = VALUES[value]
    return bad


@functools.lru_cache(maxsize=None)
def _si_oracle_is_nan(value, cell):
    W, Wi = _si_inputs()[:2]
    one = _si_bad(value, cell)[BAD:BAD + 1]
    with np.errstate(all='ignore'):
        return bool(np.isnan(nets.si_forward(one, W, head='sigmoid')).all() and
                    np.isnan(nets.si_forward(one, Wi, return_logits=True)).all())


@functools.lru_cache(maxsize=None)
def _si_ctx(mode):
    from mmla_audio_amd import _lib, weights
    c = _context(SI_SWITCHES, mode, _lib.PREC_F32 if mode == 'f32' else None)
    c.load_weights(weights.SI, weights.pack(weights.SI, _si_inputs()[0], SI_K), SI_K, _lib.HEAD_SIGMOID)
    return c


@pytest.mark.parametrize('cell', CELLS)
@pytest.mark.parametrize('value', VALUES)
@pytest.mark.parametrize('mode', ('chain',) + SI_SWITCHES)
def test_si_features(mode, value, cell):
    import torch
    from mmla_audio_amd import _lib
    _, _, _, ref_p, ref_e = _si_inputs()
    assert _si_oracle_is_nan(value, cell)
    bad = _si_bad(value, cell)
    c, f32 = _si_ctx(mode), _si_ctx('f32')
    p, p32 = c.si_forward(bad), f32.si_forward(bad)
    e, e32 = c.si_embed(bad), f32.si_embed(bad)
    print(f'{mode} {value} {cell}: bad clip {p[BAD][:3]}, f32 {p32[BAD][:3]}')
    assert np.isnan(p32[BAD]).all() and np.isnan(e32[BAD]).all()     # explicit MMLA_PREC_F32
    assert np.isnan(p[BAD]).all() and np.isnan(e[BAD]).all()         # host calls
    assert np.array_equal(_others(p), _others(p32)) and np.array_equal(_others(e), _others(e32))
    assert compare.logp_err(_others(p), _others(ref_p)) <= compare.LOGP_TOL
    assert np.abs(_others(e) - _others(ref_e)).max() <= 1e-5 * np.abs(ref_e).max()
    before = c.range_check()
    x = torch.from_numpy(bad).cuda()
    for call, width in ((c.si_forward_dev, SI_K), (c.si_embed_dev, 512)):
        out = torch.zeros((N, width), dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        call(x.data_ptr(), N, out.data_ptr())
        try:
            c.range_check()
        except _lib.MmlaError as err:
            assert err.code == _lib.MMLA_E_RANGE
        else:
            assert np.isnan(out.cpu().numpy()[BAD]).all()
    assert c.range_check() == before
