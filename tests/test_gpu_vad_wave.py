"""GPU: the speech detector with one stream per wave (vad_speech_wave_kernel) against the detector with
one thread per stream (vad_speech_kernel) and against the CPU oracle.

The arithmetic is integer and both kernels keep every chain's order, so every comparison is
array_equal: per-frame flags, voiced PCM and its length, and -- through a further call -- the state
left behind.  The per-thread side is a context created under MMLA_NO_VADW=1; the wave side is a default
context where mmla_debug_vad_path says 'wave' for the stream count, else one created under MMLA_VADW=1.
Clips: the generator of tests/test_gpu_vad.py (voiced stretches, a near-silent stretch, a digital-zero
gap), a pool of eight made once and shared read-only."""
import os

import numpy as np
import pytest

from oracle import synth, vad as ovad, webrtc_vad

pytestmark = pytest.mark.gpu

ROW = 40960
LENS_SET = (0, 479, 480, 481, 960, 961, 12000, ROW)


def _clip(seed, n=ROW):
    """voiced synth with silent gaps (and one near-silent stretch) -- VAD on and off"""
    rng = np.random.default_rng(seed)
    x = synth.clip(seed * 5, n).astype(np.int32)            # class 0: voiced
    a, b = sorted(rng.integers(0, n, 2))
    x[a:b] = rng.integers(-3, 4, b - a)
    c = int(rng.integers(0, n // 2))
    x[c:c + 4800] = 0
    return x.astype(np.int16)


def _ctx_under(name):
    from mmla_audio_amd import _lib
    old = os.environ.get(name)
    os.environ[name] = '1'
    try:
        return _lib.Context(0)
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.fixture(scope='module')
def thread_ctx():
    c = _ctx_under('MMLA_NO_VADW')
    yield c
    c.close()


@pytest.fixture(scope='module')
def default_ctx():
    from mmla_audio_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def forced_ctx():
    c = _ctx_under('MMLA_VADW')
    yield c
    c.close()


@pytest.fixture(scope='module')
def wave_ctx(default_ctx, forced_ctx):
    """n_streams -> a context whose detector call over that many streams runs the wave kernel"""
    def pick(n_streams):
        c = default_ctx if default_ctx.debug_vad_path(n_streams) else forced_ctx
        assert c.debug_vad_path(n_streams)
        return c
    return pick


@pytest.fixture(scope='module')
def pool():
    x = np.stack([_clip(100 + s) for s in range(8)])
    x.setflags(write=False)
    return x


def _same(got, want, what=''):
    (out_g, fl_g), (out_w, fl_w) = got, want
    assert len(out_g) == len(out_w) and len(fl_g) == len(fl_w)
    for i in range(len(out_w)):
        assert np.array_equal(fl_g[i], fl_w[i]), (what, i, 'frame flags')
        assert len(out_g[i]) == len(out_w[i]), (what, i, 'out_lens')
        assert np.array_equal(out_g[i], out_w[i]), (what, i, 'voiced PCM')


def test_symbol_and_switches(default_ctx, thread_ctx, forced_ctx):
    assert default_ctx.debug_vad_path(1) is True
    for n in (1, 64, 4096, 1 << 20):
        assert thread_ctx.debug_vad_path(n) is False
        assert forced_ctx.debug_vad_path(n) is True
    from mmla_audio_amd import _lib
    with pytest.raises(_lib.MmlaError):
        default_ctx.debug_vad_path(0)


@pytest.mark.parametrize('mode', [0, 3])
@pytest.mark.parametrize('ips', [1, 3])
@pytest.mark.parametrize('streams', [1, 2, 5, 65])
def test_wave_equals_per_thread(thread_ctx, wave_ctx, pool, streams, ips, mode):
    """a lone stream, a partial group, one more than 64 streams; items of unequal lens on rows of 40960"""
    n = streams * ips
    x = np.ascontiguousarray(pool[(np.arange(n) * 3 + streams) % len(pool)])
    lens = np.array([LENS_SET[(7 - i) % 8] for i in range(n)], np.int32)
    res = []
    for c in (thread_ctx, wave_ctx(streams)):
        c.vad_reset(streams, mode)
        first = c.vad_remove_silence(x, lens=lens, items_per_stream=ips)
        # a second call, full rows: it starts from the state the first left behind
        second = c.vad_remove_silence(x[::-1], items_per_stream=ips)
        res.append((first, second))
    _same(res[1][0], res[0][0], 'first call')
    _same(res[1][1], res[0][1], 'second call')
    flags = np.concatenate([f for f in res[0][1][1]])
    assert flags.any() and not flags.all()


def _square():
    """19 frames of a full-scale square wave (+32767 / -32768, period 32), then 19 frames of zeros"""
    x = np.zeros(38 * 480 + 1, np.int16)
    t = np.arange(19 * 480)
    x[:19 * 480] = np.where((t // 16) % 2 == 0, 32767, -32768)
    return x


def test_full_scale_square_then_zeros(thread_ctx, wave_ctx):
    """the wrapping paths of the filters and the energy, the hangover and the total <= MIN_ENERGY path"""
    x = _square()
    o, f = ovad.remove_silence(x, webrtc_vad.Vad(0).is_speech)
    assert len(f) == 38 and list(f) == [True] * 25 + [False] * 13, list(f)
    for c in (thread_ctx, wave_ctx(1)):
        c.vad_reset(1, 0)
        out, flags = c.vad_remove_silence([x])
        assert np.array_equal(flags[0], f) and np.array_equal(out[0], o)


def test_state_carries_across_calls(thread_ctx, wave_ctx, pool):
    a, b = pool[0], pool[1]
    w = wave_ctx(1)
    w.vad_reset(1, 3)
    _, fa = w.vad_remove_silence([a])
    _, fb = w.vad_remove_silence([b])
    w.vad_reset(1, 3)
    _, fab = w.vad_remove_silence([a, b], items_per_stream=2)
    assert np.array_equal(fa[0], fab[0]) and np.array_equal(fb[0], fab[1])
    # the first call on either kernel, then the second call on the state that kernel left: the wave
    # kernel's state after `a` is the per-thread kernel's
    thread_ctx.vad_reset(1, 3)
    _, ta = thread_ctx.vad_remove_silence([a])
    _, tb = thread_ctx.vad_remove_silence([b])
    assert np.array_equal(ta[0], fa[0]) and np.array_equal(tb[0], fb[0])
    fresh = webrtc_vad.Vad(3)
    alone = ovad.remove_silence(b, fresh.is_speech)[1]
    assert not np.array_equal(alone, fb[0]), 'the carried state does not matter on this input'


def test_against_the_cpu_oracle(wave_ctx, pool):
    """3 streams x 2 items, one oracle detector per stream; the short lengths' frame counts"""
    for m, nf in zip(LENS_SET[:6], (0, 0, 0, 1, 1, 2)):
        assert len(ovad.remove_silence(pool[0][:m], webrtc_vad.Vad(3).is_speech)[1]) == nf, m
    x = np.ascontiguousarray(pool[:6])
    c = wave_ctx(3)
    c.vad_reset(3, 3)
    out, flags = c.vad_remove_silence(x, items_per_stream=2)
    seen = []
    for s in range(3):
        ref = webrtc_vad.Vad(3)
        for k in range(2):
            o, f = ovad.remove_silence(x[2 * s + k], ref.is_speech)
            assert np.array_equal(flags[2 * s + k], f), (s, k, 'frame flags')
            assert np.array_equal(out[2 * s + k], o), (s, k, 'voiced PCM')
            seen.append(f)
    seen = np.concatenate(seen)
    assert seen.any() and not seen.all()


def test_device_pointer_lens_clamped_to_the_row(wave_ctx, pool):
    """a device lens entry of three times the row: reads and writes stay inside the item's row"""
    import torch
    from mmla_audio_amd import _lib
    c = wave_ctx(2)
    x = np.ascontiguousarray(pool[2:4])
    n, L = x.shape
    dev = torch.device('cuda:0')
    pcm = torch.from_numpy(x.copy()).to(dev)
    lens = torch.tensor([L, 3 * L], dtype=torch.int32, device=dev)
    guard = 4096
    out = torch.full((n * L + guard,), 12345, dtype=torch.int16, device=dev)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    nf = (L - 1) // 480
    speech = torch.zeros((n, nf), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c.vad_reset(2, 3)
    rc = c.lib.mmla_vad_remove_silence(c.h, pcm.data_ptr(), n, L, lens.data_ptr(), L, 1, out.data_ptr(),
                                       olen.data_ptr(), speech.data_ptr(), nf, _lib.MMLA_DEVICE_PTR)
    c.synchronize()
    assert rc == 0
    assert bool((out[n * L:] == 12345).all()), 'write past the last row'
    assert int(olen.max()) <= L
    c.vad_reset(2, 3)
    want, wflags = c.vad_remove_silence(x)
    got = out[L:L + int(olen[1])].cpu().numpy()
    assert np.array_equal(got, want[1])
    assert np.array_equal(speech[1].cpu().numpy().astype(bool), wflags[1])
