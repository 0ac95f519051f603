"""One fit driver (csrc/fit_common.h) serves mmla_si_finetune, mmla_si_base_train and mmla_od_finetune over two
workspace slots that every entry carves its own way, and the SI entries share theirs.  Whatever ran before on a
context must not show in a call's results: every trainer entry, run on ONE context in an interleaved order,
gives the bytes it gives as the first call on a fresh context.

Inputs: the smallest cases of the trainers' own tests (FIT, STOP and GRAD_CASES of si_base_cases and
od_finetune_cases, si_finetune_cases' fit and gradient cases)."""
import numpy as np
import pytest

import od_finetune_cases as OC
import si_base_cases as BC
import si_finetune_cases as FC
from mmla_audio_amd import _lib, weights

pytestmark = pytest.mark.gpu


def _si_fit(ctx):
    c = FC.fit_case()
    return ctx.si_finetune(weights.pack(weights.SI, c['W'], FC.K), FC.K, c['x'], c['labels'], c['val_x'],
                           c['val_labels'], c['perm'], FC.FIT['epochs'], FC.FIT['batch'], FC.FIT['lr'])


def _si_grad(ctx):
    W, x, labels = FC.grad_case(2)
    return ctx.si_loss_grad(weights.pack(weights.SI, W, FC.K), FC.K, x, labels)


def _base_fit(cfg, case):
    def run(ctx):
        c = case()
        out, best, hist, ran, best_ep = ctx.si_base_train(
            BC.pack(c['W'], BC.FIT_K), BC.FIT_K, c['x'], c['labels'], c['val_x'], c['val_labels'], c['perm'],
            cfg['epochs'], cfg['batch'], cfg['lr'], BC.DROP_SEED, cfg['patience'], cfg['ckpt_period'])
        return out, best, hist, np.array([ran, best_ep])
    return run


def _base_grad(B, K):
    def run(ctx):
        W, x, labels, ids, _ = BC.grad_case(B, K)
        return ctx.si_base_loss_grad(BC.pack(W, K), K, x, labels, BC.DROP_SEED, BC.GRAD_EPOCH, ids, moving=True)
    return run


def _od_fit(ctx):
    c, cfg = OC.fit_case(), OC.FIT
    out, hist, ran = ctx.od_finetune(OC.pack(c['W']), c['img'], c['labels'], c['val_img'], c['val_labels'],
                                     OC.CLASS_W, c['lr'], c['perm'], c['masks'], cfg['epochs'], cfg['batch'], 0)
    return out, hist, np.array([ran])


def _od_grad(h, w, B):
    def run(ctx):
        W, img, labels, mask = OC.grad_case(h, w, B)
        return ctx.od_loss_grad(OC.pack(W), img, labels, OC.CLASS_W, mask, moving=True)
    return run


CALLS = {
    'si_fit': _si_fit,
    'si_grad': _si_grad,
    'base_fit': _base_fit(BC.FIT, BC.fit_case),            # runs every epoch, with a checkpoint
    'base_stop': _base_fit(BC.STOP, BC.stop_case),         # stops early
    'base_grad_1x3': _base_grad(1, 3),
    'base_grad_2x70': _base_grad(2, 70),                   # a wider head: another carving of the SI slot
    'od_fit': _od_fit,
    'od_grad_20x23': _od_grad(20, 23, 3),
    'od_grad_9x8': _od_grad(9, 8, 1),
}
# fit A, loss-grad B, fit C, loss-grad A, fit B ...; the entries that share a slot follow each other with a
# larger and with a smaller carving before them, and two calls come a second time
ORDER = ('si_fit', 'base_grad_1x3', 'od_fit', 'si_grad', 'base_stop', 'od_grad_20x23', 'base_fit',
         'base_grad_2x70', 'od_grad_9x8', 'si_fit', 'od_fit', 'base_stop', 'si_grad', 'od_grad_20x23')


def _bytes(res):
    return [None if a is None else np.ascontiguousarray(a).tobytes() for a in res]


def test_interleaved_calls_on_one_context_equal_first_calls_on_fresh_contexts():
    assert set(ORDER) == set(CALLS)
    fresh = {}
    for name, call in CALLS.items():
        ctx = _lib.Context(0)
        try:
            fresh[name] = _bytes(call(ctx))
        finally:
            ctx.close()
    stop = fresh['base_stop']
    ran = np.frombuffer(stop[3], dtype=np.array([0]).dtype)[0]
    assert 0 < ran < BC.STOP['epochs'], 'the early-stopping case no longer stops early'
    assert np.frombuffer(fresh['base_fit'][3], dtype=np.array([0]).dtype)[0] == BC.FIT['epochs']
    ctx = _lib.Context(0)
    try:
        for i, name in enumerate(ORDER):
            got = _bytes(CALLS[name](ctx))
            assert len(got) == len(fresh[name])
            for k, (g, w) in enumerate(zip(got, fresh[name])):
                assert g == w, f'call {i} ({name}): output {k} differs from the same call on a fresh context'
    finally:
        ctx.close()
