"""Time a room-sized OD adaptation (mmla_od_finetune): 512 training + 128 validation feature images at
128 x 151, batch 16, 3 epochs after a one-epoch warm-up, synthetic weights, device pointers, wall clock around
the call and the stream synchronisation, three repeats.  Beside it one epoch of the float32 restatement
(tests/od_finetune_ref.py) on 16 CPU threads of the same machine.

    python tools/od_finetune_time.py [--epochs 3] [--repeats 3] [--no-cpu] [--cpu-batches N]

Prints one JSON line.  `wgrad_flop_per_step` is the weight gradients' arithmetic at batch 16 (2 * pixels *
taps * cin * cout over every convolution): with a kernel trace of one run (the share of wgrad_kernel) it
gives that kernel's achieved FLOP/s against the f32 MFMA peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

H, W_, N_TRAIN, N_VAL, BATCH = 128, 151, 512, 128, 16
CH = (32, 32, 32, 64, 64, 64, 128, 128, 128)
POOL = (True, False, False, True, False, False, True, False, False)


def wgrad_flop(batch):
    h, w, cin, total = H, W_, 16, 2.0 * batch * H * W_ * 3 * 16
    for c, pool in zip(CH, POOL):
        pix = batch * h * w
        total += 2.0 * pix * (9 * cin * c + 4 * c * c)
        if pool:
            h, w = (h + 1) // 2, (w + 1) // 2
            total += 2.0 * batch * h * w * cin * c
        cin = c
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--cpu-batches', type=int, default=N_TRAIN // BATCH,
                    help='batches of the CPU epoch to run (fewer: the epoch is extrapolated)')
    a = ap.parse_args()
    import torch
    from mmla_audio_amd import _lib, overlap_detector, weights
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (N_TRAIN + N_VAL, H, W_, 3)).astype(np.uint8)
    labels = rng.integers(0, 2, N_TRAIN + N_VAL).astype(np.int32)
    Wd = weights.synthetic(weights.OD, seed=0)
    blob = weights.pack(weights.OD, Wd)
    ep = max(a.epochs, 1)
    perm = np.stack([rng.permutation(N_TRAIN) for _ in range(ep)]).astype(np.int32)
    mask = (rng.random((ep, N_TRAIN, 512)) >= 0.25).astype(np.uint8)
    lr = overlap_detector.cosine_lr(ep).astype(np.float32)
    ctx = _lib.Context(0)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
           for k, v in dict(blob=blob, img=img[:N_TRAIN], labels=labels[:N_TRAIN], vimg=img[N_TRAIN:],
                            vlabels=labels[N_TRAIN:], perm=perm, mask=mask).items()}
    out = torch.zeros(blob.size, dtype=torch.float32, device='cuda')
    hist = torch.zeros((ep, 5), dtype=torch.float32, device='cuda')
    ran = torch.zeros(1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()

    def fit(epochs):
        t = time.perf_counter()
        ctx.od_finetune_dev(dev['blob'].data_ptr(), blob.size, dev['img'].data_ptr(), dev['labels'].data_ptr(),
                            N_TRAIN, dev['vimg'].data_ptr(), dev['vlabels'].data_ptr(), N_VAL, H, W_, (1.0, 1.0),
                            epochs, BATCH, lr, dev['perm'].data_ptr(), dev['mask'].data_ptr(), 0, out.data_ptr(),
                            hist.data_ptr(), ran.data_ptr())
        ctx.synchronize()
        return time.perf_counter() - t

    fit(1)                                   # warm-up: allocations, code objects
    times = [fit(a.epochs) for _ in range(a.repeats)]
    steps = a.epochs * (N_TRAIN // BATCH)
    res = dict(tool='od_finetune_time', n_train=N_TRAIN, n_val=N_VAL, h=H, w=W_, batch=BATCH, epochs=a.epochs,
               gpu_seconds=[round(t, 4) for t in times], gpu_seconds_per_epoch=round(min(times) / a.epochs, 4),
               gpu_ms_per_step_incl_val=round(1e3 * min(times) / steps, 3),
               wgrad_flop_per_step=wgrad_flop(BATCH), history_last=hist.cpu().numpy()[-1].tolist())
    ctx.close()
    if not a.no_cpu:
        import od_finetune_ref as ref
        torch.set_num_threads(16)
        nb = max(1, min(a.cpu_batches, N_TRAIN // BATCH))
        n = nb * BATCH
        t = time.perf_counter()
        ref.fit(Wd, img[:n], labels[:n], img[N_TRAIN:] if nb == N_TRAIN // BATCH else None,
                labels[N_TRAIN:] if nb == N_TRAIN // BATCH else None, (1.0, 1.0), lr,
                np.arange(n, dtype=np.int32)[None], mask[:1, :n], 1, BATCH, 0, torch.float32)
        dt = time.perf_counter() - t
        res.update(cpu_threads=16, cpu_batches=nb, cpu_seconds=round(dt, 2),
                   cpu_seconds_per_epoch=round(dt * (N_TRAIN // BATCH) / nb, 2))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
