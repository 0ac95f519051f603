"""Time the two device pieces of an OD-NET fit from scratch, device pointers, wall clock around
the call and the stream synchronisation:

  augment   mmla_od_augment on 4096 feature images of 128 x 151, every image at one level (1 and 3): images/s
            and the fraction of the HBM peak that one read and one write of every image amounts to
  fit       mmla_od_train, 512 training + 128 validation images at 128 x 151, batch 64, Keras initial state,
            callbacks off: seconds per epoch after a one-epoch warm-up

    python tools/od_train_time.py [--images 4096] [--epochs 2] [--repeats 3] [--no-fit] [--no-augment] [--lib SO]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

H, W_, N_TRAIN, N_VAL, BATCH = 128, 151, 512, 128, 64
HBM_PEAK = 8.0e12   # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=4096)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-fit', action='store_true')
    ap.add_argument('--no-augment', action='store_true')
    ap.add_argument('--lib', help='an A/B build of the library (make variant) instead of libmmla.so')
    a = ap.parse_args()
    import torch
    from mmla_audio_amd import _lib, overlap_detector, weights
    if a.lib:
        _lib.load_library(a.lib)
    rng = np.random.default_rng(6)
    ctx = _lib.Context(0)
    res = dict(tool='od_train_time', lib=a.lib or 'libmmla.so', h=H, w=W_)
    if not a.no_augment:
        m = a.images
        img = torch.from_numpy(rng.integers(0, 256, (m, H, W_, 3)).astype(np.uint8)).cuda()
        src = torch.arange(m, dtype=torch.int32, device='cuda')
        out = torch.zeros_like(img)
        for level in (1, 3):
            lv = torch.full((m,), level, dtype=torch.int32, device='cuda')
            torch.cuda.synchronize()
            times = []
            for _ in range(a.repeats + 1):                     # the first call warms up
                t = time.perf_counter()
                ctx.od_augment_dev(img.data_ptr(), m, H, W_, src.data_ptr(), lv.data_ptr(), m, out.data_ptr())
                ctx.synchronize()
                times.append(time.perf_counter() - t)
            best = min(times[1:])
            res[f'augment_level{level}'] = dict(
                images=m, seconds=[round(t, 6) for t in times[1:]], images_per_s=round(m / best),
                hbm_fraction=round(2.0 * m * H * W_ * 3 / best / HBM_PEAK, 4))
        del img, out
    if not a.no_fit:
        img = rng.integers(0, 256, (N_TRAIN + N_VAL, H, W_, 3)).astype(np.uint8)
        labels = rng.integers(0, 2, N_TRAIN + N_VAL).astype(np.int32)
        blob = weights.pack(weights.OD, weights.initial_od(0))
        ep = max(a.epochs, 1)
        perm = np.stack([rng.permutation(N_TRAIN) for _ in range(ep)]).astype(np.int32)
        lr = overlap_detector.cosine_lr(ep).astype(np.float32)
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
               for k, v in dict(blob=blob, img=img[:N_TRAIN], labels=labels[:N_TRAIN], vimg=img[N_TRAIN:],
                                vlabels=labels[N_TRAIN:], perm=perm).items()}
        out = torch.zeros(blob.size, dtype=torch.float32, device='cuda')
        hist = torch.zeros((ep, 7), dtype=torch.float32, device='cuda')
        words = torch.zeros(2, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()

        def fit(epochs):
            t = time.perf_counter()
            ctx.od_train_dev(dev['blob'].data_ptr(), blob.size, dev['img'].data_ptr(), dev['labels'].data_ptr(),
                             N_TRAIN, dev['vimg'].data_ptr(), dev['vlabels'].data_ptr(), N_VAL, H, W_, (1.0, 1.0),
                             epochs, BATCH, lr, dev['perm'].data_ptr(), 17, 0, 0, out.data_ptr(), 0, hist.data_ptr(),
                             words.data_ptr(), words.data_ptr() + 4)
            ctx.synchronize()
            return time.perf_counter() - t

        fit(1)                                   # warm-up: allocations, code objects
        times = [fit(a.epochs) for _ in range(a.repeats)]
        res['fit'] = dict(n_train=N_TRAIN, n_val=N_VAL, batch=BATCH, epochs=a.epochs,
                          seconds=[round(t, 4) for t in times],
                          seconds_per_epoch=round(min(times) / a.epochs, 4),
                          history_last=hist.cpu().numpy()[-1].tolist())
    ctx.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
