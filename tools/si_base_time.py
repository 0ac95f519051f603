"""Time a TIMIT-sized SI base-model fit (mmla_si_base_train): 6300 training windows, no validation set, batch
32 (197 steps an epoch, the last of 28 windows), K = 630, synthetic features standard_normal * 10, the weights
of weights.initial, device pointers, wall clock around the call and the stream synchronisation.  Two calls of
epochs = 1 and two of epochs = 3; the second of each pair counts, and the step time is the difference of the
two over the 2 * 197 steps between them, so what a call costs once (argument checks, workspace, the blob's
copy) drops out.  Beside it the float32 restatement (tests/si_base_ref.py) on the same host's CPU.

    python tools/si_base_time.py [--no-cpu] [--cpu-steps N] [--cpu-threads 16]
    python tools/si_base_time.py --trace-run      # one epochs = 1 call and nothing else, for a kernel trace

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
sys.path.insert(0, os.path.join(REPO, 'tests'))

N_TRAIN, BATCH, K = 6300, 32, 630
DROP_SEED = 0x9E3779B97F4A7C15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--cpu-steps', type=int, default=3, help='steps of the CPU restatement to time')
    ap.add_argument('--cpu-threads', type=int, default=16)
    ap.add_argument('--trace-run', action='store_true')
    a = ap.parse_args()
    import torch
    from mmla_audio_amd import _lib, weights
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((N_TRAIN, 256, 39)) * 10).astype(np.float32)
    labels = rng.integers(0, K, N_TRAIN).astype(np.int32)
    Wd = weights.initial(weights.SI, 0, K)
    blob = weights.pack(weights.SI, Wd, K)
    perm = np.stack([rng.permutation(N_TRAIN) for _ in range(3)]).astype(np.int32)
    ctx = _lib.Context(0)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
           for k, v in dict(blob=blob, x=x, labels=labels, perm=perm).items()}
    out = torch.zeros(blob.size, dtype=torch.float32, device='cuda')
    hist = torch.zeros((3, 4), dtype=torch.float32, device='cuda')
    words = torch.zeros(2, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()

    def fit(epochs):
        t = time.perf_counter()
        ctx.si_base_train_dev(dev['blob'].data_ptr(), blob.size, K, dev['x'].data_ptr(), dev['labels'].data_ptr(),
                              N_TRAIN, 0, 0, 0, epochs, BATCH, 1e-4, dev['perm'].data_ptr(), DROP_SEED, 0, 0,
                              out.data_ptr(), 0, hist.data_ptr(), words.data_ptr(), words.data_ptr() + 4)
        ctx.synchronize()
        return time.perf_counter() - t

    if a.trace_run:
        print(json.dumps(dict(tool='si_base_time', trace_run=True, seconds=round(fit(1), 4))))
        ctx.close()
        return
    steps = -(-N_TRAIN // BATCH)
    t1 = [fit(1), fit(1)]
    t3 = [fit(3), fit(3)]
    res = dict(tool='si_base_time', n_train=N_TRAIN, n_val=0, batch=BATCH, n_classes=K, steps_per_epoch=steps,
               gpu_seconds_epochs1=[round(t, 4) for t in t1], gpu_seconds_epochs3=[round(t, 4) for t in t3],
               gpu_ms_per_step=round(1e3 * (t3[1] - t1[1]) / (2 * steps), 3),
               gpu_seconds_per_epoch=round((t3[1] - t1[1]) / 2, 4), history=hist.cpu().numpy().tolist())
    ctx.close()
    if not a.no_cpu:
        import si_base_ref as ref
        torch.set_num_threads(a.cpu_threads)
        ns = max(1, a.cpu_steps)
        n = (ns + 1) * BATCH                       # one step more: the first warms torch up and is not counted
        order = np.arange(n, dtype=np.int32)[None]

        def cpu(steps_):
            t = time.perf_counter()
            m = steps_ * BATCH
            ref.fit(Wd, K, x[:m], labels[:m], None, None, order[:, :m], 1, BATCH, 1e-4, DROP_SEED,
                    dtype=torch.float32)
            return time.perf_counter() - t

        c1, call = cpu(1), cpu(ns + 1)
        res.update(cpu_threads=a.cpu_threads, cpu_steps=ns, cpu_ms_per_step=round(1e3 * (call - c1) / ns, 1))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
