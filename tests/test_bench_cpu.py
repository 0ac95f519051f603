"""CPU: bench.py's host logic -- the --gpus N launcher (ranks started under torch.distributed.run
before any GPU call), the plain / --full options, the --dump-outputs writer, the parity-sample
indices, and the CPU-baseline helpers."""
import os
import sys

import pytest

import bench


def test_gpus_n_launches_torchrun(monkeypatch):
    calls = []
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '2'])
    monkeypatch.setattr(bench.subprocess, 'call', lambda cmd, env=None: calls.append((cmd, env)) or 7)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd, env = calls[0]
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nproc-per-node=4' in cmd and '127.0.0.1' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert os.path.basename(cmd[cmd.index('--master-port') + 2]) == 'bench.py'
    assert cmd[-4:] == ['--gpus', '4', '--steps', '2']
    assert env['MASTER_ADDR'] == '127.0.0.1'


def test_sample_covers_microbatch_edges():
    idx = bench.sample_indices(65536, 16384, 24)
    for c0 in range(0, 65536, 16384):
        assert c0 in idx and c0 + 16383 in idx
    assert len(idx) >= 24 and idx == sorted(set(idx))
    assert bench.sample_indices(5, 16384, 24) == [0, 1, 2, 3, 4]


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'd'])
    a = bench.parse()
    assert a.full and a.dump_outputs == 'd' and a.steps == 3


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """float32 .npy per output; over the size budget the same seeded rows of every array, run to run"""
    import numpy as np
    import torch
    probs = torch.arange(40 * 6, dtype=torch.float32).reshape(40, 6) / 7
    am = torch.arange(40, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / 'a'), {'probs': probs, 'argmax': am})
    assert sorted(os.listdir(tmp_path / 'a')) == ['argmax.npy', 'probs.npy']
    p = np.load(tmp_path / 'a' / 'probs.npy')
    assert p.dtype == np.float32 and np.array_equal(p, probs.numpy())
    a = np.load(tmp_path / 'a' / 'argmax.npy')
    assert a.dtype == np.float32 and np.array_equal(a, np.arange(40))
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 10 * (6 + 1) * 4 + 3)
    for d in 'bc':
        bench.dump_outputs(str(tmp_path / d), {'probs': probs, 'argmax': am})
    idx = np.load(tmp_path / 'b' / 'clip_index.npy')
    assert idx.shape == (10,) and len(set(idx.tolist())) == 10 and (np.diff(idx) > 0).all()
    assert np.array_equal(np.load(tmp_path / 'b' / 'probs.npy'), probs.numpy()[idx.astype(int)])
    assert np.array_equal(np.load(tmp_path / 'b' / 'argmax.npy'), idx.astype(np.float32))
    size = sum(os.path.getsize(tmp_path / 'b' / f) for f in os.listdir(tmp_path / 'b') if f != 'clip_index.npy')
    assert size <= bench.DUMP_BUDGET_BYTES + 2 * 128          # two .npy headers
    for f in os.listdir(tmp_path / 'b'):
        assert np.array_equal(np.load(tmp_path / 'b' / f), np.load(tmp_path / 'c' / f))


def test_cpu_baseline_host_info():
    from oracle import cpu_baseline
    h = cpu_baseline.host_info()
    assert h['os_cpu_count'] >= 1 and h['affinity_cpus'] >= 1 and h['affinity']
    assert cpu_baseline._ranges([0, 1, 2, 5, 7, 8]) == '0-2,5,7-8'
    assert 1 <= cpu_baseline.usable_cores() <= h['affinity_cpus']
