"""rbs_w1l.hip as it compiles here (hipcc, no GPU): exactly one kernel, the blocks 2-3 strip kernel
with GEMM 1's weights in LDS, within the budget of two workgroups per CU -- at most 256 VGPRs (two
waves per SIMD), no spills, no scratch, at most 81 920 B of LDS (half of a CU's 160 KB) -- and with
GEMM 1 fed from LDS alone: each of its 18 k-steps reads two x fragments, and 17 of them two weight
fragments (the 18th k-step's stay in registers), by ds_read_b128."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'mmla_audio_amd', 'csrc', 'rbs_w1l.hip')
KERNEL = 'rbs_w1l_kernel<64, 76, 32, false, false>'


def _tool():
    spec = importlib.util.spec_from_file_location('lds_lookahead', os.path.join(REPO, 'tools', 'lds_lookahead.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope='module')
def compiled():
    t = _tool()
    text = t.compile_to_asm(SRC)
    meta = t.metadata(text)
    bodies = t.kernel_bodies(text, set(meta))
    names = t.demangle(list(bodies))
    return {names[sym]: (meta[sym], t.analyse(body)) for sym, body in bodies.items()}


def test_one_kernel_within_two_workgroups_per_cu(compiled):
    assert sorted(compiled) == [KERNEL]
    m, _ = compiled[KERNEL]
    print(KERNEL, m)
    assert m['vgpr_count'] <= 256, m['vgpr_count']
    assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0
    assert m['private_segment_fixed_size'] == 0
    assert m['group_segment_fixed_size'] <= 81920, m['group_segment_fixed_size']
    # the rings and parameters of rbs.hip's kernel (45 952 B) + 17 k-steps x (hi + lo) x 1 KB
    assert m['group_segment_fixed_size'] == 45952 + 17 * 2 * 1024


def test_gemm1_reads_x_and_weights_from_lds(compiled):
    """GEMM 1 is the 54-MFMA stretch (18 k-steps x 3; the prologue's, and one per unrolled chunk):
    2 x 18 x fragments + 2 x 17 weight fragments"""
    _, st = compiled[KERNEL]
    gemm1 = [s for s in st if s['mfmas'] == 54]
    assert len(gemm1) == 3
    for s in gemm1:
        assert len(s['reads']) == 2 * 18 + 2 * 17, len(s['reads'])
