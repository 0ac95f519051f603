"""rbs_tp.hip as it compiles here (hipcc, no GPU): exactly one kernel, block 1's strip kernel with the
clips' last strips paired, within the budget of three workgroups per CU -- at most 168 VGPRs (three waves
per SIMD), no spills, no scratch, at most 54 613 B of LDS (a third of a CU's 160 KB; the rings, parameters
and GEMM 2's weights are 51 072 B, as in rbs.hip's kernel)."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'mmla_audio_amd', 'csrc', 'rbs_tp.hip')
KERNEL = 'rbs_tp_kernel<128, 151, 16, true, true>'


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
    return {names[sym]: meta[sym] for sym in bodies}


def test_one_kernel_within_three_workgroups_per_cu(compiled):
    assert sorted(compiled) == [KERNEL]
    m = compiled[KERNEL]
    print(KERNEL, m)
    assert m['vgpr_count'] <= 168, m['vgpr_count']
    assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0
    assert m['private_segment_fixed_size'] == 0
    assert m['group_segment_fixed_size'] <= 54613, m['group_segment_fixed_size']
    assert m['group_segment_fixed_size'] == 51072
