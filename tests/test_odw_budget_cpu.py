"""odw.hip as it compiles here (hipcc, no GPU): every shipped instantiation keeps two workgroups per
CU -- at most 256 VGPRs (two waves per SIMD), no spills, no scratch, at most 81 920 B of LDS (half of
a CU's 160 KB)."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'mmla_audio_amd', 'csrc', 'odw.hip')


def _tool():
    spec = importlib.util.spec_from_file_location('lds_lookahead', os.path.join(REPO, 'tools', 'lds_lookahead.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope='module')
def kernels():
    t = _tool()
    text = t.compile_to_asm(SRC)
    meta = t.metadata(text)
    names = t.demangle(list(meta))
    return {names[sym]: m for sym, m in meta.items()}


def test_every_instantiation_fits_two_workgroups_per_cu(kernels):
    assert kernels and all(k.startswith('odw_kernel<') for k in kernels), sorted(kernels)
    for name, m in kernels.items():
        print(name, m)
        assert m['vgpr_count'] <= 256, (name, m['vgpr_count'])
        assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0, name
        assert m['private_segment_fixed_size'] == 0, name
        assert m['group_segment_fixed_size'] <= 81920, (name, m['group_segment_fixed_size'])
