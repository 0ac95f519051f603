"""tools/lds_lookahead.py on a hand-written assembly fragment: the MFMA distance between each
ds_read_b128 and the s_waitcnt lgkmcnt(N) that covers it, the kernel metadata it reports, reads
that feed no MFMA left out, and the conservative rule while a scalar memory read is outstanding.
Then on rbs.hip and odu.hip as they compile here (hipcc, no GPU): the register budgets that keep
the kernels' workgroups per CU, no spills, unchanged LDS sizes, and >= 3 MFMAs of lookahead in
the loops that carry the operand pipeline."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ASM = """
\t.text
\t.globl\tk1
\t.type\tk1,@function
k1:                                     ; @k1
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\tds_read_b128 v[0:3], v40
\tds_read_b128 v[4:7], v40 offset:64
\tds_read_b128 v[8:11], v41
\tds_read_b128 v[12:15], v41 offset:64
\ts_waitcnt lgkmcnt(3)
\tv_mfma_f32_32x32x16_f16 v[16:31], v[32:35], v[0:3], v[16:31]
\ts_waitcnt lgkmcnt(2)
\tv_mfma_f32_32x32x16_f16 v[16:31], v[36:39], v[4:7], v[16:31]
\tv_mfma_f32_32x32x16_f16 v[16:31], v[36:39], v[0:3], v[16:31]
\tds_read_b128 v[0:3], v42
\ts_waitcnt lgkmcnt(2)
\tv_mfma_f32_32x32x16_f16 v[16:31], v[32:35], v[8:11], v[16:31]
\ts_waitcnt lgkmcnt(0)
\tv_mfma_f32_32x32x16_f16 v[16:31], v[36:39], v[0:3], v[16:31]
\ts_barrier
\tds_read_b128 v[44:47], v43
\ts_waitcnt lgkmcnt(0)
\tv_add_f32_e32 v44, v44, v45
\ts_endpgm
.Lfunc_end0:
\t.size\tk1, .Lfunc_end0-k1
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .args:
      - .name:           a
        .size:           8
    .group_segment_fixed_size: 4096
    .name:           k1
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .sgpr_spill_count: 0
    .symbol:         k1.kd
    .vgpr_count:     48
    .vgpr_spill_count: 0
...
\t.end_amdgpu_metadata
"""


def _tool():
    spec = importlib.util.spec_from_file_location('lds_lookahead', os.path.join(REPO, 'tools', 'lds_lookahead.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_metadata_and_distances():
    t = _tool()
    meta = t.metadata(ASM)
    assert meta == {'k1': {'group_segment_fixed_size': 4096, 'private_segment_fixed_size': 0,
                           'sgpr_spill_count': 0, 'vgpr_count': 48, 'vgpr_spill_count': 0}}
    body = t.kernel_bodies(ASM, {'k1'})['k1']
    st = t.analyse(body)
    assert len(st) == 1                       # the read after the barrier feeds a VALU op: left out
    # v[0:3]: 0 MFMAs before lgkmcnt(3); v[4:7]: 1; v[8:11] and v[12:15] (never used by an MFMA:
    # left out) are covered by the lgkmcnt(2) after the third MFMA -> 3; the re-read v[0:3]: 1
    assert st[0]['mfmas'] == 5
    assert sorted(st[0]['reads']) == [0, 1, 1, 3]
    text = t.report(ASM, 'fragment')
    assert 'vgpr_count 48 spills 0 scratch 0 B  LDS 4096 B' in text
    assert 'lookahead min 0 median 1 max 3' in text


def test_outstanding_scalar_read_only_completes_at_zero():
    t = _tool()
    body = [(1, 'k:'), (2, 'ds_read_b128 v[0:3], v9'), (3, 's_load_dword s0, s[4:5], 0x0'),
            (4, 'v_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[8:11], v[16:31]'),
            (5, 's_waitcnt lgkmcnt(1)'),
            (6, 'v_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[8:11], v[16:31]'),
            (7, 's_waitcnt lgkmcnt(0)'),
            (8, 'v_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[0:3], v[16:31]')]
    st = t.analyse(body)
    assert [s['reads'] for s in st] == [[2]]


# ---- the shipped kernels, compiled here (no GPU): register budgets and the pipelined loops ---------
# kernel -> the VGPR cap that keeps its workgroups per CU (rbs: 3 and 2; odu with one strip per
# workgroup: 4, 3, 3, 3, with two: 2 and 2)
# odu_kernel<H, W, CIN, C, TW, POOL, NS (strips per workgroup), DBUF, NW, MINW, LA, LB>
ODU_BLOCK_7_TWO_STRIPS = 'odu_kernel<32, 38, 64, 128, 2, true, 2, true, 4, 2, 1, 1>'
ODU_BLOCKS_8_9_TWO_STRIPS = 'odu_kernel<16, 19, 128, 128, 4, false, 2, false, 4, 2, 1, 1>'
BUDGET = {
    'rbs_kernel<128, 151, 16, true, true>': 168,
    'rbs_kernel<64, 76, 32, false, false>': 256,
    'odu_kernel<64, 76, 32, 64, 2, true, 1, false, 4, 4, 0, 0>': 128,
    'odu_kernel<32, 38, 64, 64, 4, false, 1, false, 4, 3, 1, 1>': 168,
    'odu_kernel<32, 38, 64, 128, 2, true, 1, true, 4, 2, 1, 1>': 168,
    'odu_kernel<16, 19, 128, 128, 4, false, 1, true, 4, 2, 1, 1>': 168,
    ODU_BLOCK_7_TWO_STRIPS: 256,
    ODU_BLOCKS_8_9_TWO_STRIPS: 256,
}
LDS = {
    'rbs_kernel<128, 151, 16, true, true>': 51072,
    'rbs_kernel<64, 76, 32, false, false>': 45952,
    'odu_kernel<64, 76, 32, 64, 2, true, 1, false, 4, 4, 0, 0>': 38592,
    'odu_kernel<32, 38, 64, 64, 4, false, 1, false, 4, 3, 1, 1>': 40320,
    'odu_kernel<32, 38, 64, 128, 2, true, 1, true, 4, 2, 1, 1>': 39168,
    'odu_kernel<16, 19, 128, 128, 4, false, 1, true, 4, 2, 1, 1>': 41472,
    ODU_BLOCK_7_TWO_STRIPS: 78336,
    ODU_BLOCKS_8_9_TWO_STRIPS: 80512,
}


@pytest.fixture(scope='module')
def compiled():
    t = _tool()
    out = {}
    for src in t.DEFAULT:
        text = t.compile_to_asm(src)
        meta = t.metadata(text)
        bodies = t.kernel_bodies(text, set(meta))
        names = t.demangle(list(bodies))
        for sym, body in bodies.items():
            out[names[sym]] = (meta[sym], t.analyse(body))
    return out


def test_register_budgets_no_spills_same_lds(compiled):
    assert sorted(compiled) == sorted(BUDGET)
    for name, cap in BUDGET.items():
        m, _ = compiled[name]
        assert m['vgpr_count'] <= cap, (name, m['vgpr_count'])
        assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0, name
        assert m['private_segment_fixed_size'] == 0, name
        assert m['group_segment_fixed_size'] == LDS[name], name


def test_two_strip_instantiations_fit_two_workgroups_per_cu(compiled):
    """exactly two instantiations run two strips per workgroup, blocks 7 and 8-9 (the ones
    odu_two_strips names); each keeps two workgroups per CU: at most 256 VGPRs (two waves per SIMD),
    no spills, no scratch, at most 81 920 B of LDS (half of a CU's 160 KB)"""
    two = {n: m for n, (m, _) in compiled.items()
           if n.startswith('odu_kernel<') and n.split(', ')[6] == '2'}
    assert sorted(two) == sorted([ODU_BLOCK_7_TWO_STRIPS, ODU_BLOCKS_8_9_TWO_STRIPS])
    for name, m in two.items():
        print(name, m)
        assert m['vgpr_count'] <= 256, (name, m['vgpr_count'])
        assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0, name
        assert m['private_segment_fixed_size'] == 0, name
        assert m['group_segment_fixed_size'] <= 81920, (name, m['group_segment_fixed_size'])


def test_pipelined_loops_read_three_mfmas_ahead(compiled):
    """every converted loop: all reads but the first groups' (which have nothing to hide under) are
    issued >= 3 MFMAs before their wait; block 1's GEMM 2 is its kernel's last MFMA stretch"""
    for name, (m, st) in compiled.items():
        if name.startswith('odu_kernel') and name.endswith('1, 1>'):
            loops = [s for s in st if s['mfmas'] >= 48]
            assert len(loops) == 2, name          # GEMM a's chunk body, GEMM b's
        elif name.startswith('rbs_kernel<128'):
            loops = [st[-1]]
            assert loops[0]['mfmas'] == 27 and len(loops[0]['reads']) == 32   # 24 + 3 shortcut MFMAs
        else:
            continue
        for s in loops:
            r = sorted(s['reads'])
            assert r[len(r) // 2] >= 3, (name, r)
            assert sum(1 for v in r if v < 3) <= 8, (name, r)
