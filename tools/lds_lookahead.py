"""LDS operand lookahead of the conv kernels' GEMM loops, read off the compiled code (no GPU needed):

    python tools/lds_lookahead.py [--label NAME] [-D MACRO=V ...] [FILE ...]

FILE is a .hip source (compiled for gfx950 with the library's flags) or an assembly file (.s);
default: mmla_audio_amd/csrc/rbs.hip and odu.hip.  For every kernel it prints vgpr_count, spill
count, scratch and LDS bytes, and for every stretch of straight-line code that holds MFMAs fed from
LDS (stretches end at s_barrier and at labels; the unrolled GEMM loops are one stretch each) the
instruction distance of each ds_read_b128 that feeds an MFMA: how many MFMAs are issued between the
read and the s_waitcnt lgkmcnt(N) that covers it.  0 means the matrix pipe idles for the whole LDS
round trip unless another wave of the SIMD fills it; 3 is one (tap, k-step) group of the 3xFP16
kernels, 96 cycles of 32x32x16 MFMAs.

The LGKM counter model: LDS operations return in issue order, so `lgkmcnt(N)` completes all but the
youngest N outstanding ones; while a scalar memory read is outstanding (they may return out of order)
only lgkmcnt(0) is taken to complete anything.  This is an instruction-distance report and nothing
else.
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'mmla_audio_amd', 'csrc')
DEFAULT = [os.path.join(CSRC, 'rbs.hip'), os.path.join(CSRC, 'odu.hip')]

_LABEL = re.compile(r'^([.\w$]+):')
_LGKM = re.compile(r'lgkmcnt\((\d+)\)')
_VREG = re.compile(r'v\[(\d+):(\d+)\]|v(\d+)')
_META = re.compile(r'^\s+\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|'
                   r'group_segment_fixed_size):\s*(\S+)')


def compile_to_asm(src, defines=(), hipcc=None):
    hipcc = hipcc or os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    out = tempfile.NamedTemporaryFile(suffix='.s', delete=False).name
    cmd = [hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S',
           '-I', CSRC, '-I', os.path.join(REPO, 'include')] + [f'-D{d}' for d in defines] + [src, '-o', out]
    try:
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        with open(out) as f:
            return f.read()
    finally:
        if os.path.exists(out):
            os.unlink(out)


def metadata(text):
    """-> {kernel symbol: {vgpr_count, vgpr_spill_count, ...}} from the .amdgpu_metadata block"""
    out, cur = {}, {}
    for line in text.splitlines():
        m = _META.match(line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == 'name':                      # an argument's .name comes first and is overwritten
            cur['name'] = v
        else:
            cur[k] = int(v)
        if k == 'vgpr_spill_count':          # the last per-kernel key in emission order
            if 'name' in cur:
                out[cur['name']] = {x: y for x, y in cur.items() if x != 'name'}
            cur = {}
    return out


def _regs(tok):
    m = _VREG.fullmatch(tok.strip())
    if not m:
        return None
    if m.group(3) is not None:
        return (int(m.group(3)), int(m.group(3)))
    return (int(m.group(1)), int(m.group(2)))


def _operands(ins):
    parts = ins.split(None, 1)
    return [t.strip() for t in parts[1].split(',')] if len(parts) > 1 else []


def kernel_bodies(text, names):
    """-> {symbol: [(line number, instruction or 'label:')]} for the given kernel symbols"""
    lines = text.splitlines()
    out = {}
    i = 0
    while i < len(lines):
        m = _LABEL.match(lines[i])
        if m and m.group(1) in names:
            name, body = m.group(1), []
            i += 1
            while i < len(lines) and not lines[i].startswith('.Lfunc_end'):
                s = lines[i].split(';', 1)[0].strip()
                if s and not s.startswith('.') or _LABEL.match(s or ''):
                    body.append((i + 1, s))
                i += 1
            out[name] = body
        i += 1
    return out


def analyse(body):
    """-> list of stretches {first, last, mfmas, reads: [lookahead, ...], unfed}"""
    stretches = []
    cur = {'first': body[0][0] if body else 0, 'last': 0, 'mfmas': 0, 'reads': [], 'unfed': 0}
    pending = []          # outstanding LGKM operations, oldest first
    nmfma = 0             # MFMAs issued so far in the kernel

    def writes(ins):
        ops = _operands(ins)
        return _regs(ops[0]) if ops else None

    for k, (ln, ins) in enumerate(body):
        op = ins.split(None, 1)[0] if ins else ''
        if _LABEL.match(ins) or op == 's_barrier':
            if cur['mfmas'] or cur['reads']:
                cur['last'] = ln
                stretches.append(cur)
            cur = {'first': ln, 'last': ln, 'mfmas': 0, 'reads': [], 'unfed': 0}
            continue
        if op.startswith('v_mfma'):
            nmfma += 1
            cur['mfmas'] += 1
        elif op == 'ds_read_b128':
            dst = writes(ins)
            # feeds an MFMA if the next reader of exactly these registers, before they are written
            # again by another LDS read, is an MFMA's A or B operand
            fed = False
            for j in range(k + 1, min(len(body), k + 600)):
                jin = body[j][1]
                if jin.startswith('v_mfma'):
                    ops = _operands(jin)
                    if len(ops) >= 3 and (_regs(ops[1]) == dst or _regs(ops[2]) == dst):
                        fed = True
                        break
                elif jin.startswith('ds_read') and writes(jin) == dst:
                    break
            pending.append(('lds', fed, nmfma, cur))
        elif op.startswith('ds_'):
            pending.append(('lds', False, nmfma, cur))
        elif op.startswith('s_load') or op.startswith('s_buffer_load') or op == 's_memtime':
            pending.append(('smem', False, nmfma, cur))
        elif op == 's_waitcnt':
            m = _LGKM.search(ins)
            if m:
                n = int(m.group(1))
                if n > 0 and any(p[0] == 'smem' for p in pending):
                    continue
                done, pending = pending[:len(pending) - n] if n else pending, pending[len(pending) - n:] if n else []
                for kind, fed, at, st in done:
                    if fed:
                        st['reads'].append(nmfma - at)
    if cur['mfmas'] or cur['reads']:
        cur['last'] = body[-1][0] if body else 0
        stretches.append(cur)
    return [s for s in stretches if s['reads']]


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if not tool and os.path.exists('/opt/rocm/llvm/bin/llvm-cxxfilt'):
        tool = '/opt/rocm/llvm/bin/llvm-cxxfilt'
    if not tool:
        return {n: n for n in names}
    r = subprocess.run([tool] + list(names), stdout=subprocess.PIPE, text=True)
    got = r.stdout.strip().splitlines()
    if len(got) != len(names):
        return {n: n for n in names}
    short = {}
    for n, d in zip(names, got):
        d = d.replace('(anonymous namespace)::', '').replace('void ', '')
        short[n] = re.sub(r'\(.*\)$', '', d)
    return short


def report(text, title):
    meta = metadata(text)
    bodies = kernel_bodies(text, set(meta))
    names = demangle(list(bodies))
    out = [f'== {title}']
    for sym, body in bodies.items():
        m = meta[sym]
        out.append(f'{names[sym]}: vgpr_count {m.get("vgpr_count")} spills {m.get("vgpr_spill_count")} '
                   f'scratch {m.get("private_segment_fixed_size")} B  LDS {m.get("group_segment_fixed_size")} B')
        for s in analyse(body):
            r = s['reads']
            hist = ' '.join(f'{v}:{r.count(v)}' for v in sorted(set(r)))
            out.append(f'  lines {s["first"]:>5}-{s["last"]:<5} {s["mfmas"]:>3} MFMAs  {len(r):>3} ds_read_b128 -> MFMA  '
                       f'lookahead min {min(r)} median {statistics.median(r):g} max {max(r)}  [{hist}]')
    return '\n'.join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('files', nargs='*', default=DEFAULT)
    ap.add_argument('-D', dest='defines', action='append', default=[], help='macro for .hip inputs')
    ap.add_argument('--label', default=None, help='a name for this build in the report header')
    a = ap.parse_args(argv)
    for f in a.files:
        text = open(f).read() if f.endswith('.s') else compile_to_asm(f, a.defines)
        title = os.path.basename(f) + (f' ({a.label})' if a.label else '') + \
            (' ' + ' '.join('-D' + d for d in a.defines) if a.defines else '')
        print(report(text, title))
    return 0


if __name__ == '__main__':
    sys.exit(main())
