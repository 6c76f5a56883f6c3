"""Static instruction split of the kernels of one csrc source (gfx950 device compile with the build's flags; no GPU):

    python tools/valu_split.py k_mx.hip [name-filter] [--json]

Per kernel the assembly is cut at its first and its last MFMA (text order): "pro" is what precedes the first one (tile
set-up: addresses, masks, operand loads), "body" what lies between them (the chunk loop, once), "epi" what follows the
last (output addresses, residual, stores). Each part gets the count of VALU instructions (every v_* that is not an
MFMA), SALU instructions (s_* arithmetic / moves / compares: no waits, barriers, branches or scalar loads), branches,
integer multiplies (v_mul_lo / v_mul_hi / 64-bit v_mad) and 64-bit address steps (v_lshl_add_u64, v_lshlrev_b64,
v_add_co / v_addc pairs count as VALU only). Registers and spill counts come from the code object's metadata.
The counts are static: a part with a workgroup-uniform branch (interior / edge set-up) counts both sides.
"""
from __future__ import annotations

import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd'))

from spef_amd import _build  # noqa: E402

PARTS = ('pro', 'body', 'epi')
CLASSES = ('valu', 'salu', 'branch', 'imul', 'addr64')
_NOT_SALU = ('s_waitcnt', 's_nop', 's_barrier', 's_endpgm', 's_sleep', 's_setprio', 's_load', 's_buffer_load',
             's_branch', 's_cbranch', 's_code_end', 's_setpc', 's_swappc', 's_getpc', 's_inst_prefetch', 's_clause')
_IMUL = ('v_mul_lo_', 'v_mul_hi_', 'v_mad_u64_', 'v_mad_i64_')
_ADDR64 = ('v_lshl_add_u64', 'v_lshlrev_b64')


def assembly(source: str) -> str:
    """The gfx950 assembly of csrc/<source>, compiled as _build.py compiles it."""
    src = source if os.path.isabs(source) else os.path.join(_build.CSRC, source)
    flags = [f for f in _build._flags(src) if f != '-fPIC']
    cmd = [_build.HIPCC] + flags + ['-x', 'hip', '--cuda-device-only', '-S', src, '-o', '-']
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'hipcc failed on {src}:\n{r.stderr}')
    return r.stdout


def demangle(names):
    for tool in ('/opt/rocm/llvm/bin/llvm-cxxfilt', 'llvm-cxxfilt', 'c++filt'):
        try:
            r = subprocess.run([tool], input='\n'.join(names), capture_output=True, text=True)
        except OSError:
            continue
        if r.returncode == 0:
            out = r.stdout.splitlines()
            if len(out) == len(names):
                return dict(zip(names, out))
    return {n: n for n in names}


def short(name: str) -> str:
    """spef::mx_irb_kernel<16, 96, ...>(void const*, ...) -> mx_irb_kernel<16,96,...>"""
    if name.startswith('_Z'):   # no demangler for this name: the kernel's own name and its integer / bool arguments
        ident = ''
        rest = name[3:] if name.startswith('_ZN') else name[2:]
        while rest and rest[0].isdigit():   # <length><identifier> components of the nested name
            n = re.match(r'\d+', rest).group(0)
            ident, rest = rest[len(n):len(n) + int(n)], rest[len(n) + int(n):]
        targs = ''
        if rest.startswith('I'):
            vals = re.match(r'I((?:L[a-z]n?\d+E)+)E', rest)
            if vals:
                targs = '<' + ','.join(v.replace('n', '-') for v in re.findall(r'L[a-z](n?\d+)E', vals.group(1))) + '>'
        return ident + targs
    m = re.match(r'(?:void )?(?:spef::)?(?:\(anonymous namespace\)::)?([A-Za-z_0-9]+(?:<.*>)?)\(', name)
    s = m.group(1) if m else name
    return s.replace(', ', ',').replace('true', '1').replace('false', '0').replace('(bool)', '')


def classify(mn: str):
    """-> the set of classes one mnemonic counts in ('mfma' for a matrix instruction)."""
    if mn.startswith(('v_mfma', 'v_smfmac')):
        return ('mfma',)
    if mn.startswith('v_'):
        c = ['valu']
        if mn.startswith(_IMUL):
            c.append('imul')
        if mn.startswith(_ADDR64):
            c.append('addr64')
        return tuple(c)
    if mn.startswith(('s_branch', 's_cbranch')):
        return ('branch',)
    if mn.startswith('s_') and not mn.startswith(_NOT_SALU):
        return ('salu',)
    return ()


def split(asm: str) -> dict:
    """-> {short kernel name: {'pro' | 'body' | 'epi': {class: count}, 'mfma': n, 'vgpr': .., 'sgpr': ..,
    'vgpr_spill': .., 'sgpr_spill': ..}} for every kernel (amdhsa_kernel) of the assembly text."""
    kernels = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', asm, re.M)
    dem = demangle(kernels)
    lines = asm.splitlines()
    start = {}
    for i, ln in enumerate(lines):
        lab = ln.split(':', 1)[0] if ':' in ln and not ln[:1].isspace() else None
        if lab in dem and lab not in start:
            start[lab] = i
    meta = {}
    for blk in re.split(r'^  - ', asm[asm.find('amdhsa.kernels:'):], flags=re.M)[1:]:
        m = re.search(r'^\s*\.name:\s*(\S+)', blk, re.M)
        if not m:
            continue
        d = {}
        for key in ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count'):
            v = re.search(r'^\s*\.%s:\s*(\d+)' % key, blk, re.M)
            d[key] = int(v.group(1)) if v else None
        meta[m.group(1).strip("'\"")] = d
    out = {}
    for k in kernels:
        if k not in start:
            continue
        ops = []
        for ln in lines[start[k] + 1:]:
            t = ln.split(';')[0].strip()
            if not t or t.startswith('.') or t.endswith(':'):
                if t.startswith('.Lfunc_end'):
                    break
                continue
            mn = t.split()[0]
            ops.append(classify(mn))
        mf = [i for i, c in enumerate(ops) if c == ('mfma',)]
        rec = {p: dict.fromkeys(CLASSES, 0) for p in PARTS}
        rec['mfma'] = len(mf)
        first, last = (mf[0], mf[-1]) if mf else (len(ops), len(ops))
        for i, cs in enumerate(ops):
            part = 'pro' if i < first else ('body' if i <= last else 'epi')
            for c in cs:
                if c != 'mfma':
                    rec[part][c] += 1
        md = meta.get(k, {})
        rec.update(vgpr=md.get('vgpr_count'), sgpr=md.get('sgpr_count'), vgpr_spill=md.get('vgpr_spill_count'),
                   sgpr_spill=md.get('sgpr_spill_count'))
        out[short(dem[k])] = rec
    return out


def table(res: dict, flt: str = '') -> str:
    rows = ['kernel | pro valu (imul, addr64) salu br | body valu salu br | epi valu (imul, addr64) salu br | set-up '
            'valu | mfma | vgpr sgpr | spills v s']
    for name, r in sorted(res.items()):
        if flt not in name:
            continue
        p, b, e = r['pro'], r['body'], r['epi']
        rows.append(f"{name} | {p['valu']} ({p['imul']}, {p['addr64']}) {p['salu']} {p['branch']} | "
                    f"{b['valu']} {b['salu']} {b['branch']} | {e['valu']} ({e['imul']}, {e['addr64']}) {e['salu']} "
                    f"{e['branch']} | {p['valu'] + e['valu']} | {r['mfma']} | {r['vgpr']} {r['sgpr']} | "
                    f"{r['vgpr_spill']} {r['sgpr_spill']}")
    return '\n'.join(rows)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if not args:
        sys.exit(__doc__)
    res = split(assembly(args[0]))
    if '--json' in sys.argv:
        flt = args[1] if len(args) > 1 else ''
        print(json.dumps({k: v for k, v in res.items() if flt in k}))
    else:
        print(table(res, args[1] if len(args) > 1 else ''))
