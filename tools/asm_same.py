"""Are the kernels of moved or split csrc sources still the same machine code? (gfx950 device compile; no GPU)

    python tools/asm_same.py OTHER_ROOT k_x2.hip=k_x2_irb.hip,k_x2_irw.hip,k_x2_irp.hip,k_x2_front.hip,k_x2_pw.hip \
                                        k_mx.hip=k_mx.hip

OTHER_ROOT is a checkout of the commit to compare against (``git worktree add`` or an unpacked ``git archive``). Each
OLD=NEW[,NEW...] pair compiles OTHER_ROOT's csrc/OLD with that checkout's flags for it and this tree's csrc/NEW files
with theirs (spef_amd/_build.py of either side, ``--cuda-device-only -S``), and compares every kernel of OLD with the
kernel of the same mangled name in the NEW files: the instruction text (comments dropped, local labels renumbered in
order of appearance), the kernel descriptor directives, and the metadata's register counts and segment sizes. Every
kernel of OLD must be in exactly one NEW file, and the NEW files may hold no kernel that OLD has not. Exit status 0
when all pairs are identical. A development aid for refactors: it only diffs.
"""
from __future__ import annotations

import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'spacecraft-pose-estimation-framework_amd'
META = ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')


def build_module(root: str):
    """spef_amd/_build.py of the checkout at ``root`` (its paths and per-file flags are its own)."""
    path = os.path.join(root, PKG, 'spef_amd', '_build.py')
    spec = importlib.util.spec_from_file_location('_build_' + str(abs(hash(root))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, source: str) -> str:
    src = os.path.join(build.CSRC, source)
    flags = [f for f in build._flags(src) if f != '-fPIC']
    r = subprocess.run([build.HIPCC] + flags + ['-x', 'hip', '--cuda-device-only', '-S', src, '-o', '-'],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'hipcc failed on {src}:\n{r.stderr}')
    return r.stdout


def kernels(asm: str) -> dict:
    """-> {mangled kernel name: (instruction lines, descriptor lines, metadata dict)}"""
    names = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', asm, re.M)
    lines = asm.splitlines()
    meta = {}
    for blk in re.split(r'^  - ', asm[asm.find('amdhsa.kernels:'):], flags=re.M)[1:]:
        m = re.search(r'^\s*\.name:\s*(\S+)', blk, re.M)
        if m:
            meta[m.group(1).strip("'\"")] = {
                k: (re.search(r'^\s*\.%s:\s*(\d+)' % k, blk, re.M) or [None, None])[1] for k in META}
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ':'))
        text, labels = [], {}
        for ln in lines[start + 1:]:
            t = ln.split(';')[0].strip()
            if t.startswith('.Lfunc_end'):
                break
            if t:
                text.append(t)
        renum = lambda m: labels.setdefault(m.group(0), f'.L{len(labels)}')   # noqa: E731
        text = [re.sub(r'\.L[A-Za-z_]*\d+(?:_\d+)?', renum, t) for t in text]
        d0 = next(i for i, ln in enumerate(lines) if re.match(r'\s*\.amdhsa_kernel\s+' + re.escape(name) + r'\s*$', ln))
        desc = []
        for ln in lines[d0 + 1:]:
            if '.end_amdhsa_kernel' in ln:
                break
            desc.append(ln.split(';')[0].strip())
        out[name] = (text, desc, meta.get(name, {}))
    return out


def compare(old_root: str, old_src: str, new_srcs: list) -> bool:
    old = kernels(assembly(build_module(old_root), old_src))
    here = build_module(ROOT)
    new, where = {}, {}
    ok = True
    for s in new_srcs:
        for name, k in kernels(assembly(here, s)).items():
            if name in new:
                print(f'  TWICE   {name}: {where[name]} and {s}')
                ok = False
            new[name], where[name] = k, s
    per_file = dict.fromkeys(new_srcs, 0)
    for name, (text, desc, meta) in sorted(old.items()):
        if name not in new:
            print(f'  MISSING {name}')
            ok = False
            continue
        ntext, ndesc, nmeta = new[name]
        diffs = [what for what, a, b in (('text', text, ntext), ('descriptor', desc, ndesc), ('metadata', meta, nmeta))
                 if a != b]
        if diffs:
            first = next((i for i, (a, b) in enumerate(zip(text, ntext)) if a != b), min(len(text), len(ntext)))
            print(f'  DIFFERS {name} ({where[name]}): {", ".join(diffs)}; {len(text)} -> {len(ntext)} instructions, '
                  f'first difference at {first}; metadata {meta} -> {nmeta}')
            ok = False
        else:
            per_file[where[name]] += 1
    for name in sorted(set(new) - set(old)):
        print(f'  NEW     {name} ({where[name]})')
        ok = False
    print(f'{old_src}: {len(old)} kernels; identical: ' + ', '.join(f'{s} {n}' for s, n in per_file.items()) +
          ('' if ok else '  -- NOT the same'))
    return ok


if __name__ == '__main__':
    if len(sys.argv) < 3 or any('=' not in a for a in sys.argv[2:]):
        sys.exit(__doc__)
    results = [compare(sys.argv[1], a.split('=')[0], a.split('=')[1].split(',')) for a in sys.argv[2:]]
    sys.exit(0 if all(results) else 1)
