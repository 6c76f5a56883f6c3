"""The grid over which the fp16x2 launch plan (csrc/x2_plan.hpp) is pinned: shared by tools/record_x2_kernel_names.py
(which records tests/golden/x2_kernel_names.json from a built library) and tests/test_x2_plan.py (which replays it
through a host build of the plan alone)."""
import itertools
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'x2_kernel_names.json')

# (cin, hidden, cout, stride, expand, residual): the geometries of the primary tile table (MobileNet-V2 blocks 1,
# 2, 3, 4, 5-6, 7, 8-10, 11, 12-13, 14, 15-16, 17), then two that no table has
GEOMETRIES = [
    (32, 32, 16, 1, 0, 0), (16, 96, 24, 2, 1, 0), (24, 144, 24, 1, 1, 1), (24, 144, 32, 2, 1, 0),
    (32, 192, 32, 1, 1, 1), (32, 192, 64, 2, 1, 0), (64, 384, 64, 1, 1, 1), (64, 384, 96, 1, 1, 0),
    (96, 576, 96, 1, 1, 1), (96, 576, 160, 2, 1, 0), (160, 960, 160, 1, 1, 1), (160, 960, 320, 1, 1, 0),
    (32, 192, 32, 1, 1, 0), (320, 1920, 320, 1, 1, 1),
]
N_SUPPORTED = 12
BATCHES = [1, 2, 64]
MAPS = [(3, 5), (8, 8), (8, 12), (16, 16), (15, 24), (30, 48), (32, 32), (60, 96), (64, 64), (128, 128)]   # OH, OW
SCRATCH = [0, 1]
IO = [0, 1, 2, 3]
NUM_CU = [64, 256, 304]


def points():
    """Every grid point (cin, hid, cout, stride, expand, res, B, OH, OW, scratch, io, num_cu), geometry slowest."""
    for g, b, (oh, ow), sc, io, cu in itertools.product(GEOMETRIES, BATCHES, MAPS, SCRATCH, IO, NUM_CU):
        yield g + (b, oh, ow, sc, io, cu)


def build_dump(out_dir: str) -> str:
    """tools/x2_plan_dump.cpp + csrc/x2_plan.hpp with the host compiler: no HIP headers, no library."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    exe = os.path.join(out_dir, 'x2_plan_dump')
    csrc = os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd', 'csrc')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', f'-I{csrc}',
                        os.path.join(ROOT, 'tools', 'x2_plan_dump.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_dump(exe: str, pts) -> list:
    """-> per point {'known', 'found', 'kind', 'TH', 'TW', 'NW', 'WCO', 'P', 'name'} (name None when no kernel)."""
    text = ''.join(' '.join(str(int(v)) for v in p) + '\n' for p in pts)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    out = []
    for line in r.stdout.splitlines():
        f = line.split()
        d = dict(zip(('known', 'found', 'kind', 'TH', 'TW', 'NW', 'WCO', 'P'), map(int, f[:8])))
        d['name'] = None if f[8] == '-' else f[8]
        out.append(d)
    return out
