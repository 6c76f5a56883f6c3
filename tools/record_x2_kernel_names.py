"""Record which kernel the fp16x2 dispatch names at every point of tests/x2_plan_cases.py (no GPU):
    python tools/record_x2_kernel_names.py [--lib PATH] [--out PATH] [--rev COMMIT]

Calls the library's own x2_irb_kernel_name and x2_irb_supported (host functions that never touch the device) through
ctypes, by default on this tree's built library, and writes tests/golden/x2_kernel_names.json: the axes of the grid,
``supported`` per geometry and ``names`` per point (an index into ``kernels``, in the order of x2_plan_cases.points()).
tests/test_x2_plan.py replays it through a host build of csrc/x2_plan.hpp. The fixture was recorded on b4be7ee, the
last commit in which the label, the support check and the launch each walked the tile tables themselves; record it
again only when a change means to alter which kernel runs where, and say so."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import x2_plan_cases as C  # noqa: E402

KERNELS = [None, 'x2_irb_kernel', 'x2_irw_kernel', 'x2_irp_kernel']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd', 'spef_amd', 'lib',
                                                  'libspef_mi355x.so'))
    ap.add_argument('--out', default=C.FIXTURE)
    ap.add_argument('--rev', default=None, help='the commit the library was built from (default: git rev-parse HEAD)')
    args = ap.parse_args()
    lib = ctypes.CDLL(args.lib)
    name = lib._ZN4spef18x2_irb_kernel_nameEiiiibbiiibii   # spef::x2_irb_kernel_name(int x4, bool x2, int x3, bool, int x2)
    name.restype = ctypes.c_char_p
    name.argtypes = [ctypes.c_int] * 4 + [ctypes.c_bool] * 2 + [ctypes.c_int] * 3 + [ctypes.c_bool] + [ctypes.c_int] * 2
    sup = lib._ZN4spef16x2_irb_supportedEiiiibb            # spef::x2_irb_supported(int x4, bool x2)
    sup.restype = ctypes.c_bool
    sup.argtypes = [ctypes.c_int] * 4 + [ctypes.c_bool] * 2
    names = []
    for p in C.points():
        n = name(*p[:4], bool(p[4]), bool(p[5]), *p[6:9], bool(p[9]), p[10], p[11])
        names.append(KERNELS.index(n.decode() if n is not None else None))
    rev = args.rev or subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True,
                                     text=True).stdout.strip()
    doc = {'recorded_at': rev or None, 'geometries': C.GEOMETRIES, 'batches': C.BATCHES, 'maps': C.MAPS,
           'scratch': C.SCRATCH, 'io': C.IO, 'num_cu': C.NUM_CU, 'kernels': KERNELS,
           'supported': [bool(sup(*g[:4], bool(g[4]), bool(g[5]))) for g in C.GEOMETRIES], 'names': names}
    with open(args.out, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print(f'{len(names)} points: ' + ', '.join(f'{k}: {names.count(i)}' for i, k in enumerate(KERNELS)))


if __name__ == '__main__':
    main()
