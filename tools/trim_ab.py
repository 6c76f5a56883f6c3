"""Per-kernel A/B of two values of one tuning option (default SPEF_OPT_TRIM) on the fp16mx headline workload, in ONE
process and on one engine (GPU box, development tool): python tools/trim_ab.py 1 3 [passes [option id]] -> one JSON
line per pass and value {kernel: us per step}, the values alternating, then per kernel the range of each value and
whether every pass of the last value is below every pass of the first. One process: both settings see the same clocks,
buffers and warm-up. E.g. SPEF_OPT_X2_STAGE: python tools/trim_ab.py 0 1 4 10."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd')]

import numpy as np
import torch

from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.engine import Engine
from spef_amd.weights import synthetic_state_dict

vals = [int(sys.argv[1]), int(sys.argv[2])]
passes = int(sys.argv[3]) if len(sys.argv) > 3 else 4
opt = int(sys.argv[4]) if len(sys.argv) > 4 else L.OPT_TRIM
B, S, steps = int(os.environ.get('B', 64)), int(os.environ.get('S', 512)), int(os.environ.get('STEPS', 20))
eng = Engine(Bl.pack(synthetic_state_dict(mobilenet_v2(), seed=1001), dtype='fp16mx'), 'cuda:0')
fr = torch.from_numpy(np.random.Generator(np.random.PCG64(0)).integers(0, 256, (B, S, S, 3), dtype=np.uint8)).cuda()
res = {v: [] for v in vals}
for p in range(-1, passes):   # pass -1: both settings once, unrecorded (code objects loaded, the clock out of idle)
    for v in (vals if p % 2 == 0 else vals[::-1]):
        eng.set_option(opt, v)
        for _ in range(5):
            eng.forward(fr)
        torch.cuda.synchronize()
        eng.profile_begin()
        for _ in range(steps):
            eng.forward(fr)
        prof = eng.profile_end()
        t = {k: round(x[1] / steps * 1e3, 2) for k, x in prof.items()}
        if p < 0:
            continue
        res[v].append(t)
        print(f'opt{opt}={v}', json.dumps(t))
a, b = vals
for k in res[a][0]:
    ra, rb = [t[k] for t in res[a]], [t[k] for t in res[b]]
    print(f'{k}: {a}: {min(ra):.2f}-{max(ra):.2f}  {b}: {min(rb):.2f}-{max(rb):.2f}  '
          f'mean {sum(rb) / len(rb) - sum(ra) / len(ra):+.2f} us  ordered {max(rb) < min(ra)}')
