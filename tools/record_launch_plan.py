"""Record the launch plan of every schedule into tests/golden/launch_plan.json (needs the MI355X):
    python tools/record_launch_plan.py [--out PATH]

For each case of tests/launch_plan_cases.py: a synthetic model, the case's options, the entry point once unprofiled and
once between profile_begin and profile_end. Per case the file keeps ``plan`` {kernel key: [launches, bytes, flops]}
(bytes and flops as the profiler prints them: deterministic host arithmetic, no timing), ``shapes`` of the outputs and
``sha256`` of the raw output bytes; once per file the device's compute-unit count (fp16x2 sizes its tiles by it).
Every case runs twice; the hash is kept only where every run gave the same bytes, else it is null, and a plan that
differs between the two runs is an error.

The fixture pins what the scheduler does at the commit it was recorded on: tests/test_gpu_launch_plan.py replays it. Run
this again only when a change means to alter which kernel runs where, and say so."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd'), ROOT):
    sys.path.insert(0, p)
import launch_plan_cases as LP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'launch_plan.json'))
    ap.add_argument('--rev', default=None, help='the commit being recorded (default: git rev-parse HEAD)')
    args = ap.parse_args()
    rev = args.rev or subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True,
                                     text=True).stdout.strip()
    cases = {}
    for cid in LP.CASES:
        plan, shapes, hashes = LP.run_case(cid)
        plan2, shapes2, hashes2 = LP.run_case(cid)
        assert plan == plan2 and shapes == shapes2, f'{cid}: the plan differs between two runs'
        same = len(set(hashes + hashes2)) == 1
        cases[cid] = {'plan': plan, 'shapes': shapes, 'sha256': hashes[0] if same else None}
        print(f'{cid}: {len(plan)} keys, {sum(v[0] for v in plan.values())} launches, '
              f'{"hash " + hashes[0][:12] if same else "outputs differ between runs: null"}', flush=True)
    doc = {'compute_units': LP.compute_units(), 'recorded_at': rev or None, 'cases': cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    nulls = [c for c, v in cases.items() if v['sha256'] is None]
    print(f'{len(cases)} cases, {len(nulls)} without a hash: {nulls}')


if __name__ == '__main__':
    main()
