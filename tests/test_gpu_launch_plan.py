"""GPU: the launch plan of every schedule equals the recorded one (tests/golden/launch_plan.json, written by
tools/record_launch_plan.py). Per case -- tests/launch_plan_cases.py: every schedule family under every schedule option
at the smallest shapes that take each branch of the schedulers -- the profiler's kernel keys and, per key, the launch
count and the algorithmic bytes and flops must match exactly: they are integers and ``%.1f`` strings of deterministic
host arithmetic, so a block that moved to another kernel, bit-identical or not, shows here. Where the fixture holds a
hash (the recorder got the same output bytes from every run) the output bytes must hash the same."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_plan_cases as LP  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_plan.json')) as _f:
    FIXTURE = json.load(_f)


@pytest.mark.parametrize('case_id', sorted(LP.CASES))
def test_launch_plan(case_id):
    cus = LP.compute_units()
    if cus != FIXTURE['compute_units']:
        pytest.skip(f"the plan was recorded on {FIXTURE['compute_units']} compute units, this device has {cus} "
                    '(fp16x2 sizes its tiles by the count)')
    assert set(FIXTURE['cases']) == set(LP.CASES)
    want = FIXTURE['cases'][case_id]
    if case_id.startswith('int8-'):   # integer arithmetic end to end: every int8 case carries a hash
        assert want['sha256']
    plan, shapes, hashes = LP.run_case(case_id)
    assert sorted(plan) == sorted(want['plan'])
    for key, rec in want['plan'].items():
        assert plan[key] == rec, key
    assert shapes == want['shapes']
    if want['sha256'] is not None:
        assert hashes == [want['sha256']] * len(hashes)
