"""CPU: tools/valu_split.py on csrc/k_mx.hip (one gfx950 device compile, no GPU): every kernel splits into set-up,
chunk body and epilogue around its MFMAs, and each lean mx_irb_kernel instantiation (SPEF_OPT_TRIM bit 1, the last
template argument) has strictly fewer static set-up VALU instructions than the instantiation it replaces in the same
build. No absolute threshold: compilers differ; the measured counts are in DESIGN.md section 3."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def split():
    spec = importlib.util.spec_from_file_location('valu_split', os.path.join(ROOT, 'tools', 'valu_split.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod._build.HIPCC):
        pytest.fail('hipcc is required: ' + mod._build.HIPCC)
    return mod.split(mod.assembly('k_mx.hip'))


def test_every_kernel_has_three_parts_and_an_mfma(split):
    assert any(k.startswith('front_mx_kernel<') for k in split), sorted(split)
    for name, r in split.items():
        assert r['mfma'] >= 1, name
        for part in ('pro', 'body', 'epi'):
            assert r[part]['valu'] > 0, (name, part)
        assert r['vgpr_spill'] == 0, name


def test_lean_set_up_is_smaller(split):
    pairs = 0
    for name, old in split.items():
        m = re.fullmatch(r'mx_irb_kernel<(.*),0>', name)
        if not m:
            continue
        new = split[f'mx_irb_kernel<{m.group(1)},1>']
        pairs += 1
        su_old, su_new = old['pro']['valu'] + old['epi']['valu'], new['pro']['valu'] + new['epi']['valu']
        print(name, 'set-up valu', su_old, '->', su_new, 'imul', old['pro']['imul'] + old['epi']['imul'], '->',
              new['pro']['imul'] + new['epi']['imul'])
        assert su_new < su_old, (name, su_old, su_new)
        assert new['pro']['valu'] < old['pro']['valu'] and new['epi']['valu'] < old['epi']['valu'], name
        assert new['body']['valu'] <= old['body']['valu'], name   # the chunk loop is not what changed
    assert pairs == 3
