"""The fp16x2 / fp16mx launch plan (csrc/x2_plan.hpp: which kernel, tile and hidden split a block runs on) on the host:
tools/x2_plan_dump.cpp compiles the plan file alone with the host compiler, and its output over the grid of
x2_plan_cases.py must name the kernel that tests/golden/x2_kernel_names.json holds -- recorded from the library's own
x2_irb_kernel_name / x2_irb_supported at b4be7ee, when label, support check and launch each walked the tables
themselves (tools/record_x2_kernel_names.py) -- and must hit the tile choices the source comments derive by hand."""
import json

import pytest

import x2_plan_cases as C

B3, B8, B15, B17 = C.GEOMETRIES[2], C.GEOMETRIES[6], C.GEOMETRIES[10], C.GEOMETRIES[11]


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    exe = C.build_dump(str(tmp_path_factory.mktemp('x2_plan')))
    return lambda pts: C.run_dump(exe, pts)


@pytest.fixture(scope='module')
def grid(dump):
    pts = list(C.points())
    return pts, dump(pts)


def test_grid_is_the_recorded_one():
    with open(C.FIXTURE) as f:
        fx = json.load(f)
    assert [tuple(g) for g in fx['geometries']] == C.GEOMETRIES and fx['batches'] == C.BATCHES
    assert [tuple(m) for m in fx['maps']] == C.MAPS and fx['scratch'] == C.SCRATCH and fx['io'] == C.IO
    assert fx['num_cu'] == C.NUM_CU and len(fx['names']) == len(list(C.points())) == 14 * 3 * 10 * 2 * 4 * 3
    assert fx['supported'] == [True] * C.N_SUPPORTED + [False] * (len(C.GEOMETRIES) - C.N_SUPPORTED)
    assert len({tuple(g) for g in fx['geometries'][:C.N_SUPPORTED]}) == 12   # every row of the primary table


def test_kernel_names_equal_the_recorded_dispatch(grid):
    pts, plans = grid
    with open(C.FIXTURE) as f:
        fx = json.load(f)
    assert len(plans) == len(pts)
    bad = [(p, pl['name'], fx['kernels'][i]) for p, pl, i in zip(pts, plans, fx['names']) if pl['name'] != fx['kernels'][i]]
    assert not bad, f'{len(bad)} of {len(pts)} points differ, first: {bad[:5]}'
    seen = {pl['name'] for pl in plans}
    assert seen == {None, 'x2_irb_kernel', 'x2_irw_kernel', 'x2_irp_kernel'}   # the grid reaches every family


def test_supported_equals_the_recorded_dispatch(grid):
    """x2_irb_supported is the plan's `known`: per geometry, whatever the map, the batch, the I/O or the device."""
    pts, plans = grid
    with open(C.FIXTURE) as f:
        fx = json.load(f)
    sup = {tuple(g): s for g, s in zip(fx['geometries'], fx['supported'])}
    for p, pl in zip(pts, plans):
        assert bool(pl['known']) == sup[p[:6]], p
        assert pl['found'] == (pl['name'] is not None) and (pl['known'] or not pl['found']), p


def _one(dump, g, B, oh, ow, scratch, io, cu):
    return dump([g + (B, oh, ow, scratch, io, cu)])[0]


def _row(pl):
    return (pl['kind'], pl['TH'], pl['TW'], pl['NW'], pl['WCO'], pl['P'])


def test_block3_takes_16x16_tiles_only_where_they_divide_the_map(dump):
    for io in C.IO:
        assert _row(_one(dump, B3, 64, 64, 64, 1, io, 256)) == (0, 16, 16, 8, 1, 1)
        assert _row(_one(dump, B3, 64, 60, 96, 1, io, 256)) == (0, 8, 16, 4, 1, 1)


def test_small_maps_split_the_hidden_dimension(dump):
    # 8 x 12 map at B = 64: 128 tiles of 8 x 8, two parts each = 256 workgroups on 256 CUs
    assert _row(_one(dump, B15, 64, 8, 12, 1, 0, 256)) == (1, 8, 8, 8, 1, 2)
    assert _row(_one(dump, B17, 64, 8, 12, 1, 0, 256)) == (2, 8, 8, 8, 2, 2)
    # without scratch, or with fp16 I/O, the primary row; fp16 I/O has no kernel there (kind 5 is not the slab kernel)
    for g in (B15, B17):
        assert _row(_one(dump, g, 64, 8, 12, 0, 0, 256)) == (5, 8, 8, 8, 1, 1)
        for io in (1, 2, 3):
            pl = _one(dump, g, 64, 8, 12, 1, io, 256)
            assert _row(pl) == (5, 8, 8, 8, 1, 1) and not pl['found'] and pl['name'] is None


def test_16x16_maps_at_b64_fill_the_device_without_a_split(dump):
    # 256 tiles are not fewer than 256 CUs; on 304 CUs they are, but 512 parts exceed 304
    for cu in (256, 304):
        pl = _one(dump, B15, 64, 16, 16, 1, 0, cu)
        assert _row(pl) == (5, 8, 8, 8, 1, 1) and pl['name'] == 'x2_irp_kernel'


def test_role_split_blocks_have_no_fp16_io_kernel(dump):
    assert _one(dump, B8, 64, 32, 32, 1, 0, 256)['name'] == 'x2_irw_kernel'
    pl = _one(dump, B8, 64, 32, 32, 1, 1, 256)
    assert pl['known'] and not pl['found'] and pl['name'] is None
