"""The clear field paths through the guarded arena (tests/guarded.py; run with -m gpu on an MI355X): fcpp_field_path_counts_clear and
fcpp_field_path_fill_clear on slots carved out of ONE uint8 CUDA tensor, and their host twin on a numpy arena -- 256 bytes of 0xA5 in front
of and behind every slot, outputs pre-filled with 0x5A, every pointer only naturally aligned.  n = 65 and n = 1, both modes, each optional
output NULL in turn.  After each call the guards are intact -- nothing is written outside the n, 2 n_total + n and total_samples ranges --
the inputs have the bits that were put in, and every output element has the bits the host twin gives on ordinary arrays.  The test
inspects memory afterwards; nothing in it provokes a fault."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.guarded import Arena
from tests.support import Gpu
from tests.test_field_paths_clear_host import ENTRY, EXIT, FIELD_OUTS, REGION_DUBINS, REGION_RS, SLOT_OUTS, batch_of_65, host_paths_clear
from tests.test_field_paths_host import SAMPLE_KEYS, SAMPLE_TYPES
from tests.test_route_host import HOLED_SQUARE, R, cut_with_angle
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu

SPACING = 0.5
COUNT_OUTS = (('offsets', np.int64), ('leg_offsets', np.int64), ('work', np.float64), ('transit', np.float64), ('status', np.int32)) + \
    tuple((k, t) for k, t, _ in SLOT_OUTS) + FIELD_OUTS
REQUIRED = ('offsets', 'leg_offsets')
OPTIONAL = tuple(k for k, _ in COUNT_OUTS if k not in REQUIRED)
COUNT_SUBSETS = [tuple(k for k, _ in COUNT_OUTS)] + [tuple(k for k, _ in COUNT_OUTS if k != drop) for drop in OPTIONAL]
FILL_SUBSETS = [SAMPLE_KEYS] + [tuple(k for k in SAMPLE_KEYS if k != drop) for drop in SAMPLE_KEYS]


@pytest.fixture
def gpu():
    g = Gpu()
    g.ctx.bind_stream()
    return g


def case(mode, n):
    """-> inputs (name -> array), sizes, the host twin's result on ordinary arrays: no failed field, so no NaN among the expected values"""
    if n == 1:
        cut, regions, order = cut_with_angle([HOLED_SQUARE], 0.0, 4.0), [REGION_RS if mode else REGION_DUBINS], None
        entry, exit = ENTRY[None].copy(), EXIT[None].copy()
    else:
        cut, regions, order, entry, exit = batch_of_65()
    want = host_paths_clear(cut, regions, mode=mode, order=order, entry=entry, exit=exit)
    assert not want['status'].any() and (want['leg_rank'] < 0).any() and (mode == 1 or (want['leg_rank'] > 0).any())
    ro, vo, rx, ry = pack(regions)
    inputs = dict(soff=cut['offsets'], ax=cut['ax'], ay=cut['ay'], bx=cut['bx'], by=cut['by'], length=cut['length'], angle=cut['angle'],
                  ro=ro, vo=vo, rx=rx, ry=ry)
    if order is not None:
        inputs['order'] = np.ascontiguousarray(order, dtype=np.int32)
    for name, pose in (('e', entry), ('x', exit)):
        for k, c in enumerate('xyh'):
            inputs[name + c] = np.ascontiguousarray(pose[:, k])
    return inputs, (len(cut['offsets']) - 1, int(cut['offsets'][-1]), len(vo) - 1, len(rx)), want


def head(A, n, nt, n_rings, n_verts, mode):
    return (n, A.ptr('soff'), nt, A.ptr('ax'), A.ptr('ay'), A.ptr('bx'), A.ptr('by'), A.ptr('length'), A.ptr('angle'), A.ptr('order'), R, mode, SPACING,
            A.ptr('ex'), A.ptr('ey'), A.ptr('eh'), A.ptr('xx'), A.ptr('xy'), A.ptr('xh'), A.ptr('ro'), n_rings, A.ptr('vo'), n_verts, A.ptr('rx'), A.ptr('ry'))


def arena(inputs, extra=()):
    A = Arena()
    for k, a in list(inputs.items()) + list(extra):
        A.input(k, a)
    return A


@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
@pytest.mark.parametrize('n', [65, 1])
def test_device_entries_stay_in_bounds(gpu, mode, n):
    inputs, (nf, nt, n_rings, n_verts), want = case(mode, n)
    for outs in COUNT_SUBSETS:
        A = arena(inputs)
        for k, dt in COUNT_OUTS:
            if k in outs:
                A.output(k, dt, want[k].size)
        A.build(gpu.dev)
        off_h = np.full(nf + 1, -1, np.int64)
        hd = head(A, nf, nt, n_rings, n_verts, mode)
        rc = gpu.lib.fcpp_field_path_counts_clear(gpu.h, hd[0], hd[1], E._host_ptr(inputs['soff']), *hd[2:], A.ptr('offsets'), E._host_ptr(off_h),
                                                  *[A.ptr(k) for k, _ in COUNT_OUTS[1:]])
        assert rc == L.OK, gpu.lib.fcpp_last_error()
        A.check({k: want[k] for k in outs})
        assert np.array_equal(off_h, want['offsets'])
    for outs in FILL_SUBSETS:
        A = arena(inputs, [('leg_offsets', want['leg_offsets'])])
        for k in SAMPLE_KEYS:
            if k in outs:
                A.output(k, SAMPLE_TYPES[k], want['total'])
        A.build(gpu.dev)
        hd = head(A, nf, nt, n_rings, n_verts, mode)
        rc = gpu.lib.fcpp_field_path_fill_clear(gpu.h, hd[0], hd[1], None, *hd[2:], A.ptr('leg_offsets'), want['total'], *[A.ptr(k) for k in SAMPLE_KEYS])
        assert rc == L.OK, gpu.lib.fcpp_last_error()
        A.check({k: want[k] for k in outs})


@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
@pytest.mark.parametrize('n', [65, 1])
def test_host_twin_stays_in_bounds(mode, n):
    lib = L.load()
    inputs, (nf, nt, n_rings, n_verts), want = case(mode, n)
    all_outs = tuple(k for k, _ in COUNT_OUTS) + SAMPLE_KEYS
    for outs in [all_outs] + [tuple(k for k in all_outs if k != drop) for drop in all_outs]:
        A = arena(inputs)
        for k, dt in COUNT_OUTS:
            if k in outs:
                A.output(k, dt, want[k].size)
        for k in SAMPLE_KEYS:
            if k in outs:
                A.output(k, SAMPLE_TYPES[k], want['total'])
        A.build(None)
        rc = lib.fcpp_debug_field_paths_clear(*head(A, nf, nt, n_rings, n_verts, mode), *[A.ptr(k) for k, _ in COUNT_OUTS], want['total'],
                                              *[A.ptr(k) for k in SAMPLE_KEYS])
        assert rc == L.OK, lib.fcpp_last_error()
        A.check({k: want[k] for k in outs})
