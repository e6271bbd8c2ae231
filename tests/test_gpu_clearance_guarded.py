"""The connector clearance through the guarded arena (tests/guarded.py; run with -m gpu on an MI355X): fcpp_conn_clear and
fcpp_route_transit_clear on slots carved out of ONE uint8 CUDA tensor, and their host twins on a numpy arena -- 256 bytes of 0xA5 around
every slot, outputs pre-filled with 0x5A, every pointer only naturally aligned.  After each call the guards are intact, the inputs have the
bits that were put in, and every output element has the bits the host twin gives on ordinary arrays (none of them the pre-fill pattern, so
an element that was never written cannot pass).  Outputs passed as NULL have no slot: the rest is written as in the full call.

T is in / out: with penalty 0 it is an input slot that must keep its bits; with a penalty it is an output slot that is loaded with the
plain blocks before the call (fcpp_memcpy_h2d on the device, a view on the host)."""
import ctypes as C

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from tests.guarded import Arena
from tests.support import Gpu
from tests.test_clearance_host import PENALTY, host_clear, host_solve, host_transit_clear
from tests.test_gpu_clearance import FIVE, REGIONS, WORKS, random_pairs
from tests.test_route_host import cut_with_angle, host_transit
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu

R_ELEM, R_TRANSIT, N_PATHS = 4.0, 6.0, 65
CONN_OUTS = (('crossings', np.int32), ('inside', np.int8), ('first_s', np.float64), ('field_status', np.int32))
CONN_SUBSETS = [tuple(k for k, _ in CONN_OUTS), ('inside',), ('first_s',), ('crossings', 'field_status')]


@pytest.fixture
def gpu():
    g = Gpu()
    g.ctx.bind_stream()
    return g


def conn_case(mode):
    """65 solved paths without an unsolved one and without a bad field: no NaN among the expected values (bit equality is value equality)"""
    frm, to = random_pairs(11 + mode, N_PATHS)
    fields = [FIVE[0], FIVE[2], FIVE[4]]
    pair_field = (np.arange(N_PATHS) * 7) % 4 - 1
    word, seg, _ = host_solve(frm, to, R_ELEM, mode)
    want = host_clear(mode, frm, R_ELEM, word, seg, pair_field, fields)
    want = {k: np.ascontiguousarray(want[k]) for k, _ in CONN_OUTS}
    assert not np.isnan(want['first_s']).any() and (want['crossings'] > 0).any() and np.isinf(want['first_s']).any()
    return frm, word, seg, pair_field.astype(np.int64), pack(fields), want


def conn_arena(case, outs, device):
    frm, word, seg, pair_field, (ro, vo, x, y), want = case
    A = Arena()
    for name, a in (('fx', frm[:, 0]), ('fy', frm[:, 1]), ('fh', frm[:, 2]), ('word', word), ('seg', seg.reshape(-1)), ('pair_field', pair_field),
                    ('ro', ro), ('vo', vo), ('x', x), ('y', y)):
        A.input(name, a)
    for k, dt in CONN_OUTS:
        if k in outs:
            A.output(k, dt, want[k].size)
    A.build(device)
    args = (A.ptr('fx'), A.ptr('fy'), A.ptr('fh'), R_ELEM, A.ptr('word'), A.ptr('seg'), A.ptr('pair_field'), len(ro) - 1, A.ptr('ro'), len(vo) - 1,
            A.ptr('vo'), len(x), A.ptr('x'), A.ptr('y'), *[A.ptr(k) for k, _ in CONN_OUTS])
    return A, args


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('where', ['device', 'host'])
def test_conn_clear_stays_in_bounds(gpu, mode, where):
    case = conn_case(mode)
    want = case[-1]
    for outs in CONN_SUBSETS:
        A, args = conn_arena(case, outs, gpu.dev if where == 'device' else None)
        rc = gpu.lib.fcpp_conn_clear(gpu.h, mode, N_PATHS, *args) if where == 'device' else gpu.lib.fcpp_debug_conn_clear(mode, N_PATHS, *args)
        assert rc == L.OK, gpu.lib.fcpp_last_error()
        A.check({k: want[k] for k in outs})


@pytest.fixture(scope='module')
def transit_case():
    cut = cut_with_angle(WORKS, 0.0, 4.0)
    per_mode = {}
    for mode in (0, 1):
        T0, toff = host_transit(cut, R_TRANSIT, mode)
        Tp = T0.copy()
        B = host_transit_clear(cut, REGIONS, Tp, toff, R_TRANSIT, mode, PENALTY)
        per_mode[mode] = (T0, Tp, B, toff)
    return cut, per_mode


def transit_on_an_arena(gpu, cut, regions, per_mode, mode, penalty, where):
    T0, Tp, B, toff = per_mode[mode]
    soff = cut['offsets']
    ro, vo, x, y = pack(regions)
    A = Arena()
    for name, a in (('soff', soff), ('ax', cut['ax']), ('ay', cut['ay']), ('bx', cut['bx']), ('by', cut['by']), ('angle', cut['angle']), ('toff', toff),
                    ('ro', ro), ('vo', vo), ('x', x), ('y', y)):
        A.input(name, a)
    if penalty:
        A.output('T', np.float64, T0.size)
    else:
        A.input('T', T0)
    A.output('B', np.uint8, B.size)
    A.build(gpu.dev if where == 'device' else None)
    if penalty and where == 'device':
        assert gpu.lib.fcpp_memcpy_h2d(gpu.h, A.ptr('T'), C.c_void_p(T0.ctypes.data), T0.nbytes) == L.OK
        assert gpu.lib.fcpp_ctx_synchronize(gpu.h) == L.OK
    elif penalty:
        A.view('T')[:] = T0
    n, nt, tt = len(soff) - 1, int(soff[-1]), int(toff[-1])
    tail = (tt, A.ptr('ro'), len(vo) - 1, A.ptr('vo'), len(x), A.ptr('x'), A.ptr('y'), float(penalty), A.ptr('T'), A.ptr('B'))
    head = (A.ptr('ax'), A.ptr('ay'), A.ptr('bx'), A.ptr('by'), A.ptr('angle'), R_TRANSIT, mode, A.ptr('toff'))
    if where == 'device':
        rc = gpu.lib.fcpp_route_transit_clear(gpu.h, n, A.ptr('soff'), soff.ctypes.data, nt, *head, toff.ctypes.data, *tail)
    else:
        rc = gpu.lib.fcpp_debug_route_transit_clear(n, A.ptr('soff'), nt, *head, *tail)
    assert rc == L.OK, gpu.lib.fcpp_last_error()
    A.check({'T': Tp, 'B': B} if penalty else {'B': B})


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('penalty', [0.0, PENALTY])
@pytest.mark.parametrize('where', ['device', 'host'])
def test_route_transit_clear_stays_in_bounds(gpu, transit_case, mode, penalty, where):
    cut, per_mode = transit_case
    transit_on_an_arena(gpu, cut, REGIONS, per_mode, mode, penalty, where)


@pytest.mark.parametrize('mode', [0, 1])
def test_region_of_259_rings_stays_in_bounds(gpu, mode):
    """the new shape class, a region of more rings than the transit kernel has threads (tests/test_gpu_clearance.py), once per mode"""
    from tests.test_gpu_clearance import many_ring_regions
    from tests.test_clearance_host import many_ring_work
    cut = cut_with_angle([many_ring_work()] * 4, 0.0, 4.0)
    T0, toff = host_transit(cut, R_TRANSIT, mode)
    Tp = T0.copy()
    B = host_transit_clear(cut, many_ring_regions(), Tp, toff, R_TRANSIT, mode, PENALTY)
    transit_on_an_arena(gpu, cut, many_ring_regions(), {mode: (T0, Tp, B, toff)}, mode, PENALTY, 'device')
