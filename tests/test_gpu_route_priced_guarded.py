"""The priced transit block through the guarded arena (tests/guarded.py; run with -m gpu on an MI355X): fcpp_route_transit_priced on slots
carved out of ONE uint8 CUDA tensor, and its host twin on a numpy arena -- 256 bytes of 0xA5 in front of and behind every slot, T and K
pre-filled with 0x5A, every pointer only naturally aligned.  T is OUT ONLY: every entry of every block must be written, from the pre-fill,
with the bits the host twin gives on ordinary arrays; nothing beside the blocks; nothing at all for a field over the cap; K_dev = NULL
accepted.  The test inspects memory afterwards; nothing in it provokes a fault."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from tests.guarded import Arena
from tests.support import Gpu
from tests.test_clearance_host import INSET_SQUARE, PENALTY
from tests.test_field_paths_clear_host import ALL_CLEAR
from tests.test_gpu_route_priced import NINE, NINE_REGION
from tests.test_route_host import HOLED_SQUARE, cut_with_angle, t_offsets
from tests.test_route_priced_host import W, host_transit_priced, strip
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu():
    g = Gpu()
    g.ctx.bind_stream()
    return g


def call(gpu, where, cut, regions, radius, mode, slots):
    """declare the inputs and `slots` (name -> (dtype, count, written)), build, call -> the arena"""
    soff = cut['offsets']
    toff = t_offsets(soff)
    ro, vo, x, y = pack(regions)
    A = Arena()
    for name, a in (('soff', soff), ('ax', cut['ax']), ('ay', cut['ay']), ('bx', cut['bx']), ('by', cut['by']), ('angle', cut['angle']), ('toff', toff),
                    ('ro', ro), ('vo', vo), ('x', x), ('y', y)):
        A.input(name, a)
    for name, (dt, count, written) in slots.items():
        A.output(name, dt, count, written=written)
    A.build(gpu.dev if where == 'device' else None)
    head = (len(soff) - 1, A.ptr('soff'))
    tail = (int(soff[-1]), A.ptr('ax'), A.ptr('ay'), A.ptr('bx'), A.ptr('by'), A.ptr('angle'), float(radius), mode, A.ptr('toff'))
    rest = (int(toff[-1]), A.ptr('ro'), len(vo) - 1, A.ptr('vo'), len(x), A.ptr('x'), A.ptr('y'), PENALTY, A.ptr('T'), A.ptr('K'))
    if where == 'device':
        rc = gpu.lib.fcpp_route_transit_priced(gpu.h, *head, soff.ctypes.data, *tail, toff.ctypes.data, *rest)
    else:
        rc = gpu.lib.fcpp_debug_route_transit_priced(*head, *tail, *rest)
    assert rc == L.OK, gpu.lib.fcpp_last_error()
    return A


@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
@pytest.mark.parametrize('with_k', [True, False], ids=['K', 'K_null'])
@pytest.mark.parametrize('where', ['device', 'host'])
def test_every_entry_of_every_block_is_written_and_nothing_beside(gpu, mode, with_k, where):
    works = [INSET_SQUARE, strip(513), NINE, strip(1), [(0, 0), (10, 0), (10, 1), (0, 1)], strip(3)]
    regions = [HOLED_SQUARE, ALL_CLEAR, NINE_REGION, ALL_CLEAR, ALL_CLEAR, []]
    cut = cut_with_angle(works, 0.0, W)
    assert np.diff(cut['offsets']).tolist() == [14, 513, 9, 1, 0, 3]
    T, K, toff = host_transit_priced(cut, regions, 3.0, mode)
    assert toff.tolist() == [0, 784, 784, 1108, 1112, 1112, 1148] and not np.isnan(T).any()
    assert (K == -1).any() and (K == 0).any() and ((K > 0).any() or mode == 0)
    slots = {'T': (np.float64, T.size, True)}
    if with_k:
        slots['K'] = (np.int8, K.size, True)
    A = call(gpu, where, cut, regions, 3.0, mode, slots)
    A.check({'T': T, 'K': K} if with_k else {'T': T})


@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
@pytest.mark.parametrize('where', ['device', 'host'])
def test_nothing_at_all_for_a_field_over_the_cap(gpu, mode, where):
    cut = cut_with_angle([strip(513)], 0.0, W)
    assert t_offsets(cut['offsets']).tolist() == [0, 0]
    A = call(gpu, where, cut, [ALL_CLEAR], 3.0, mode, {'T': (np.float64, 64, False), 'K': (np.int8, 64, False)})
    A.check({})
