"""fcpp_cells_counts and fcpp_cells_fill on guarded buffers (tests/guarded.py): every output element is written and nothing beside it, the
inputs keep their bits, every pointer is only naturally aligned (the float64 and int64 arrays at 8 mod 16, the int32 ones at 4 mod 8),
and outputs passed as NULL are accepted.  Once per kernel instance: the kinds of tests/cell_cases.py::device_cases of at most 64 edges
(one wavefront a field) and all of them (four).  The expected values are the host twin's; fields of every status stand between fields
with cells, so a field that wrote outside its own ranges would show in a neighbour's."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import engine as E
from tests import cell_cases as CC
from tests.guarded import Arena
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu


def _batch(instance):
    kinds = CC.device_cases()
    own = {name: a for name, _, a in CC.named_cases()}
    names = [k for k in kinds if instance == 'four_wavefronts' or sum(len(r) for r in kinds[k]) <= 64]
    return [kinds[k] for k in names], np.asarray([own.get(k, 0.3) for k in names])


@pytest.mark.parametrize('events', (CC.REFLEX, CC.EXTREMA))
@pytest.mark.parametrize('instance', ('one_wavefront', 'four_wavefronts'))
def test_counts_and_fill_on_guarded_buffers(instance, events):
    import torch
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    fields, ang = _batch(instance)
    min_area = 1e-3
    h = CC.HostCells(fields, ang, events, min_area=min_area)
    ro, vo, x, y = pack(fields)
    n, C, V = h.n, int(h.co[-1]), int(h.cvo[-1])
    assert (h.status == 0).sum() > 20 and (h.status != 0).sum() >= 5 and C > n

    def inputs():
        return Arena().input('ring_offsets', ro).input('vert_offsets', vo).input('x', x).input('y', y).input('angle', ang)

    def head(a):
        return (ctx.handle, n, a.ptr('ring_offsets'), len(vo) - 1, a.ptr('vert_offsets'), len(x), a.ptr('x'), a.ptr('y'), a.ptr('angle'), events, min_area)

    ctx.bind_stream()
    a = inputs().output('cell_offsets', np.int64, n + 1).output('cvert_offsets', np.int64, n + 1)
    for name in ('status', 'n_cuts', 'dropped'):
        a.output(name, np.int32, n)
    a.output('dropped_area', np.float64, n).build(dev)
    co_h, cvo_h = np.full(n + 1, -7, np.int64), np.full(n + 1, -7, np.int64)
    rc = ctx.lib.fcpp_cells_counts(*head(a), a.ptr('cell_offsets'), co_h.ctypes.data, a.ptr('cvert_offsets'), cvo_h.ctypes.data, a.ptr('status'),
                                   a.ptr('n_cuts'), a.ptr('dropped'), a.ptr('dropped_area'))
    assert rc == 0, ctx.lib.fcpp_last_error()
    a.check({'cell_offsets': h.co, 'cvert_offsets': h.cvo, 'status': h.status, 'n_cuts': h.n_cuts, 'dropped': h.dropped,
             'dropped_area': h.dropped_area})
    assert np.array_equal(co_h, h.co) and np.array_equal(cvo_h, h.cvo)

    # every output NULL; then the offsets alone
    b = inputs().build(dev)
    assert ctx.lib.fcpp_cells_counts(*head(b), None, None, None, None, None, None, None, None) == 0, ctx.lib.fcpp_last_error()
    b.check({})
    b = inputs().output('cvert_offsets', np.int64, n + 1).build(dev)
    assert ctx.lib.fcpp_cells_counts(*head(b), None, None, b.ptr('cvert_offsets'), None, None, None, None, None) == 0, ctx.lib.fcpp_last_error()
    b.check({'cvert_offsets': h.cvo})

    c = inputs().input('cell_offsets', h.co).input('cvert_offsets', h.cvo)
    c.output('out_vert_offsets', np.int64, C + 1).output('out_x', np.float64, V).output('out_y', np.float64, V).output('out_src', np.int32, V)
    c.output('cell_field', np.int32, C).output('area', np.float64, C).build(dev)
    rc = ctx.lib.fcpp_cells_fill(*head(c), c.ptr('cell_offsets'), c.ptr('cvert_offsets'), C, V, c.ptr('out_vert_offsets'), c.ptr('out_x'),
                                 c.ptr('out_y'), c.ptr('out_src'), c.ptr('cell_field'), c.ptr('area'))
    assert rc == 0, ctx.lib.fcpp_last_error()
    c.check({'out_vert_offsets': h.ovo, 'out_x': h.x, 'out_y': h.y, 'out_src': h.src, 'cell_field': h.field, 'area': h.area})

    d = inputs().input('cell_offsets', h.co).input('cvert_offsets', h.cvo).output('out_y', np.float64, V).build(dev)
    rc = ctx.lib.fcpp_cells_fill(*head(d), d.ptr('cell_offsets'), d.ptr('cvert_offsets'), C, V, None, None, d.ptr('out_y'), None, None, None)
    assert rc == 0, ctx.lib.fcpp_last_error()
    d.check({'out_y': h.y})
