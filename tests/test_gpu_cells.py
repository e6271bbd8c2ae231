"""GPU tests of the field cells (run with -m gpu on an MI355X): the kernels of csrc/fcpp_cells.hip against the same rule on the host
(fcpp_debug_cells) BIT FOR BIT -- both field offset arrays, status, cuts, dropped and dropped_area, the cells' vertex offsets, x, y, src,
cell_field and area.

One batch of 257 fields per mode is cut on the host once and shared: field j is kind j mod K of tests/cell_cases.py::device_cases -- the
named shapes and their tilted copies, stars of 3 / 63 / 64 / 65 / 256 / 257 / 1024 edges and one of 1025, stars with ponds, every status,
the touching rings and the two fields of 260 rings -- the first K fields at their own cut angle (the named shapes at 0 and 0.5 rad), the
rest at angles that cycle through ANGLES.  The rule takes every field on its own (tests/test_cells_host.py asserts that on the host), so the
batches of 1 / 63 / 65 fields are prefixes of it and their expected arrays prefixes of the host's.  The launcher does not chunk: a launch
takes the whole batch, and 257 fields are 257 workgroups of the 256-lane instance (any field of more than 64 edges selects it).  The
one-wavefront instance runs alone on the kinds of at most 64 edges, to which the over-the-cap fields are added: they are EUNSUPPORTED in
either instance, and the 260 rings of one of them take its ring loops through five rounds of 64 lanes."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import cells as CL
from field_coverage_path_planning_amd import engine as E
from tests import cell_cases as CC
from tests.support import bits as _bits, np_of as _np

pytestmark = pytest.mark.gpu

ANGLES = (0.0, 0.5, 0.3, -1.1, np.pi / 2, 2.5, -0.2)
MODES = (('reflex', CC.REFLEX), ('extrema', CC.EXTREMA))
N_FULL = 257


def full_batch():
    kinds = CC.device_cases()
    own = {name: a for name, _, a in CC.named_cases()}
    names = list(kinds)
    fields = [kinds[names[j % len(names)]] for j in range(N_FULL)]
    angles = [own.get(names[j], 0.3) if j < len(names) else ANGLES[j % len(ANGLES)] for j in range(N_FULL)]
    return names, fields, np.asarray(angles)


@pytest.fixture(scope='module')
def batch():
    return full_batch()


@pytest.fixture(scope='module')
def host(batch):
    """fcpp_debug_cells of the full batch in both modes, computed once and left unchanged"""
    _, fields, angles = batch
    return {name: CC.HostCells(fields, angles, ev) for name, ev in MODES}


def prefix(h, m):
    C, V = int(h.co[m]), int(h.cvo[m])
    return dict(co=h.co[:m + 1], ovo=h.ovo[:C + 1], x=h.x[:V], y=h.y[:V], src=h.src[:V], field=h.field[:C], area=h.area[:C], status=h.status[:m],
                n_cuts=h.n_cuts[:m], dropped=h.dropped[:m], dropped_area=h.dropped_area[:m])


def assert_equal_bits(cs, want):
    assert np.array_equal(_np(cs.cell_offsets), want['co']) and np.array_equal(cs.cell_offsets_host, want['co'])
    assert np.array_equal(_np(cs.status), want['status'])
    assert np.array_equal(_np(cs.n_cuts), want['n_cuts']) and np.array_equal(_np(cs.dropped), want['dropped'])
    assert np.array_equal(_bits(_np(cs.dropped_area)), _bits(want['dropped_area']))
    assert np.array_equal(_np(cs.fields.vert_offsets), want['ovo'])
    assert np.array_equal(_np(cs.fields.ring_offsets), np.arange(len(want['ovo'])))
    assert np.array_equal(_bits(_np(cs.fields.x)), _bits(want['x'])) and np.array_equal(_bits(_np(cs.fields.y)), _bits(want['y']))
    assert np.array_equal(_np(cs.src), want['src'])
    assert np.array_equal(_np(cs.field), want['field'].astype(np.int64))
    assert np.array_equal(_bits(_np(cs.area)), _bits(want['area']))


def test_the_batch_holds_what_it_should(batch, host):
    names, fields, _ = batch
    h = host['reflex']
    st = dict(zip(names, h.status[:len(names)]))
    assert st['star1024'] == 0 and st['star1025'] == CC.EUNSUPPORTED and st['ponds259'] == CC.EUNSUPPORTED and st['tri_ponds259'] == 0
    assert st['touching'] == CC.EUNSUPPORTED and st['nan'] == CC.EINVAL and st['empty'] == CC.EINVAL
    assert len(fields[names.index('tri_ponds259')]) == 260 and len(np.concatenate(fields[names.index('tri_ponds259')])) <= CC.MAX_EDGES
    assert (h.status == 0).sum() > 200 and h.co[-1] > 5000


@pytest.mark.parametrize('mode', [m for m, _ in MODES])
@pytest.mark.parametrize('m', (1, 63, 65, N_FULL))
def test_device_equals_host_bit_for_bit(batch, host, mode, m):
    _, fields, angles = batch
    cs = CL.field_cells(fields[:m], angles[:m], events=mode)
    assert_equal_bits(cs, prefix(host[mode], m))


@pytest.mark.parametrize('mode, ev', MODES)
def test_the_one_wavefront_instance_alone(batch, mode, ev):
    names, fields, angles = batch
    edges = lambda f: sum(len(r) for r in f)
    pick = [j for j in range(len(names)) if edges(fields[j]) <= 64 or edges(fields[j]) > CC.MAX_EDGES]
    assert {'star64', 'star63', 'star3', 'ponds259', 'star1025', 'two_diamonds', 'touching'} <= {names[j] for j in pick}
    assert max(edges(fields[j]) for j in pick if edges(fields[j]) <= CC.MAX_EDGES) == 64
    sub, ang = [fields[j] for j in pick] * 3, np.tile(angles[pick], 3)
    h = CC.HostCells(sub, ang, ev)
    assert_equal_bits(CL.field_cells(sub, ang, events=mode), prefix(h, len(sub)))


@pytest.mark.parametrize('mode, ev', MODES)
def test_the_field_of_259_ponds(mode, ev):
    """260 rings: the second round of the ring loops of the 256-lane instance; the diamond ponds' 1040 edges are over the cap, the
    triangular ponds' 781 under it"""
    tri = CC.ponds_field(259, kind='triangle')
    fields = [tri, CC.ponds_field(259, kind='diamond'), tri[1:] + tri[:1]]          # (the third: the outline is the LAST ring)
    ang = np.array([0.3, 0.0, 0.3])
    h = CC.HostCells(fields, ang, ev)
    assert h.status.tolist() == [0, CC.EUNSUPPORTED, 0] and h.n_cuts[0] == (4 if ev else 5) * 259
    assert h.co[1] == 1 + h.n_cuts[0] - 259 and h.co[3] - h.co[2] == h.co[1]
    assert_equal_bits(CL.field_cells(fields, ang, events=mode), prefix(h, 3))


@pytest.mark.parametrize('mode, ev', MODES)
def test_min_area_drops_the_same_cells(batch, mode, ev):
    _, fields, angles = batch
    m = 65
    h = CC.HostCells(fields[:m], angles[:m], ev, min_area=40.0)
    assert h.dropped.sum() > 100 and h.co[-1] > 100
    assert_equal_bits(CL.field_cells(fields[:m], angles[:m], events=mode, min_area=40.0), prefix(h, m))


def test_scalar_angle_and_packed_fields():
    fields = [CC.YOU, CC.NAMED['holed_square']]
    pf = E.polygon_fields(fields)
    cs = CL.field_cells(pf, 0.0, events='reflex')
    assert _np(cs.cell_offsets).tolist() == [0, 3, 7] and _np(cs.field).tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert _np(cs.angle).tolist() == [0.0, 0.0] and cs.events == 'reflex' and cs.n == 2
    with pytest.raises(ValueError):
        CL.field_cells(pf, 0.0, events='convex')
    with pytest.raises(ValueError):
        CL.field_cells(pf, [0.0, 0.1, 0.2])
