"""GPU tests of plan_polygon_cells(..., tour=True) (run with -m gpu on an MI355X): the cell tour closing the cell chain on the U, the H and
the rectangle with two diamond ponds of tests/cell_cases.py, at the settings of tests/test_gpu_cell_plan.py (W = 2, R = 2, spacing 0.5,
cut angle 0, track angles {0, pi / 2}, 10 m of turn cost per swath), with headland loops and a mission.

The tour only reorders and turns round what the router already offers: the cells' swath samples are the same multiset with and without it,
every cell's driven order is a permutation of its swaths, the tour's cost is the cells' connector lengths plus its joints (the same
lengths in another order of addition: 1e-9 relative, the project's length tolerance), it never exceeds the stored order's cost, and the
mission drives the cells in the tour's order.  Which fields fall strictly is an observation; the strict case is the host line scene.

MEASURED on an MI355X (printed by test_tour_closes_the_chain; Dubins, the exit pose south-west of the field, 8 starts), tour cost against
the stored order at each cell's own winner: the U (3 cells) 161.123 m against 224.483 m, the H (5 cells) 218.682 m against 261.038 m, the
rectangle with two diamond ponds (5 cells) 375.139 m against 496.139 m; 44 of the 71 swaths are driven the other way."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import cells as CL
from tests.cell_cases import AITCH, NAMED, YOU
from tests.support import np_of as _np

pytestmark = pytest.mark.gpu

W, R, SPACING = 2.0, 2.0, 0.5
ANGLES = (0.0, np.pi / 2)
TURN_COST = 10.0
FIELDS = [YOU, AITCH, NAMED['two_diamonds']]
EXIT = [(-5.0, -8.0, np.pi)] * 3
ENTRY = [(-5.0, -5.0, 0.0)] * 3


@pytest.fixture(scope='module')
def plans():
    """the three fields planned with and without the tour, computed once and left unchanged"""
    kw = dict(turn_cost=TURN_COST, headland_paths=True, mission='headland_first', entry=ENTRY, exit=EXIT)
    return (CL.plan_polygon_cells(FIELDS, W, R, SPACING, ANGLES, 0.0, tour=True, **kw), CL.plan_polygon_cells(FIELDS, W, R, SPACING, ANGLES, 0.0, **kw),
            CL.plan_polygon_cells(FIELDS, W, R, SPACING, ANGLES, 0.0, **kw))


def test_tour_closes_the_chain(plans):
    plan, bare, _ = plans
    t = plan.tour
    coff = t.cell_offsets_host
    assert bare.tour is None and _np(t.status).tolist() == [0, 0, 0]
    cost, stored, joints = _np(t.cost), _np(t.stored_cost), _np(t.joint_length)
    for f, name in enumerate(('you', 'aitch', 'two_diamonds')):
        print('%s: %d cells, tour cost %.3f m, stored %.3f m, joints %.3f m, winner %d, sweeps %d'
              % (name, coff[f + 1] - coff[f], cost[f], stored[f], joints[f], _np(t.winner)[f], _np(t.sweeps)[f]))
    assert np.isfinite(cost).all() and (cost <= stored).all()
    order, node = _np(t.order), _np(t.node)
    soff = plan.swaths.offsets_host
    transit = _np(plan.paths.transit_length)
    assert _np(plan.paths.status).tolist() == [0] * int(coff[-1])
    for f in range(3):
        c0, c1 = int(coff[f]), int(coff[f + 1])
        assert sorted(order[c0:c1].tolist()) == list(range(c1 - c0))
        kept = [c for c in range(c0, c1) if soff[c + 1] > soff[c]]
        assert all(node[c] >= 0 for c in kept) and all(node[c] == -1 for c in range(c0, c1) if c not in kept)
        assert _np(t.skipped)[f] == c1 - c0 - len(kept)
        total = transit[c0:c1].sum() + joints[f]
        assert abs(total - cost[f]) <= 1e-9 * max(1.0, abs(cost[f])), (f, total, cost[f])
    # every cell's driven order is a permutation of its swaths
    driven = _np(plan.route.order)
    for c in range(int(coff[-1])):
        m = int(soff[c + 1] - soff[c])
        assert sorted((driven[soff[c]:soff[c + 1]] >> 1).tolist()) == list(range(m))


def test_the_work_is_the_same(plans):
    """Every swath is driven once in both plans, over its whole length, with the same samples counted from the end it is entered at.  (As
    POINTS the samples of a swath driven the other way are the same multiset only where its length is a multiple of the spacing: a
    swath is sampled every `spacing` metres from its start.  The distances from the driven start are the same multiset always, and so
    is the multiset of points of the swaths whose direction did not change.)"""
    plan, bare, _ = plans
    soff = plan.swaths.offsets_host
    assert np.array_equal(soff, bare.swaths.offsets_host)
    a, b = _np(plan.swaths.a), _np(plan.swaths.b)
    assert np.array_equal(a, _np(bare.swaths.a)) and np.array_equal(b, _np(bare.swaths.b))

    def by_swath(p):
        """global swath -> (direction, its samples (k, 2))"""
        off, leg, part = p.paths.offsets_host, _np(p.paths.leg), _np(p.paths.part)
        xy = np.stack([_np(p.paths.x), _np(p.paths.y)], axis=1)
        order = _np(p.route.order)
        out = {}
        for c in range(len(soff) - 1):
            sl = slice(int(off[c]), int(off[c + 1]))
            for k in range(int(soff[c + 1] - soff[c])):
                o = int(order[soff[c] + k])
                pts = xy[sl][(part[sl] == 0) & (leg[sl] == 2 * k + 1)]
                assert int(soff[c]) + (o >> 1) not in out
                out[int(soff[c]) + (o >> 1)] = (o & 1, pts)
        return out

    with_tour, without = by_swath(plan), by_swath(bare)
    assert sorted(with_tour) == sorted(without) == list(range(int(soff[-1]))) and len(with_tour) > 0
    assert sum(len(p) for _, p in with_tour.values()) == int((plan.paths.part == 0).sum()) == int((bare.paths.part == 0).sum())
    turned = 0
    for g in with_tour:
        (d1, p1), (d0, p0) = with_tour[g], without[g]
        start1, start0 = (b[g] if d1 else a[g]), (b[g] if d0 else a[g])
        s1, s0 = np.hypot(*(p1 - start1).T), np.hypot(*(p0 - start0).T)
        assert s1.shape == s0.shape and len(s1) >= 1
        assert np.abs(s1 - s0).max() <= 1e-9 * 100.0, g          # the same samples along the swath, from the end it is entered at
        assert np.abs(p1[0] - start1).max() <= 1e-9 * 100.0 and np.abs(p1[-1] - (a[g] if d1 else b[g])).max() <= 1e-9 * 100.0
        if d1 == d0:
            assert np.array_equal(p1, p0), g
        turned += d1 != d0
    print('%d of %d swaths are driven the other way under the tour' % (turned, len(with_tour)))


def test_mission_drives_the_cells_in_tour_order(plans):
    plan, _, _ = plans
    m, t = plan.mission, plan.tour
    assert _np(m.status).tolist() == [0, 0, 0]
    n_loops = int(plan.headland_paths.offsets.numel()) - 1
    off = plan.paths.offsets_host
    item_path, item_set, ioff = _np(m.item_path), _np(m.item_set), _np(m.item_offsets)
    coff, order = t.cell_offsets_host, _np(t.order)
    for f in range(3):
        items = slice(int(ioff[f]), int(ioff[f + 1]))
        cells_driven = (item_path[items][item_set[items] == 1] - n_loops).tolist()
        want = [int(coff[f] + c) for c in order[coff[f]:coff[f + 1]] if off[coff[f] + c + 1] > off[coff[f] + c]]
        assert cells_driven == want and len(want) > 0, (f, cells_driven, want)
    assert int(((m.part == 0) & (m.src_set == 1)).sum()) == int((plan.paths.part == 0).sum())


def test_without_the_tour_nothing_changes(plans):
    _, bare, again = plans
    assert np.array_equal(_np(bare.paths.x).view(np.uint64), _np(again.paths.x).view(np.uint64))
    assert np.array_equal(_np(bare.route.order), _np(again.route.order)) and np.array_equal(_np(bare.mission.item_path), _np(again.mission.item_path))
    # the stored order of the cells, as before the tour existed
    n_loops = int(bare.headland_paths.offsets.numel()) - 1
    cells_driven = _np(bare.mission.item_path)[_np(bare.mission.item_set) == 1] - n_loops
    assert cells_driven.tolist() == sorted(cells_driven.tolist())
