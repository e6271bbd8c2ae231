"""GPU tests of plan_polygon_cells (run with -m gpu on an MI355X): the polygon chain with an angle per CELL on one U-shaped field -- two
12 x 60 m legs on a 72 x 12 m bar -- at W = 2, R = 2, spacing 0.5, cut angle 0, track angles {0, pi / 2}, 10 m of turn cost per swath.

The point of the cells is the swath count: at ONE angle per field either the legs (angle 0) or the bar (pi / 2) is cut into stubs; with
the work area split at the bar's upper side, the legs are driven along y and the bar along x.  The test computes both sides -- the cells'
summed swath count and what plan_polygon_fields gives the same field at its single best angle -- and asserts the inequality, no figure.
No coverage threshold is asserted either: adjacent cells driven at different angles leave wedges at their seams, which no headland pass
covers; the report shows them, and the counts are only checked against each other."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import cells as CL
from field_coverage_path_planning_amd import engine as E
from tests.cell_cases import YOU
from tests.support import np_of as _np

pytestmark = pytest.mark.gpu

W, R, SPACING = 2.0, 2.0, 0.5
ANGLES = (0.0, np.pi / 2)
TURN_COST = 10.0          # [m] per swath, for both plans: without it an angle is chosen by swath LENGTH alone, which is area / W at any angle


@pytest.fixture(scope='module')
def plans():
    """the two plans of the U, computed once and left unchanged"""
    cells = CL.plan_polygon_cells([YOU], W, R, SPACING, ANGLES, 0.0, turn_cost=TURN_COST)
    single = E.plan_polygon_fields([YOU], W, R, SPACING, ANGLES, turn_cost=TURN_COST)
    return cells, single


def test_cells_of_the_u_and_their_paths(plans):
    plan, _ = plans
    cs = plan.cells
    n_cells = int(cs.cell_offsets_host[-1])
    assert _np(cs.status).tolist() == [0] and n_cells >= 3 and _np(cs.field).tolist() == [0] * n_cells and cs.events == 'extrema'
    assert _np(plan.swaths.status).tolist() == [0] * n_cells and (_np(plan.angle_index) >= 0).all()
    assert _np(plan.paths.status).tolist() == [0] * n_cells
    off = plan.paths.offsets_host
    assert len(off) == n_cells + 1 and (off[1:] > off[:-1]).sum() >= 3
    # every cell's path is taken by curvature and validate, as one CSR batch and alone
    p = plan.paths
    veh = E.make_vehicle(min_turn_radius=R)
    v = np.full(int(p.x.numel()), 3.0)
    kap = _np(E.curvature(p.x, p.y, offsets=p.offsets))
    flags, stats = E.validate(p.x, p.y, v, veh, offsets=p.offsets)
    assert kap.shape == (int(p.x.numel()),) and np.isfinite(kap).all() and kap.max() <= 1 / R + 1e-6
    assert int(flags.numel()) == int(p.x.numel()) and all(len(col) == n_cells for col in stats.values())
    for k in range(n_cells):
        sl = slice(int(off[k]), int(off[k + 1]))
        if sl.stop > sl.start:
            x, y, _, _ = p.field(k)
            assert np.array_equal(_np(E.curvature(x, y)), kap[sl])
            assert np.array_equal(_np(E.validate(x, y, v[sl], veh)[0]), _np(flags)[sl])
    # the legs are driven along y, the bar along x: both angles are in use
    assert set(_np(plan.angle_index).tolist()) == {0, 1}


def test_fewer_swaths_than_one_angle_per_field(plans):
    plan, single = plans
    per_cells = int(plan.swaths.offsets_host[-1])
    per_field = int(single.swaths.offsets_host[-1])
    print('swaths: %d over the cells, %d at the field\'s one best angle' % (per_cells, per_field))
    assert _np(single.swaths.status).tolist() == [0] and per_field > 0
    assert per_cells < per_field


def test_mission_and_speeds_over_the_cells():
    veh = E.make_vehicle()
    plan = CL.plan_polygon_cells([YOU], W, R, SPACING, ANGLES, 0.0, turn_cost=TURN_COST, headland_paths=True, mission='headland_first', speeds=veh,
                                 entry=[(-5.0, -5.0, 0.0)], exit=[(-5.0, -8.0, np.pi)])
    m = plan.mission
    assert int(m.offsets.numel()) - 1 == 1 and _np(m.status).tolist() == [0] and int(m.offsets_host[-1]) > 0
    # the joined sets: the headland loops first, then the cells' paths that have samples; each of those is driven once
    n_loops = int(plan.headland_paths.offsets.numel()) - 1
    off = plan.paths.offsets_host
    with_samples = int((off[1:] > off[:-1]).sum())
    item_path, item_set = _np(m.item_path), _np(m.item_set)
    assert sorted(item_path[item_set == 1].tolist()) == list(range(n_loops, n_loops + with_samples))
    assert sorted(item_path[item_set == 0].tolist()) == list(range(n_loops))
    assert _np(m.skipped).tolist() == [0]
    # the cells' work is all there: the mission's swath samples are the cells' swath samples
    assert int(((m.part == 0) & (m.src_set == 1)).sum()) == int((plan.paths.part == 0).sum())
    assert _np(plan.speeds.status).tolist() == [0]
    s_, t_, _, totals = plan.speeds.trajectory()
    length, time = (float(a) for a in totals[0])
    print('mission: %.1f m in %.1f s' % (length, time))
    assert np.isfinite(_np(t_)).all() and np.isfinite([length, time]).all() and length > 0.0 and time > 0.0
    with pytest.raises(ValueError):
        CL.plan_polygon_cells([YOU], W, R, SPACING, ANGLES, 0.0, mission='headland_first')
    with pytest.raises(ValueError):
        CL.plan_polygon_cells([YOU], W, R, SPACING, ANGLES, 0.0, entry=[(-5.0, -5.0, 0.0)])


def test_coverage_counts_of_the_original_field():
    plan = CL.plan_polygon_cells([YOU], W, R, SPACING, ANGLES, 0.0, turn_cost=TURN_COST, headland_paths=True, coverage_resolution=0.5)
    cov = plan.coverage
    assert _np(cov.status).tolist() == [0]
    counts = _np(cov.counts)[0]
    inside, covered = int(counts[0]), int(counts[1])
    print('coverage counts', counts.tolist(), 'rate', _np(cov.rate).tolist())
    assert 0 < covered <= inside
