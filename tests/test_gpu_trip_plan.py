"""GPU tests of the service trips' Python layer (run with -m gpu on an MI355X): service_trips, trip_paths and plan_trips of
field_coverage_path_planning_amd/trips.py on the rectangle [0, 60] x [0, 40] cut at angle 0 and width 4 -- ten swaths of 60 m --, turning
radius 2, spacing 0.5, the service pose (-5, 20, pi / 2) west of the field, route_swaths(entry = exit = service, starts = 8); Dubins and
Reeds-Shepp.  The split's cost is held to the numpy oracle's minimum over all 16 x 2^9 stop sets of the tables actually used (the transit
block and the ways to and from the service pose, read back from the device), the trips' paths to the split's cost, to the undivided path of
the same tour (work, coverage) and, with a region to stay clear of, to field_paths on a hand-built one-trip SwathSet."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import engine as E
from field_coverage_path_planning_amd import trips as TR
from tests import trip_cases as TC
from tests.mission_cases import HOLED_SQUARE
from tests.support import bits, np_of

pytestmark = pytest.mark.gpu

RECT = [[(0.0, 0.0), (60.0, 0.0), (60.0, 40.0), (0.0, 40.0)]]
W, R, SPACING = 4.0, 2.0, 0.5
SERVICE = np.array([[-5.0, 20.0, np.pi / 2]])
SAMPLE_COLS = ('x', 'y', 'heading', 'kappa', 'part', 'gear', 'leg')


@pytest.fixture(scope='module', params=[False, True], ids=['dubins', 'reeds-shepp'])
def scene(request):
    """the swaths, the route and the tables the split reads: computed once per mode and left unchanged"""
    rev = request.param
    E.get_context(None).bind_stream()
    ss = E.polygon_swaths([RECT], 0.0, W)
    assert np_of(ss.length).tolist() == [60.0] * 10
    route = E.route_swaths(ss, R, reversing=rev, entry=SERVICE, exit=SERVICE, starts=8, spacing=SPACING)
    Rc = E._chord_radius(R, SPACING)
    T, _ = E.swath_transit(ss, Rc, reversing=rev)
    In = np_of(E._route_ends(ss, SERVICE, True, Rc, rev, None))
    Out = np_of(E._route_ends(ss, SERVICE, False, Rc, rev, None))
    return rev, ss, route, np_of(T).reshape(20, 20), In, Out


def same_samples(a, b, sl_a=slice(None), sl_b=slice(None)):
    for k in SAMPLE_COLS:
        assert np_of(getattr(a, k))[sl_a].tobytes() == np_of(getattr(b, k))[sl_b].tobytes(), k


def test_capacity_of_150_m_makes_five_trips(scene):
    rev, ss, route, T, In, Out = scene
    sp = TR.service_trips(ss, route, SERVICE, 150.0, R, spacing=SPACING, reversing=rev)
    tour, trip = np_of(sp.tour), np_of(sp.trip)
    assert np_of(sp.status).tolist() == [0] and np_of(sp.n_trips).tolist() == [5] and np_of(sp.overfull).tolist() == [0]          # three swaths are 180 m
    assert np_of(sp.stops).tolist() == [4] and np_of(sp.trip_offsets).tolist() == [0, 5] and np_of(sp.trip_field).tolist() == [0] * 5
    # the trips partition the tour
    assert sorted((tour >> 1).tolist()) == list(range(10)) and trip[0] == 0 and set(np.diff(trip).tolist()) <= {0, 1} and trip[-1] == 4
    tso = np_of(sp.trip_swath_offsets)
    assert tso[0] == 0 and tso[-1] == 10 and all((trip[tso[k]:tso[k + 1]] == k).all() for k in range(5))
    work = np_of(sp.trip_work)
    assert (work <= 150.0).all() and work.sum() == 600.0 and work.tolist() == [60.0 * (tso[k + 1] - tso[k]) for k in range(5)]
    # the oracle: every stop set of every variant, on the tables the split used
    tours = np_of(route.tours)
    length = np_of(ss.length)
    row = np.empty(16)
    for v in range(16):
        P, d, base = TC.tables(TC.variant(tours[v >> 1], v & 1), T, length, In, Out, In, Out, 0.0)
        row[v] = TC.plus(base, TC.brute(P, d, 150.0, 150.0))
    print('costs', np_of(sp.costs)[0], 'oracle', row)
    assert bits(np_of(sp.costs)[0]).tolist() == bits(row).tolist()
    assert bits(np_of(sp.cost))[0] == bits(row.min()) and np_of(sp.winner)[0] == int(np.argmin(row))
    # no dearer than the route's own order with its best stops
    own = TR.service_trips(ss, route, SERVICE, 150.0, R, spacing=SPACING, reversing=rev, candidates='route', both_ways=False)
    assert np_of(own.tour).tolist() == np_of(route.order).tolist() and bits(np_of(own.base)).tolist() == bits(np_of(route.cost)).tolist()
    assert np_of(own.costs).shape == (1, 2) and np.isnan(np_of(own.costs)[0, 1])
    assert np_of(sp.cost)[0] <= np_of(route.cost)[0] + np_of(own.extra)[0]


def test_a_capacity_beyond_the_field_is_the_route(scene):
    rev, ss, route, T, In, Out = scene
    sp, tp = TR.plan_trips(type('Plan', (), dict(swaths=ss, route=route))(), SERVICE, 1e9, R, SPACING, reversing=rev)
    assert np_of(sp.n_trips).tolist() == [1] and not np_of(sp.trip).any() and np_of(sp.extra).tolist() == [0.0]
    assert bits(np_of(sp.costs)[:, 0::2]).tolist() == bits(np_of(route.costs)).tolist()
    whole = E.field_paths(ss, R, SPACING, reversing=rev, order=sp.tour, entry=SERVICE, exit=SERVICE)
    assert np_of(tp.offsets).tolist() == np_of(whole.offsets).tolist() and int(tp.offsets_host[-1]) > 1000
    same_samples(tp, whole)
    assert np_of(tp.pass_id()).tolist() == np_of(whole.leg).tolist()


@pytest.mark.parametrize('stop_cost', [0.0, 3.0])
def test_trip_paths_drive_what_the_split_priced(scene, stop_cost):
    rev, ss, route, T, In, Out = scene
    sp = TR.service_trips(ss, route, SERVICE, 150.0, R, spacing=SPACING, reversing=rev, stop_cost=stop_cost)
    tp = TR.trip_paths(ss, sp, R, SPACING, reversing=rev)
    K = int(sp.trip_offsets_host[-1])
    assert K == 5 and np_of(tp.status).tolist() == [0] * K and np_of(tp.path_field()).tolist() == [0] * K
    cost, stops = float(np_of(sp.cost)[0]), int(np_of(sp.stops)[0])
    driven = float(np_of(tp.transit_length).sum())
    print('cost', cost, 'stops', stops, 'driven', driven, 'difference', driven - (cost - stop_cost * stops))
    assert abs(driven - (cost - stop_cost * stops)) <= 1e-9 * (1 + cost)
    assert abs(float(np_of(tp.work_length).sum()) - 600.0) <= 1e-9 and np_of(tp.work_length).tolist() == np_of(sp.trip_work).tolist()
    # every trip leaves from the service point and comes back to it
    off, x, y = tp.offsets_host, np_of(tp.x), np_of(tp.y)
    for k in range(K):
        for at in (off[k], off[k + 1] - 1):
            assert abs(x[at] - SERVICE[0, 0]) <= 1e-9 and abs(y[at] - SERVICE[0, 1]) <= 1e-9, (k, at)
    # the trips cover what the undivided path of the same tour covers, and overlap where it overlaps
    whole = E.field_paths(ss, R, SPACING, reversing=rev, order=sp.tour, entry=SERVICE, exit=SERVICE)
    a = E.polygon_coverage([RECT], W, 0.5, paths=(tp,))
    b = E.polygon_coverage([RECT], W, 0.5, paths=(whole,))
    assert np_of(a.counts).tolist() == np_of(b.counts).tolist() and np_of(a.status).tolist() == [0]
    ids = np_of(tp.pass_id())[np_of(tp.work())]
    assert len(set(ids.tolist())) == 10          # (a pass id per swath, none shared by two trips)
    # the vehicle stands at both ends of every trip
    v = np_of(E.path_speeds(tp, E.make_vehicle()).v)
    assert all(v[off[k]] == 0.0 and v[off[k + 1] - 1] == 0.0 for k in range(K)) and v.max() > 0.0


def test_entry_and_exit_belong_to_the_first_and_the_last_trip(scene):
    rev, ss, route, T, In, Out = scene
    gate_in, gate_out = np.array([[-8.0, 2.0, 0.0]]), np.array([[-8.0, 38.0, np.pi]])
    sp = TR.service_trips(ss, route, SERVICE, 150.0, R, spacing=SPACING, reversing=rev, entry=gate_in, exit=gate_out, first_capacity=70.0)
    assert np_of(sp.n_trips)[0] >= 5 and np_of(sp.trip_work)[0] == 60.0
    tp = TR.trip_paths(ss, sp, R, SPACING, reversing=rev)
    off, x, y = tp.offsets_host, np_of(tp.x), np_of(tp.y)
    K = len(off) - 1
    near = lambda at, px, py: abs(x[at] - px) <= 1e-9 and abs(y[at] - py) <= 1e-9
    assert near(off[0], -8.0, 2.0) and near(off[K] - 1, -8.0, 38.0)          # the gates: the first trip's start, the last trip's end
    assert near(off[1] - 1, -5.0, 20.0) and near(off[1], -5.0, 20.0)         # in between: the service point
    cost = float(np_of(sp.cost)[0])
    assert abs(float(np_of(tp.transit_length).sum()) - cost) <= 1e-9 * (1 + cost)


def test_a_trip_clear_of_the_pond_is_field_paths_on_its_own_swaths():
    import torch
    E.get_context(None).bind_stream()
    ss = E.polygon_swaths([HOLED_SQUARE], 0.0, W)
    route = E.route_swaths(ss, R, entry=SERVICE, exit=SERVICE, starts=4, spacing=SPACING, clear_of=[HOLED_SQUARE])
    sp = TR.service_trips(ss, route, SERVICE, 100.0, R, spacing=SPACING, clear_of=[HOLED_SQUARE])
    tp = TR.trip_paths(ss, sp, R, SPACING, clear_of=[HOLED_SQUARE])
    K = int(sp.trip_offsets_host[-1])
    assert K >= 3 and np_of(tp.status).tolist() == [0] * K and tp.leg_rank is not None
    k = 1
    tso, tour = np_of(sp.trip_swath_offsets), np_of(sp.tour)
    mine = tour[tso[k]:tso[k + 1]]
    s = mine >> 1
    dev = ss.a.device
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    one = E.SwathSet(up(np.array([0, len(s)], dtype=np.int64)), np.array([0, len(s)], dtype=np.int64), up(np_of(ss.a)[s]), up(np_of(ss.b)[s]),
                     up(np_of(ss.line)[s]), up(np_of(ss.length)[s]), ss.status[:1], ss.n_lines[:1], ss.angle[:1])
    order = 2 * np.arange(len(s)) + (mine & 1)
    want = E.field_paths(one, R, SPACING, order=order.astype(np.int32), entry=SERVICE, exit=SERVICE, clear_of=[HOLED_SQUARE])
    off = tp.offsets_host
    assert off[k + 1] - off[k] == int(want.offsets_host[-1]) > 0
    same_samples(tp, want, slice(off[k], off[k + 1]))
    assert bits(np_of(tp.transit_length)[k:k + 1]).tolist() == bits(np_of(want.transit_length)).tolist()
