"""GPU tests of the swath router (run with -m gpu on an MI355X): the kernels of csrc/fcpp_route.hip against the same rule on the host
(fcpp_debug_route_transit / fcpp_debug_route) BIT FOR BIT -- the transit blocks, every candidate's tour and cost, winner, sweeps, status and
the stored cost.  The minimum over (delta, code) pairs does not depend on how the device hands the moves to its threads and every delta is
one expression, so nothing here is compared to a bound.  Then swath_route(order=...) through the project's own operators.

The fields: strips of k working widths (k lines at angle 0, hence m = k swaths) for m = 0, 1, 2, 3, 4, 5, 63, 64, 65 and 130 -- tours and
move counts on both sides of the 64-lane and 256-thread boundaries --, the square with a hole, the L with its hole, a 65-vertex star at an
oblique angle and a field with a NaN vertex (a swath status, m = 0).  R = 6 as in tests/test_route_host.py."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.support import np_of as _np
from tests.test_route_host import HOLED_SQUARE, MIN_GAIN, R, bits, cut_with_angle, host_lengths, host_route, host_transit, oriented_poses
from tests.test_guarded_host import ROUTE_S, ROUTE_STRIPS, ROUTE_W, assert_permutations
from tests.test_guarded_host import strip as _strip
from tests.test_swaths_host import ELL, HOLE, rings_of, star

pytestmark = pytest.mark.gpu

W = ROUTE_W          # _strip(k): a strip of k working widths of ROUTE_W = 3.2
NAN_FIELD = np.array(ELL, dtype=np.float64)
NAN_FIELD[3, 0] = np.nan


KINDS = [(_strip(65), 0.0), (HOLED_SQUARE, 0.0), (_strip(0.25), 0.0), (_strip(1), 0.0), (_strip(2), 0.0), (_strip(3), 0.0), (_strip(4), 0.0),
         (_strip(5), 0.0), (_strip(63), 0.0), (_strip(64), 0.0), (_strip(130), 0.0), ([ELL, HOLE], 0.3), (star(65, 65), 1.1), (NAN_FIELD, 0.0),
         (HOLED_SQUARE, 0.7)]
COUNTS = [65, None, 0, 1, 2, 3, 4, 5, 63, 64, 130, None, None, 0, None]


def batch(n):
    """n fields cycling through the kinds (a batch of one is the strip of 65 swaths), the later rounds moved a little"""
    rng = np.random.default_rng(7 + n)
    fields, angles = [], []
    for i in range(n):
        f, a = KINDS[i % len(KINDS)]
        shift = rng.uniform(-20.0, 20.0, 2) * (i >= len(KINDS))
        fields.append([r + shift for r in rings_of(f)])
        angles.append(a)
    return fields, np.asarray(angles)


def field_poses(n):
    k = np.arange(n, dtype=np.float64)
    return np.column_stack([-15.0 - k, -10.0 + 0.5 * k, 0.3 + 0.01 * k]), np.column_stack([75.0 + k, 60.0 - 0.5 * k, 1.2 - 0.01 * k])


@pytest.fixture(scope='module')
def reference():
    """per batch size: the fields, the host's cut, and per mode the host's transit blocks -- computed once, left unchanged"""
    out = {}
    for n in (1, 65):
        fields, angles = batch(n)
        cut = cut_with_angle(fields, angles, W)
        for i in range(min(n, len(COUNTS))):
            if COUNTS[i] is not None:
                assert cut['offsets'][i + 1] - cut['offsets'][i] == COUNTS[i]
        out[n] = (fields, angles, cut, {mode: host_transit(cut, R, mode) for mode in (0, 1)})
    return out


@pytest.fixture(scope='module')
def device_cut(reference):
    return {n: E.polygon_swaths(reference[n][0], reference[n][1], W) for n in reference}


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [1, 65])
def test_transit_equals_host_bit_for_bit(reference, device_cut, n, mode):
    _, _, cut, hostT = reference[n]
    ss = device_cut[n]
    assert np.array_equal(ss.offsets_host, cut['offsets']) and np.array_equal(bits(_np(ss.a)), bits(cut['a']))
    T, toff = E.swath_transit(ss, R, reversing=bool(mode))
    assert np.array_equal(toff, hostT[mode][1]) and T.numel() == toff[-1]
    assert np.array_equal(bits(_np(T)), bits(hostT[mode][0]))


def host_ends(cut, mode, entry, exit):
    En, Xn = [], []
    for i in range(len(cut['offsets']) - 1):
        ent, ext = oriented_poses(cut, i)
        En.append(host_lengths(np.tile(entry[i], (len(ent), 1)), ent, R, mode))
        Xn.append(host_lengths(ext, np.tile(exit[i], (len(ext), 1)), R, mode))
    return np.concatenate(En), np.concatenate(Xn)


# S in {1, 2, 5}, both modes, with and without E / X, max_sweeps 0, 1 and the default (None), on both batch sizes
SOLVES = [(65, 0, 5, True, None), (65, 1, 2, False, None), (65, 0, 1, False, 0), (65, 1, 5, True, 1), (1, 0, 5, True, None), (1, 1, 1, False, 1),
          (1, 0, 2, True, 0), (1, 1, 5, False, None)]


@pytest.mark.parametrize('n,mode,S,with_ends,max_sweeps', SOLVES)
def test_solve_equals_host_bit_for_bit(reference, device_cut, monkeypatch, n, mode, S, with_ends, max_sweeps):
    _, _, cut, hostT = reference[n]
    ss = device_cut[n]
    entry, exit = field_poses(n) if with_ends else (None, None)
    En, Xn = host_ends(cut, mode, entry, exit) if with_ends else (None, None)
    host = host_route(cut['offsets'], *hostT[mode], En, Xn, S=S, max_sweeps=max_sweeps)
    dev = E.route_swaths(ss, R, reversing=bool(mode), entry=entry, exit=exit, starts=S, min_gain=MIN_GAIN, max_sweeps=max_sweeps)
    assert np.array_equal(_np(dev.tours), host['tours'])
    assert np.array_equal(bits(_np(dev.costs)), bits(host['costs']))
    assert np.array_equal(_np(dev.order), host['route']) and np.array_equal(bits(_np(dev.cost)), bits(host['cost']))
    assert np.array_equal(bits(_np(dev.stored_cost)), bits(host['stored']))
    for k in ('winner', 'sweeps', 'status'):
        assert np.array_equal(_np(getattr(dev, k)), host[k]), k
    assert np.all(host['status'] == 0)
    if max_sweeps is None:
        assert np.all(host['sweeps'] < host['max_sweeps']) and np.all(host['cost'] <= host['stored'])
        if n == 65 and mode == 0:          # (W = 3.2 < 2 R: the Dubins boustrophedon is all loops)
            assert (host['cost'] < host['stored'] - MIN_GAIN).sum() >= 30
    if n == 65 and max_sweeps == 0:
        # solved in chunks of a few fields: the same results
        monkeypatch.setattr(E, 'ROUTE_T_BUDGET', 300 * 1024)
        assert len(E._route_chunks(cut['offsets'], E.ROUTE_T_BUDGET)) > 5
        again = E.route_swaths(ss, R, reversing=bool(mode), starts=S, max_sweeps=0)
        assert np.array_equal(_np(again.order), host['route']) and np.array_equal(bits(_np(again.costs)), bits(host['costs']))


# ---- tour lengths on the edges of the solve kernel's blocks --------------------------------------------------------------------------------
# ROUTE_STRIPS: m = 255, 256, 257 -- a tour that ends under, on and over the 256-thread stride -- in both modes; 511 and the cap 512 (int16
# positions up to 1023, every sweep 1.8e6 moves) Dubins only: their transit blocks are 8 MiB each.
EDGE_MODES = [(0, len(ROUTE_STRIPS)), (1, 3)]


@pytest.fixture(scope='module')
def edge_reference():
    """per mode: the host's cut of the strips, its transit blocks and E / X -- computed once, left unchanged"""
    out = {}
    for mode, count in EDGE_MODES:
        fields = [_strip(k) for k in ROUTE_STRIPS[:count]]
        cut = cut_with_angle(fields, 0.0, W)
        assert list(np.diff(cut['offsets'])) == list(ROUTE_STRIPS[:count])
        entry, exit = field_poses(count)
        out[mode] = (fields, cut, host_transit(cut, R, mode), entry, exit, host_ends(cut, mode, entry, exit))
    return out


@pytest.mark.parametrize('mode,count', EDGE_MODES)
def test_tour_length_edges_equal_host_bit_for_bit(edge_reference, mode, count):
    fields, cut, (T, toff), entry, exit, (En, Xn) = edge_reference[mode]
    ss = E.polygon_swaths(fields, 0.0, W)
    assert np.array_equal(ss.offsets_host, cut['offsets']) and np.array_equal(bits(_np(ss.a)), bits(cut['a']))
    devT, dev_toff = E.swath_transit(ss, R, reversing=bool(mode))
    assert np.array_equal(dev_toff, toff) and np.array_equal(bits(_np(devT)), bits(T))
    for max_sweeps in (0, 3):
        host = host_route(cut['offsets'], T, toff, En, Xn, S=ROUTE_S, max_sweeps=max_sweeps)
        dev = E.route_swaths(ss, R, reversing=bool(mode), entry=entry, exit=exit, starts=ROUTE_S, min_gain=MIN_GAIN, max_sweeps=max_sweeps)
        assert np.array_equal(_np(dev.tours), host['tours'])
        assert np.array_equal(bits(_np(dev.costs)), bits(host['costs']))
        assert np.array_equal(_np(dev.order), host['route']) and np.array_equal(bits(_np(dev.cost)), bits(host['cost']))
        assert np.array_equal(bits(_np(dev.stored_cost)), bits(host['stored']))
        for k in ('winner', 'sweeps', 'status'):
            assert np.array_equal(_np(getattr(dev, k)), host[k]), k
        # what must actually happen: every field is routed, every tour a permutation, and with sweeps allowed moves ARE applied at the cap
        assert np.all(host['status'] == 0) and np.isfinite(host['costs']).all()
        assert_permutations(host['tours'], cut['offsets'])
        if max_sweeps == 0:
            assert np.all(host['sweeps'] == 0)
        else:
            assert np.all(host['sweeps'] >= 1) and np.all(host['sweeps'] <= 3) and np.all(host['cost'] < host['stored'])
            if mode == 0:
                assert cut['offsets'][-1] - cut['offsets'][-2] == 512 and host['sweeps'][-1] >= 1


def test_statuses_on_the_device():
    import torch
    strip = lambda k: np.array([(0, 0), (10, 0), (10, 4.0 * k), (0, 4.0 * k)], dtype=np.float64)
    fields = [strip(513), HOLED_SQUARE, strip(3)]
    cut = cut_with_angle(fields, 0.0, 4.0)
    ss = E.polygon_swaths(fields, 0.0, 4.0)
    assert list(np.diff(ss.offsets_host)) == [513, 14, 3]
    # a swath of the holed square that is not finite: its transits are NaN, the stored cost is not finite
    a = ss.a.clone()
    a[513 + 3, 0] = float('nan')
    ss.a = a
    cut['ax'] = cut['ax'].copy()
    cut['ax'][513 + 3] = np.nan
    T, toff = host_transit(cut, R, 0)
    host = host_route(cut['offsets'], T, toff, S=5, max_sweeps=20)
    dev = E.route_swaths(ss, R, starts=5, max_sweeps=20)
    assert _np(dev.status).tolist() == [L.EUNSUPPORTED, L.EINVAL, 0] == host['status'].tolist()
    assert np.array_equal(_np(dev.tours), host['tours']) and np.array_equal(_np(dev.order), host['route'])
    # (NaN costs: equal as NaN, whatever the payload; finite ones exactly)
    assert np.array_equal(_np(dev.costs), host['costs'], equal_nan=True) and np.array_equal(_np(dev.cost), host['cost'], equal_nan=True)
    assert np.isnan(host['cost'][:2]).all() and np.array_equal(bits(_np(dev.cost)[2:]), bits(host['cost'][2:]))
    assert np.array_equal(_np(dev.winner), host['winner']) and np.array_equal(_np(dev.sweeps), host['sweeps'])
    k = np.arange(513)
    assert np.array_equal(_np(dev.field(0)), 2 * k + (k & 1)) and np.array_equal(_np(dev.field(1)), 2 * k[:14] + (k[:14] & 1))
    with pytest.raises(L.FcppError):
        E.route_swaths(ss, R, starts=0)
    with pytest.raises(L.FcppError):
        E.route_swaths(ss, -1.0)
    assert torch.cuda.is_available()


# ---- swath_route(order=...) -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def holed():
    ss = E.polygon_swaths([HOLED_SQUARE], 0.0, 4.0)
    return ss, {rev: E.route_swaths(ss, R, reversing=rev, spacing=0.5) for rev in (False, True)}


def _runs(part):
    cut = np.flatnonzero(np.diff(part)) + 1
    return np.concatenate([[0], cut]), np.concatenate([cut, [len(part)]])


@pytest.mark.parametrize('reversing', [False, True])
def test_swath_route_follows_the_order(holed, reversing):
    ss, routes = holed
    route = routes[reversing]
    order = _np(route.field(0)).astype(np.int64)
    m = len(order)
    assert m == 14 and np.array_equal(np.sort(order >> 1), np.arange(m)) and route.status[0] == 0
    assert route.cost[0] < route.stored_cost[0] - MIN_GAIN
    x, y, h, part = (_np(t) for t in E.swath_route(ss, 0, R, 0.5, reversing=reversing, order=route))
    lo, hi = _runs(part)
    assert len(lo) == 2 * m - 1 and np.all(part[lo[0::2]] == 0) and np.all(part[lo[1::2]] == 1)
    # every swath once, in the order and the directions of the route: a swath run starts and ends at the oriented swath's end points
    a, b = _np(ss.a), _np(ss.b)
    for k, p in enumerate(order):
        s, e = (b[p >> 1], a[p >> 1]) if p & 1 else (a[p >> 1], b[p >> 1])
        i0, i1 = lo[2 * k], hi[2 * k] - 1
        assert np.array_equal([x[i0], y[i0]], s) and np.array_equal([x[i1], y[i1]], e)
    # the connectors driven are the ones the router priced: the solve on the driven pairs at swath_route's radius
    (f_s, f_e), (r_s, r_e) = ss.poses(0)
    f_s, f_e, r_s, r_e = (_np(t) for t in (f_s, f_e, r_s, r_e))
    odd = (order & 1).astype(bool)[:, None]
    start, end = np.where(odd, r_s[order >> 1], f_s[order >> 1]), np.where(odd, r_e[order >> 1], f_e[order >> 1])
    solve = E.rs_solve if reversing else E.dubins_solve
    length = _np(solve(end[:-1], start[1:], E._chord_radius(R, 0.5))[2])
    cost = float(route.cost[0])
    print('holed square reversing=%s: cost %.9f, driven connectors %.9f, stored %.9f' % (reversing, cost, length.sum(), float(route.stored_cost[0])))
    assert abs(length.sum() - cost) <= 1e-9 * (1 + cost)
    # and their sampled lengths: every Dubins connector's samples are `spacing` apart but the last step (Reeds-Shepp samples per gear run)
    assert reversing or np.all((hi[1::2] - lo[1::2] - 1) * 0.5 >= length - 1e-9) and np.all((hi[1::2] - lo[1::2] - 2) * 0.5 <= length + 1e-9)
    # an order given as a plain array; an order that is no permutation
    again = E.swath_route(ss, 0, R, 0.5, reversing=reversing, order=order)
    assert all(np.array_equal(_np(p), q) for p, q in zip(again, (x, y, h, part)))
    with pytest.raises(ValueError):
        E.swath_route(ss, 0, R, 0.5, order=np.r_[order[:-1], order[0]])


@pytest.mark.parametrize('reversing', [False, True])
def test_candidate_zero_order_is_the_stored_route_bit_for_bit(holed, reversing):
    ss, _ = holed
    k = np.arange(14)
    plain = E.swath_route(ss, 0, R, 0.5, reversing=reversing)
    given = E.swath_route(ss, 0, R, 0.5, reversing=reversing, order=2 * k + (k & 1))
    for p, q in zip(plain, given):
        assert p.dtype == q.dtype and np.array_equal(_np(p).view(np.int8), _np(q).view(np.int8))
    stored = E.route_swaths(ss, R, reversing=reversing, starts=1, max_sweeps=0, spacing=0.5)
    assert np.array_equal(_np(stored.field(0)), 2 * k + (k & 1))
    assert np.array_equal(bits(_np(stored.cost)), bits(_np(stored.stored_cost)))


def test_routed_path_is_flagged_no_more_than_the_stored_one(holed):
    """Connectors know no boundary: validate() flags what leaves the field or crosses the hole.  Reported; asserted only as "not worse"."""
    ss, routes = holed
    veh = E.make_vehicle()
    counts = {}
    for name, order in (('stored', None), ('routed', routes[False])):
        x, y, _, _ = E.swath_route(ss, 0, R, 0.5, order=order)
        v = np.ones(x.numel())
        flags, st = E.validate(x, y, v, veh, [HOLED_SQUARE[0]], [HOLED_SQUARE[1]])
        flags = _np(flags).view(np.uint32)
        counts[name] = int(((flags & (L.FLAG_OUTSIDE | L.FLAG_OBSTACLE)) != 0).sum())
        print('%s route: %d points, %d flagged (outside %d, in the hole %d)' % (name, x.numel(), counts[name], st['n_outside'][0], st['n_in_obstacle'][0]))
    assert counts['routed'] <= counts['stored']
