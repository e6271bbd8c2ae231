"""CPU-side tests of the field paths: the three entries exist (header, ctypes binding, libfcpp.so; ABI version still 5), argument errors need
no device -- and the RULE, through fcpp_debug_field_paths (csrc/fcpp_fpathfn.h on the host: the very expressions the kernels run), on swaths
cut by fcpp_debug_swaths.

Checkers that share no code with the rule: a numpy restatement of the swath legs written from include/fcpp.h (numpy float64 is the same IEEE
arithmetic, so "bit for bit" is meant literally); fcpp_debug_dubins / fcpp_debug_rs on the driven pairs for the connectors' records; the
count rule restated; geometric properties of the samples.  Tolerances come from the rule: a connector ends within 2^-43 (radius + straight)
of the next leg's start (the connectors' documented bound, about 1e-11 m here), asserted at 1e-9 m; a route's cost and the driven
connectors differ only by the entries the router evaluates on the mirrored pair: 1e-9 (1 + cost), the tolerance of tests/test_gpu_route.py.
Consecutive Dubins samples are at most `spacing` apart (a chord is no longer than its arc) and, but for the last step, at least the chord of
an arc of that length; on a straight the true distance IS the spacing and the float64 coordinates (about 100 m, an ulp of 1.4e-14 m) put
the measured step a few ulp to either side of it (measured: + 1.0e-15 m), so both bounds carry the same 1e-9 m of slack.

R = 6 as in tests/test_route_host.py."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.support import check_entries, p as _p
from tests.test_guarded_host import ROUTE_W, strip
from tests.test_route_host import HOLED_SQUARE, R, bits, cut_with_angle, host_lengths, host_route, host_transit, oriented_poses
from tests.test_swaths_host import ELL, HOLE

ENTRIES = {'fcpp_field_path_counts': 27, 'fcpp_field_path_fill': 30, 'fcpp_debug_field_paths': 35}
SAMPLE_KEYS = ('x', 'y', 'heading', 'kappa', 'part', 'gear', 'leg')
SAMPLE_TYPES = dict(x=np.float64, y=np.float64, heading=np.float64, kappa=np.float64, part=np.int8, gear=np.int8, leg=np.int32)


def _cols(pose):
    if pose is None:
        return None, None, None
    pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(-1, 3)
    return tuple(np.ascontiguousarray(pose[:, k]) for k in range(3))


def host_paths(cut, radius, spacing, mode=0, order=None, entry=None, exit=None, expect=0, length=None, n=None, soff=None, n_total=None):
    """fcpp_debug_field_paths on a host_cut(): sized with cap = 0, then filled -> dict of arrays (the call's error code under 'rc')"""
    lib = L.load()
    soff = cut['offsets'] if soff is None else soff
    n = len(cut['offsets']) - 1 if n is None else n
    nt = int(cut['offsets'][-1]) if n_total is None else n_total
    ax, ay, bx, by = (np.ascontiguousarray(cut[k]) for k in ('ax', 'ay', 'bx', 'by'))
    length = np.ascontiguousarray(cut['length'] if length is None else length)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    ent, ext = _cols(entry), _cols(exit)
    n_slots = max(2 * nt + n, 0)
    out = dict(offsets=np.full(max(n, 0) + 1, -7, np.int64), leg_offsets=np.full(n_slots + 1, -7, np.int64), work=np.full(max(n, 0), -7.0),
               transit=np.full(max(n, 0), -7.0), status=np.full(max(n, 0), -7, np.int32), leg_word=np.full(n_slots, -7, np.int32),
               leg_seg=np.full((n_slots, 5), -7.0), leg_total=np.full(n_slots, -7.0))
    head = (n, _p(soff), nt, _p(ax), _p(ay), _p(bx), _p(by), _p(length), _p(cut['angle']), _p(order), float(radius), mode, float(spacing),
            *[_p(c) for c in ent], *[_p(c) for c in ext], _p(out['offsets']), _p(out['leg_offsets']), _p(out['work']), _p(out['transit']),
            _p(out['status']), _p(out['leg_word']), _p(out['leg_seg']), _p(out['leg_total']))
    rc = lib.fcpp_debug_field_paths(*head, 0, *([None] * 7))
    assert rc == expect, lib.fcpp_last_error()
    out['rc'] = rc
    if rc:
        return out
    total = int(out['offsets'][-1])
    for k in SAMPLE_KEYS:
        out[k] = np.full(total, 77, SAMPLE_TYPES[k])
    assert lib.fcpp_debug_field_paths(*head, total, *[_p(out[k]) for k in SAMPLE_KEYS]) == 0
    out['total'] = total
    return out


def first_slots(soff):
    return 2 * soff[:-1] + np.arange(len(soff) - 1)


def stored_order(soff):
    return np.concatenate([2 * np.arange(m) + (np.arange(m) & 1) for m in np.diff(soff)] + [np.zeros(0, np.int64)]).astype(np.int32)


def driven(cut, i, order):
    """field i's legs in driving order: (start poses, end poses) of its swaths, (m, 3) each, headings unwrapped as the router forms them"""
    ent, ext = oriented_poses(cut, i)
    o = np.asarray(order[cut['offsets'][i]:cut['offsets'][i + 1]], dtype=np.int64)
    return ent[o], ext[o], o


def count_rule(T, step):
    K = int(np.floor(T / step)) + 1
    return K + (1 if (K - 1) * step < T else 0)


def leg_slices(res, i, soff):
    """field i: {slot: slice of its samples}"""
    f0 = int(2 * soff[i] + i)
    m = int(soff[i + 1] - soff[i])
    lo = res['leg_offsets']
    return {j: slice(int(lo[f0 + j]), int(lo[f0 + j + 1])) for j in range(2 * m + 1)}


def wrap_diff(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def host_solve_full(f, t, radius, mode):
    lib = L.load()
    f, t = np.ascontiguousarray(f, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3)
    cols = [np.ascontiguousarray(p[:, k]) for p in (f, t) for k in range(3)]
    ns = 5 if mode else 3
    word, seg, tot = np.zeros(len(f), np.int32), np.zeros((len(f), ns)), np.zeros(len(f))
    fn = lib.fcpp_debug_rs if mode else lib.fcpp_debug_dubins
    assert fn(len(f), *[_p(c) for c in cols], float(radius), _p(word), _p(seg), _p(tot)) == 0
    return word, seg, tot


def gear_runs(seg):
    """the gear runs of a Reeds-Shepp path restated: lengths of the maximal stretches of non-zero segments of one sign"""
    runs, sign = [], 0
    for v in seg:
        if v == 0.0:
            continue
        s = 1 if v > 0 else -1
        if s != sign and len(runs) < 3:
            runs.append(0.0)
            sign = s
        runs[-1] += abs(v)
    return runs or [0.0]


FIELD_CASES = {
    'strips': ([strip(k) for k in (0.25, 1, 2, 3, 5)], 0.0, ROUTE_W),
    'holed_square': ([HOLED_SQUARE], 0.0, 4.0),
    'ell_hole': ([[ELL, HOLE]], 0.3, 4.0),
}
ENTRY, EXIT = np.array([-15.0, -10.0, 0.3]), np.array([75.0, 60.0, 1.2])


@pytest.fixture(scope='module')
def cuts():
    out = {k: cut_with_angle(f, a, W) for k, (f, a, W) in FIELD_CASES.items()}
    assert list(np.diff(out['strips']['offsets'])) == [0, 1, 2, 3, 5]
    assert int(out['holed_square']['offsets'][1]) == 14
    return out


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    check_entries(ENTRIES)
    for name in ('field_paths', 'FieldPaths', 'plan_polygon_fields'):
        assert hasattr(E, name), name


@pytest.mark.parametrize('spacing', [0.5, 7.0, 100.0])
@pytest.mark.parametrize('case', list(FIELD_CASES))
def test_swath_legs_equal_the_numpy_restatement(cuts, case, spacing):
    cut = cuts[case]
    soff = cut['offsets']
    res = host_paths(cut, R, spacing)
    assert np.all(res['status'] == 0)
    order = stored_order(soff)
    n_legs = 0
    for i in range(len(soff) - 1):
        start, end, o = driven(cut, i, order)
        sl = leg_slices(res, i, soff)
        m = len(o)
        if m == 0:
            assert res['offsets'][i + 1] == res['offsets'][i] and res['work'][i] == 0.0 and res['transit'][i] == 0.0
            continue
        work = 0.0
        for k in range(m):
            s = sl[2 * k + 1]
            length = cut['length'][soff[i] + (o[k] >> 1)]
            K = count_rule(length, spacing)
            assert s.stop - s.start == K
            t = np.minimum((np.arange(K, dtype=np.float64) * spacing) / length, 1.0)
            x = start[k, 0] + t * (end[k, 0] - start[k, 0])
            y = start[k, 1] + t * (end[k, 1] - start[k, 1])
            x[-1], y[-1] = end[k, 0], end[k, 1]
            assert np.array_equal(bits(res['x'][s]), bits(x)) and np.array_equal(bits(res['y'][s]), bits(y)), (i, k)
            h = res['heading'][s]
            assert np.all(bits(h) == bits(h[0])) and -np.pi < h[0] <= np.pi and wrap_diff(h[0], start[k, 2]) < 1e-12
            assert np.all(res['kappa'][s] == 0.0) and np.all(res['gear'][s] == 1) and np.all(res['part'][s] == 0)
            assert np.all(res['leg'][s] == 2 * k + 1)
            work = work + length
            n_legs += 1
        assert bits(res['work'][i]) == bits(work)
    assert n_legs == soff[-1]
    if case == 'holed_square':
        counts = np.diff(res['leg_offsets'])[1::2]
        want = {0.5: {81, 25}, 7.0: {7, 3}, 100.0: {2}}[spacing]          # 40 m: no extra end sample at 0.5, a remainder at 7, two at 100
        assert set(counts.tolist()) == want and np.all(np.isin(cut['length'], (40.0, 12.0)))


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('with_ends', [False, True])
@pytest.mark.parametrize('case,spacing', [('strips', 0.5), ('holed_square', 0.5), ('ell_hole', 0.5), ('holed_square', 7.0)])
def test_connectors(cuts, case, spacing, with_ends, mode):
    cut = cuts[case]
    soff = cut['offsets']
    n = len(soff) - 1
    entry = np.tile(ENTRY, (n, 1)) if with_ends else None
    exit = np.tile(EXIT, (n, 1)) if with_ends else None
    res = host_paths(cut, R, spacing, mode, entry=entry, exit=exit)
    assert np.all(res['status'] == 0)
    order = stored_order(soff)
    x, y, part, gear = res['x'], res['y'], res['part'], res['gear']
    n_conn = 0
    for i in range(n):
        start, end, o = driven(cut, i, order)
        m = len(o)
        sl = leg_slices(res, i, soff)
        f0 = int(2 * soff[i] + i)
        if m == 0:
            assert sl[0].stop == sl[0].start
            continue
        # the driven pairs, slot by slot
        froms = ([ENTRY] if with_ends else []) + list(end[:-1]) + ([end[-1]] if with_ends else [])
        tos = ([start[0]] if with_ends else []) + list(start[1:]) + ([EXIT] if with_ends else [])
        slots = ([0] if with_ends else []) + [2 * k + 2 for k in range(m - 1)] + ([2 * m] if with_ends else [])
        if not with_ends:
            assert sl[0].stop == sl[0].start and sl[2 * m].stop == sl[2 * m].start
        if not slots:
            continue
        word, seg, tot = host_solve_full(np.asarray(froms), np.asarray(tos), R, mode)
        transit = 0.0
        for c, j in enumerate(slots):
            s = sl[j]
            ns = seg.shape[1]
            assert res['leg_word'][f0 + j] == word[c] >= 0
            assert np.array_equal(bits(res['leg_seg'][f0 + j, :ns]), bits(seg[c])) and bits(res['leg_total'][f0 + j]) == bits(tot[c])
            transit = transit + tot[c]
            runs = gear_runs(seg[c]) if mode else [(seg[c, 0] + seg[c, 1]) + seg[c, 2]]
            assert s.stop - s.start == sum(count_rule(r, spacing) for r in runs), (i, j)
            assert np.all(part[s] == (2 if j == 0 else 3 if j == 2 * m else 1)) and np.all(res['leg'][s] == j)
            step = np.hypot(np.diff(x[s]), np.diff(y[s]))
            if mode == 0:
                assert np.all(gear[s] == 1)
                assert np.all(step <= spacing + 1e-9), (i, j, step.max() - spacing)
                assert np.all(step[:-1] >= 2 * R * np.sin(spacing / (2 * R)) - 1e-9)
                assert np.all(np.isin(np.abs(res['kappa'][s]), (0.0, 1.0 / R)))
            else:
                # every cusp twice, with opposite gears
                flips = np.flatnonzero(np.diff(gear[s].astype(np.int64)) != 0)
                assert len(flips) == len(runs) - 1 and np.all(np.abs(gear[s]) == 1)
                assert np.all(step[flips] <= 1e-9) and np.all(gear[s][flips] == -gear[s][flips + 1])
            # ends: the connector starts where the leg before ends (doubled) and ends within 1e-9 m of the next leg's start
            assert np.array_equal([x[s.start], y[s.start]], froms[c][:2])
            assert np.hypot(x[s.stop - 1] - tos[c][0], y[s.stop - 1] - tos[c][1]) <= 1e-9
            assert wrap_diff(res['heading'][s.stop - 1], tos[c][2]) <= 1e-9
            n_conn += 1
        assert bits(res['transit'][i]) == bits(transit)
    assert n_conn > 0


@pytest.mark.parametrize('with_ends', [False, True])
def test_layout(cuts, with_ends):
    cut = cuts['strips']
    soff = cut['offsets']
    n = len(soff) - 1
    res = host_paths(cut, R, 0.5, 1, entry=np.tile(ENTRY, (n, 1)) if with_ends else None, exit=np.tile(EXIT, (n, 1)) if with_ends else None)
    assert np.array_equal(res['offsets'][:-1], res['leg_offsets'][first_slots(soff)]) and res['offsets'][-1] == res['leg_offsets'][-1] == res['total']
    assert len(res['leg_offsets']) == 2 * soff[-1] + n + 1 and np.all(np.diff(res['leg_offsets']) >= 0)
    for i in range(n):
        m = int(soff[i + 1] - soff[i])
        s = slice(int(res['offsets'][i]), int(res['offsets'][i + 1]))
        leg, part = res['leg'][s].astype(np.int64), res['part'][s]
        assert np.all(np.diff(leg) >= 0)
        want = np.where(leg % 2 == 1, 0, np.where(leg == 0, 2, np.where(leg == 2 * m, 3, 1)))
        assert np.array_equal(part, want)
        assert (set(part.tolist()) >= {2, 3}) if (with_ends and m) else not (set(part.tolist()) & {2, 3})
        if m:
            assert set(leg.tolist()) == set(range(0 if with_ends else 1, 2 * m + (1 if with_ends else 0)))


@pytest.mark.parametrize('mode', [0, 1])
def test_stored_order_equals_the_explicit_one(cuts, mode):
    for cut in cuts.values():
        plain = host_paths(cut, R, 0.5, mode)
        given = host_paths(cut, R, 0.5, mode, order=stored_order(cut['offsets']))
        for k in SAMPLE_KEYS + ('offsets', 'leg_offsets', 'work', 'transit', 'status'):
            assert np.array_equal(plain[k].view(np.uint8), given[k].view(np.uint8)), k


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('with_ends', [False, True])
def test_routed_order_drives_every_swath_once_at_the_routes_cost(cuts, mode, with_ends):
    cut = cuts['holed_square']
    soff = cut['offsets']
    T, toff = host_transit(cut, R, mode)
    ent, ext = oriented_poses(cut, 0)
    En = host_lengths(np.tile(ENTRY, (len(ent), 1)), ent, R, mode) if with_ends else None
    Xn = host_lengths(ext, np.tile(EXIT, (len(ext), 1)), R, mode) if with_ends else None
    route = host_route(soff, T, toff, En, Xn, S=8)
    assert route['status'][0] == 0 and route['cost'][0] < route['stored'][0]
    res = host_paths(cut, R, 0.5, mode, order=route['route'], entry=ENTRY if with_ends else None, exit=EXIT if with_ends else None)
    assert res['status'][0] == 0
    start, end, o = driven(cut, 0, route['route'])
    sl = leg_slices(res, 0, soff)
    for k in range(len(o)):
        s = sl[2 * k + 1]
        assert np.array_equal([res['x'][s.start], res['y'][s.start]], start[k, :2])
        assert np.array_equal([res['x'][s.stop - 1], res['y'][s.stop - 1]], end[k, :2])
    assert np.array_equal(np.sort(o >> 1), np.arange(14))
    cost = route['cost'][0]
    print('holed square mode %d ends %s: route cost %.12f, driven %.12f' % (mode, with_ends, cost, res['transit'][0]))
    assert abs(res['transit'][0] - cost) <= 1e-9 * (1 + cost)
    assert bits(res['work'][0]) == bits(np.cumsum(cut['length'][o >> 1])[-1])


def test_failures_are_per_field(cuts):
    # three fields: the holed square, the strip of 3 and the L with its hole; field 1 is poisoned in turn
    cut = cut_with_angle([HOLED_SQUARE, strip(3), [ELL, HOLE]], [0.0, 0.0, 0.3], 4.0)
    soff = cut['offsets']
    m1, s1 = int(soff[2] - soff[1]), int(soff[1])
    assert m1 >= 2
    entry, exit = np.tile(ENTRY, (3, 1)), np.tile(EXIT, (3, 1))
    good = host_paths(cut, R, 0.5, 0, order=stored_order(soff), entry=entry, exit=exit)
    assert np.all(good['status'] == 0)

    def poisoned(**kw):
        res = host_paths(cut, R, 0.5, 0, **{**dict(order=stored_order(soff), entry=entry, exit=exit), **kw})
        assert list(res['status']) == [0, L.EINVAL, 0]
        assert res['offsets'][2] == res['offsets'][1] and np.isnan(res['work'][1]) and np.isnan(res['transit'][1])
        for i in (0, 2):
            a = slice(int(res['offsets'][i]), int(res['offsets'][i + 1]))
            b = slice(int(good['offsets'][i]), int(good['offsets'][i + 1]))
            for k in SAMPLE_KEYS:
                assert np.array_equal(res[k][a].view(np.uint8), good[k][b].view(np.uint8)), (k, i)
            assert bits(res['work'][i]) == bits(good['work'][i]) and bits(res['transit'][i]) == bits(good['transit'][i])

    twice = stored_order(soff)
    twice[s1 + 1] = twice[s1] ^ 1                  # swath 0 of field 1 twice (in both directions)
    poisoned(order=twice)
    beyond = stored_order(soff)
    beyond[s1] = 2 * m1                            # the first entry that names no swath
    poisoned(order=beyond)
    negative = stored_order(soff)
    negative[s1 + m1 - 1] = -1
    poisoned(order=negative)
    for bad in (np.nan, np.inf, -1.0):
        length = cut['length'].copy()
        length[s1 + 1] = bad
        poisoned(length=length)
    nan_entry = entry.copy()
    nan_entry[1, 2] = np.nan
    poisoned(entry=nan_entry)
    nan_exit = exit.copy()
    nan_exit[1, 0] = np.nan
    poisoned(exit=nan_exit)


def test_argument_errors(cuts):
    lib = L.load()
    cut = cuts['holed_square']
    soff, nt = cut['offsets'], int(cut['offsets'][-1])
    assert host_paths(cut, R, 0.5)['rc'] == 0
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan), dict(spacing=np.nan), dict(spacing=0.0),
               dict(spacing=np.inf), dict(mode=2), dict(mode=-1)):
        args = {**dict(radius=R, spacing=0.5, mode=0), **kw}
        assert host_paths(cut, args['radius'], args['spacing'], args['mode'], expect=L.EINVAL)['rc'] == L.EINVAL, kw
    for kw in (dict(n=-1), dict(n_total=-1), dict(soff=np.array([1, nt], np.int64)), dict(soff=np.array([0, nt - 1], np.int64)),
               dict(n_total=nt + 1)):
        assert host_paths(cut, R, 0.5, expect=L.ESIZE, **kw)['rc'] == L.ESIZE, kw
    bad_angle = dict(cut, angle=np.array([np.nan]))
    assert host_paths(bad_angle, R, 0.5, expect=L.EINVAL)['rc'] == L.EINVAL
    # an entry pose given in part; required arrays
    ax, ay, bx, by, ln, ang = (np.ascontiguousarray(cut[k]) for k in ('ax', 'ay', 'bx', 'by', 'length', 'angle'))
    one = np.zeros(1)
    tail = [None] * 8 + [0] + [None] * 7
    assert lib.fcpp_debug_field_paths(1, _p(soff), nt, _p(ax), _p(ay), _p(bx), _p(by), _p(ln), _p(ang), None, R, 0, 0.5, _p(one), None, _p(one), None, None,
                                      None, *tail) == L.EINVAL
    assert lib.fcpp_debug_field_paths(1, None, nt, _p(ax), _p(ay), _p(bx), _p(by), _p(ln), _p(ang), None, R, 0, 0.5, *([None] * 6), *tail) == L.EINVAL
    assert lib.fcpp_debug_field_paths(1, _p(soff), nt, _p(ax), _p(ay), _p(bx), _p(by), None, _p(ang), None, R, 0, 0.5, *([None] * 6), *tail) == L.EINVAL
    # the device entries refuse a NULL handle before anything else
    assert lib.fcpp_field_path_counts(None, 1, _p(soff), _p(soff), nt, _p(ax), _p(ay), _p(bx), _p(by), _p(ln), _p(ang), None, R, 0, 0.5, *([None] * 12)) == L.EINVAL
    assert lib.fcpp_field_path_fill(None, 1, _p(soff), _p(soff), nt, _p(ax), _p(ay), _p(bx), _p(by), _p(ln), _p(ang), None, R, 0, 0.5, *([None] * 7), 0,
                                    *([None] * 7)) == L.EINVAL


@pytest.mark.parametrize('mode', [0, 1])
def test_a_field_alone_and_as_field_40_of_65(mode):
    rng = np.random.default_rng(11)
    kinds = [(HOLED_SQUARE, 0.0), ([ELL, HOLE], 0.3), (strip(3), 0.0), (strip(0.25), 0.0)]
    fields, angles = [], []
    for i in range(65):
        f, a = kinds[i % len(kinds)]
        fields.append(f)
        angles.append(a)
    fields[40], angles[40] = [ELL, HOLE], 0.3
    entry = np.column_stack([rng.uniform(-30, 0, 65), rng.uniform(-30, 0, 65), rng.uniform(-3, 3, 65)])
    exit = np.column_stack([rng.uniform(60, 90, 65), rng.uniform(50, 80, 65), rng.uniform(-3, 3, 65)])
    batch = cut_with_angle(fields, angles, 4.0)
    alone = cut_with_angle([fields[40]], [angles[40]], 4.0)
    big = host_paths(batch, R, 0.5, mode, entry=entry, exit=exit)
    one = host_paths(alone, R, 0.5, mode, entry=entry[40:41], exit=exit[40:41])
    s = slice(int(big['offsets'][40]), int(big['offsets'][41]))
    assert s.stop - s.start == one['total'] > 0
    for k in SAMPLE_KEYS:
        assert np.array_equal(big[k][s].view(np.uint8), one[k].view(np.uint8)), k
    assert bits(big['work'][40]) == bits(one['work'][0]) and bits(big['transit'][40]) == bits(one['transit'][0])
