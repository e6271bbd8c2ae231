"""CPU-side tests of the Reeds-Shepp connectors: the five entries exist (header, ctypes binding, libfcpp.so; ABI version still 5), argument
errors need no device, the engine raises without a GPU -- and the MATHEMATICS, through fcpp_debug_rs (csrc/fcpp_rsfn.h on the host: the very
function the kernels run, bit for bit).

Most properties below need no formula at all: the chosen (word, seg) integrated in numpy.longdouble ends on the goal; the total is bounded
below by the chord and by R |dh|, above by the two Dubins paths of the pair (fcpp_debug_dubins; forward, and all in reverse); the length is a
METRIC -- symmetric, and a solver that misses a shorter word for (a, c) is caught by a detour through b in the triangle inequality.

The restatement is written from the PUBLISHED normalised formulas (J. A. Reeds, L. A. Shepp, "Optimal paths for a car that goes both forwards
and backwards", Pacific J. Math. 145 (1990), section 8: start pose at the origin, unit radius; time-flip, reflect and backwards applied
to the INPUTS, every transform evaluated on its own -- the library shares eight polar forms between them).  How independent it is, formula by
formula: 8.1 - 8.4 and 8.9 - 8.10 are the paper's polar forms as the public OMPL ReedsSheppStateSpace writes them (8.9 with atan2(r, -2),
8.10 on the rotated vector (-eta, xi)); 8.11 is the products-inside-atan2 form; 8.7 and 8.8 come from the chain of the four tangent
circles' centres, in complex numbers -- the same derivation as the library's header, so for these two the restatement checks the arithmetic,
not the derivation.  The formula-free properties (closure, bounds, metric) carry the weight.  Its angle reduction and its feasibility tests
are the naive ones (no tolerance).  It runs in float64 and in numpy.longdouble.

Tolerances come from the project, not from what the code gives: positions and lengths 1e-9 m, headings 1e-12 rad."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.support import REPO, check_entries

P_TOL, H_TOL = 1e-9, 1e-12
EDGE = 1e-9             # a pair with a root / acos argument or a sign test of the restatement this close to its edge may be left out of the EQUALITY
FRAGILE_CAP = 0.005     # ... at most this share of a run (asserted): the cap of tests/test_dubins_host.py
RADII = (2.0, 8.0, 25.0)
N_RANDOM = 60_000

# the table of include/fcpp.h: word = 4 * base + flip + 2 * mirror
BASES = ('L+S+L+', 'L+S+R+', 'L+R-L+', 'L+R-L-', 'L-R-L+', 'L+R+L-R-', 'L+R-L-R+', 'L+R-S-L-', 'L+R-S-R-', 'L-S-R-L+', 'R-S-R-L+', 'L+R-S-L-R+')
TURNS = np.zeros((48, 5), dtype=np.int64)
GEARS = np.zeros((48, 5), dtype=np.int64)
for _w in range(48):
    _b = BASES[_w >> 2]
    for _k in range(len(_b) // 2):
        _t = {'L': 1, 'R': -1, 'S': 0}[_b[2 * _k]]
        TURNS[_w, _k] = -_t if _w & 2 else _t
        _g = 1 if _b[2 * _k + 1] == '+' else -1
        GEARS[_w, _k] = -_g if _w & 1 else _g
N_SEG = np.array([len(BASES[w >> 2]) // 2 for w in range(48)])

ENTRIES = {'fcpp_rs_solve': 12, 'fcpp_rs_matrix': 12, 'fcpp_rs_counts': 7, 'fcpp_rs_sample': 17, 'fcpp_debug_rs': 11}


def _cols(frm, to):
    frm, to = np.ascontiguousarray(frm, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(to, dtype=np.float64).reshape(-1, 3)
    return len(frm), [np.ascontiguousarray(a[:, k]) for a in (frm, to) for k in range(3)]


def host_solve(frm, to, R):
    """fcpp_debug_rs -> (word int32 (n,), seg (n, 5), total (n,))"""
    lib = L.load()
    n, cols = _cols(frm, to)
    word, seg, tot = np.empty(n, dtype=np.int32), np.empty((n, 5)), np.empty(n)
    rc = lib.fcpp_debug_rs(n, *[c.ctypes.data for c in cols], float(R), word.ctypes.data, seg.ctypes.data, tot.ctypes.data)
    assert rc == 0, lib.fcpp_last_error()
    return word, seg, tot


def dubins_total(frm, to, R):
    lib = L.load()
    n, cols = _cols(frm, to)
    tot = np.empty(n)
    rc = lib.fcpp_debug_dubins(n, *[c.ctypes.data for c in cols], float(R), None, None, tot.ctypes.data)
    assert rc == 0, lib.fcpp_last_error()
    return tot


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def random_pairs(rng, n, R, near):
    """the generator of tests/test_dubins_host.py: positions U[0, 5000)^2, headings U(-pi, pi]; near: the goal within U[0, 4R) of the start"""
    frm = np.column_stack((rng.uniform(0, 5000, n), rng.uniform(0, 5000, n), -rng.uniform(-np.pi, np.pi, n)))
    if near:
        r, a = rng.uniform(0, 4 * R, n), rng.uniform(-np.pi, np.pi, n)
        pos = frm[:, :2] + np.column_stack((r * np.cos(a), r * np.sin(a)))
    else:
        pos = np.column_stack((rng.uniform(0, 5000, n), rng.uniform(0, 5000, n)))
    return frm, np.column_stack((pos, -rng.uniform(-np.pi, np.pi, n)))


def integrate(frm, R, word, seg, dtype=np.longdouble):
    """the end pose of (word, seg) from the start pose: plain arc and straight formulas with SIGNED lengths -> x, y, heading (unwrapped)"""
    f = np.asarray(frm, dtype=dtype).reshape(-1, 3)
    x, y, h = f[:, 0].copy(), f[:, 1].copy(), f[:, 2].copy()
    R = dtype(R)
    seg = np.asarray(seg, dtype=dtype)
    for k in range(5):
        sg, ln = TURNS[word, k], seg[:, k]
        nh = h + sg * ln / R
        x = np.where(sg != 0, x + sg * R * (np.sin(nh) - np.sin(h)), x + ln * np.cos(h))
        y = np.where(sg != 0, y - sg * R * (np.cos(nh) - np.cos(h)), y + ln * np.sin(h))
        h = nh
    return x, y, h


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def restate(frm, to, R, dtype=np.float64):
    """-> (totals (n, 48) in metres, inf where a word is infeasible; near (n,): some root / acos argument or sign test within EDGE of its edge)"""
    f, t = np.asarray(frm, dtype=dtype).reshape(-1, 3), np.asarray(to, dtype=dtype).reshape(-1, 3)
    R = dtype(R)
    pi = dtype(4) * np.arctan(dtype(1))
    n = len(f)
    dx, dy = t[:, 0] - f[:, 0], t[:, 1] - f[:, 1]
    c0, s0 = np.cos(f[:, 2]), np.sin(f[:, 2])
    X, Y, PHI = (dx * c0 + dy * s0) / R, (-dx * s0 + dy * c0) / R, t[:, 2] - f[:, 2]
    tot = np.full((n, 48), np.inf, dtype=dtype)
    near = np.zeros(n, dtype=bool)

    def m(a):       # into [-pi, pi]
        v = np.fmod(a, 2 * pi)
        return np.where(v < -pi, v + 2 * pi, np.where(v > pi, v - 2 * pi, v))

    def polar(x, y):
        return np.sqrt(x * x + y * y), np.arctan2(y, x)

    def edge(*vals):
        nonlocal near
        for v in vals:
            a = np.abs(np.asarray(v, dtype=np.float64))
            near |= (a < EDGE) | (np.abs(a - np.pi) < EDGE)

    def put(word, ok, segs):
        total = sum(np.abs(s) for s in segs)
        cur = tot[:, word]
        tot[:, word] = np.where(ok & (total < cur), total, cur)

    with np.errstate(invalid='ignore', divide='ignore'):
        for tr in range(4):
            flip, mirror = tr & 1, tr >> 1
            x, y = (-X if flip else X), (-Y if mirror else Y)
            phi = -PHI if flip != mirror else PHI
            sp, cp = np.sin(phi), np.cos(phi)
            xb, yb = x * cp + y * sp, x * sp - y * cp
            zero = np.zeros(n, dtype=dtype)
            # 8.1 L+S+L+
            u, tt = polar(x - sp, y - 1 + cp)
            v = m(phi - tt)
            edge(tt, v)
            put(0 + tr, (tt >= 0) & (v >= 0), (tt, u, v))
            # 8.2 L+S+R+
            u1, t1 = polar(x + sp, y - 1 - cp)
            a = u1 * u1 - 4
            u = np.sqrt(np.abs(a))
            tt = m(t1 + np.arctan2(dtype(2), u))
            v = m(tt - phi)
            edge(a, tt, v)
            put(4 + tr, (a >= 0) & (tt >= 0) & (v >= 0), (tt, u, v))
            # 8.3 / 8.4 L+R-L(+-), and 8.4 backwards L-R-L+
            for back, (px, py) in enumerate(((x, y), (xb, yb))):
                u1, th = polar(px - sp, py - 1 + cp)
                u = -2 * np.arcsin(np.clip(u1 / 4, -1, 1))
                tt = m(th + u / 2 + pi)
                v = m(phi - tt + u)
                edge(4 - u1, tt, v)
                ok = (u1 <= 4) & (tt >= 0)
                if not back:
                    put(8 + tr, ok & (v >= 0), (tt, u, v))
                    put(12 + tr, ok & (v <= 0), (tt, u, v))
                else:
                    put(16 + tr, ok & (v <= 0), (v, u, tt))
            # 8.7 L+R+L-R-  and  8.8 L+R-L-R+
            xi, eta = x + sp, y - 1 - cp
            rho = (2 + np.sqrt(xi * xi + eta * eta)) / 4
            u = np.arccos(np.clip(rho, -1, 1))
            # (the four circle centres, each 2 from the next: xi + i eta = 2 (2 cos u - 1) e^{i (t - u - pi/2)})
            tt = m(np.arctan2(eta, xi) + pi / 2 + u)
            v = m(tt - 2 * u - phi)
            edge(1 - rho, tt, v)
            put(20 + tr, (rho <= 1) & (tt >= 0) & (v <= 0), (tt, u, u, v))
            rho = (20 - xi * xi - eta * eta) / 16
            u = -np.arccos(np.clip(rho, -1, 1))
            # (xi + i eta = 2 e^{i (t - pi/2)} (2 - e^{i |u|}): the division by (2 - e^{i |u|}) done in complex numbers)
            z = (xi + 1j * eta) / (2 - np.cos(u) + 1j * np.sin(u)) if dtype is np.float64 else None
            if z is None:
                den_r, den_i = 2 - np.cos(u), np.sin(u)            # (longdouble has no complex twin here: the same quotient by hand)
                zr, zi = xi * den_r + eta * den_i, eta * den_r - xi * den_i
            else:
                zr, zi = z.real, z.imag
            tt = m(np.arctan2(zi, zr) + pi / 2)
            v = m(tt - phi)
            edge(rho, 1 - rho, tt, v)
            put(24 + tr, (rho >= 0) & (rho <= 1) & (tt >= 0) & (v >= 0), (tt, u, u, v))
            # 8.9 L+R-S-L-, 8.10 L+R-S-R- and both backwards
            for back, (px, py) in enumerate(((x, y), (xb, yb))):
                rho, th = polar(px - sp, py - 1 + cp)
                a = rho * rho - 4
                r = np.sqrt(np.abs(a))
                u = 2 - r
                tt = m(th + np.arctan2(r, dtype(-2)))
                v = m(phi - pi / 2 - tt)
                edge(a, u, tt, v)
                put((36 if back else 28) + tr, (a >= 0) & (tt >= 0) & (u <= 0) & (v <= 0), (tt, pi / 2 + zero, u, v))
                xi, eta = px + sp, py - 1 - cp
                rho, tt = polar(-eta, xi)
                u = 2 - rho
                v = m(tt + pi / 2 - phi)
                edge(u, tt, v)
                put((40 if back else 32) + tr, (rho >= 2) & (tt >= 0) & (u <= 0) & (v <= 0), (tt, pi / 2 + zero, u, v))
            # 8.11 L+R-S-L-R+
            xi, eta = x + sp, y - 1 - cp
            a = xi * xi + eta * eta - 4
            u = 4 - np.sqrt(np.abs(a))
            tt = m(np.arctan2((4 - u) * xi - 2 * eta, -2 * xi + (u - 4) * eta))
            v = m(tt - phi)
            edge(a, u, tt, v)
            put(44 + tr, (a >= 0) & (u <= 0) & (tt >= 0) & (v >= 0), (tt, pi / 2 + zero, u, pi / 2 + zero, v))
    return tot * R, near


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_five_entries():
    check_entries(ENTRIES)          # (ABI version 5: additions only)


def test_prototypes_bind_them_and_the_library_exports_them():
    protos = {n: (res, args) for n, res, args in L.PROTOTYPES}
    lib = L.load()
    for name, n_args in ENTRIES.items():
        assert name in protos, name
        res, args = protos[name]
        assert res is C.c_int and len(args) == n_args, name
        assert hasattr(lib, name), name
    assert protos['fcpp_rs_solve'][1][8] is C.c_double and protos['fcpp_rs_matrix'][1][9] is C.c_double
    assert protos['fcpp_rs_counts'][1][4] is C.c_double
    assert protos['fcpp_rs_sample'][1][5] is C.c_double and protos['fcpp_rs_sample'][1][8] is C.c_double
    assert lib.fcpp_abi_version() == 5


def test_argument_errors_need_no_device():
    lib = L.load()
    z = np.zeros(8)
    p = z.ctypes.data
    assert lib.fcpp_rs_solve(None, 0, None, None, None, None, None, None, 8.0, None, None, None) == L.EINVAL
    assert lib.fcpp_rs_matrix(None, 0, None, None, None, 0, None, None, None, 8.0, None, None) == L.EINVAL
    assert lib.fcpp_rs_counts(None, 0, None, None, 0.5, None, None) == L.EINVAL
    assert lib.fcpp_rs_sample(None, 0, None, None, None, 8.0, None, None, 0.5, None, 0, None, None, None, None, None, None) == L.EINVAL
    assert lib.fcpp_last_error()
    w = np.zeros(4, dtype=np.int32)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        assert lib.fcpp_debug_rs(1, p, p, p, p, p, p, bad, w.ctypes.data, p, p) == L.EINVAL
    assert lib.fcpp_debug_rs(-1, p, p, p, p, p, p, 8.0, w.ctypes.data, p, p) == L.ESIZE
    assert lib.fcpp_debug_rs(1, None, p, p, p, p, p, 8.0, w.ctypes.data, p, p) == L.EINVAL
    assert lib.fcpp_debug_rs(0, None, None, None, None, None, None, 8.0, None, None, None) == 0
    assert lib.fcpp_debug_rs(1, p, p, p, p, p, p, 8.0, None, None, None) == 0        # every output may be NULL


def test_engine_surface_exists_and_has_no_cpu_fallback():
    import inspect
    for name in ('rs_solve', 'rs_matrix', 'rs_paths'):
        assert callable(getattr(E, name))
    from field_coverage_path_planning_amd import multi_layer_planner_v3 as M
    for fn in (E.BatchResult.drivable_connectors, M.TwoLayerPathPlannerV37.drivable_connectors):
        assert inspect.signature(fn).parameters['reversing'].default is False
    import torch
    if torch.cuda.is_available():       # (with a GPU the calls compute: tests/test_gpu_rs.py)
        return
    a, b = np.array([[0.0, 0.0, 0.0]]), np.array([[10.0, 0.0, 0.0]])
    with pytest.raises(RuntimeError):
        E.rs_solve(a, b, 8.0)
    with pytest.raises(RuntimeError):
        E.rs_matrix(a, b, 8.0)
    with pytest.raises(RuntimeError):
        E.rs_paths(a, b, 8.0, 0.5)


def test_the_table_of_the_header_is_the_one_the_tests_use():
    """include/fcpp.h and csrc/fcpp_rsfn.h both print the twelve base words; they must be the BASES above, in that order."""
    for path in (('include', 'fcpp.h'), ('field_coverage_path_planning_amd', 'csrc', 'fcpp_rsfn.h')):
        text = open(os.path.join(REPO, *path)).read()
        found = {int(b): ''.join(w.split()) for b, w in re.findall(r'base\s+(\d+)\s+((?:[LRS][+-]\s)+)', text)}
        assert found == dict(enumerate(BASES)), (path, found)


# ---- closed forms --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RADII)
def test_straight_ahead_straight_behind_and_goal_equal_to_start(R):
    """The goal on the start's heading line with the same heading, d ahead: any path is at least as long as the chord d, and the straight
    attains it, forward.  The goal d BEHIND: the same straight in reverse gear (one negative segment).  Goal == start: nothing to drive."""
    # (oblique headings far from the origin: ox + d cos h rounds to ulp(ox), so the goal lies up to 1e-12 m beside the heading line; the
    #  shortest path is then the straight with two arcs of ~1e-11 rad, d + O(1e-10) m long -- still d within P_TOL, and still one gear.  Below
    #  d ~ 1 mm that rounding alone asks for a wiggle longer than d, so smaller d are not the closed form)
    for d in (0.001, 0.01, 0.05, 1.0, 3.2, 2 * R, 1234.5):
        for h, ox, oy in ((0.0, 100.0, 200.0), (0.7, 100.0, 200.0), (-2.9, 100.0, 200.0), (np.pi, 100.0, 200.0), (2.2, 4096.0, 17.0),
                          (1.1, 3000.0, 3999.0), (0.7, 0.0, 0.0)):
            for sgn in (1.0, -1.0):
                f = np.array([[ox, oy, h]])
                t = np.array([[ox + sgn * d * np.cos(h), oy + sgn * d * np.sin(h), h]])
                w, seg, tot = host_solve(f, t, R)
                assert abs(tot[0] - d) <= P_TOL, (d, h, sgn, tot)
                assert abs(seg[0].sum() - sgn * d) <= P_TOL          # signed: forward ahead, reverse behind
                assert (np.sign(seg[0][seg[0] != 0]) == sgn).all(), (d, h, sgn, w, seg)      # one gear: no cusp
    w, seg, tot = host_solve([[0, 0, 0]], [[7.25, 0, 0]], R)
    assert w[0] == 0 and tuple(seg[0]) == (0.0, 7.25, 0.0, 0.0, 0.0) and tot[0] == 7.25          # (axis-aligned: exact)
    w, seg, tot = host_solve([[0, 0, 0]], [[-7.25, 0, 0]], R)
    assert w[0] == 1 and tuple(seg[0]) == (0.0, -7.25, 0.0, 0.0, 0.0) and tot[0] == 7.25         # word 0 under the flip: L- S- L-
    assert not np.signbit(seg[0][[0, 2, 3, 4]]).any()                                              # the zeros are +0
    w, seg, tot = host_solve([[12.5, -3.0, 1.25]], [[12.5, -3.0, 1.25]], R)
    assert w[0] == 0 and not seg.any() and tot[0] == 0.0
    hs = np.linspace(-np.pi, np.pi, 1001)
    p = np.column_stack((np.full_like(hs, 4321.0), np.full_like(hs, 17.0), hs))
    w, seg, tot = host_solve(p, p, R)
    assert not tot.any() and not w.any() and not seg.any()


@pytest.mark.parametrize('R', RADII)
def test_about_turn_on_the_spot_is_the_three_point_turn(R):
    """(0, 0, 0) -> (0, 0, pi).  |dh/ds| <= 1/R along any path, so turning the heading by pi takes at least pi R of path.  The three-point
    turn L+(a) R-(a) L+(a) turns the heading by +a each time (a reverse right arc turns it counter-clockwise too): 3a = pi, a = pi/3, total
    pi R -- it attains the bound.  It closes: the L circle of the start is centred (0, R), the R circle after the first arc lies at distance
    2R from it at angle a - pi/2 = -pi/6, the last L circle at 2R from that at angle 2a + pi/2 = 7pi/6: 2R (cos(-pi/6) + cos(7pi/6)) = 0
    and 2R (sin(-pi/6) + sin(7pi/6)) = -2R, so the last centre is (0, -R) -- the L centre of the goal pose (0, 0, pi).  The mirror image
    R+ L- R+ and both flips have the same length; the lowest word wins: 8 = base 2 (L+R-L+), no flip, no mirror."""
    w, seg, tot = host_solve([[0, 0, 0]], [[0, 0, np.pi]], R)
    assert abs(tot[0] - np.pi * R) <= P_TOL
    assert w[0] == 8, w
    assert np.abs(seg[0] - R * np.pi / 3 * np.array([1, -1, 1, 0, 0])).max() <= P_TOL


def test_swath_to_swath_turn_reverses_and_beats_dubins():
    """(0, 0, 0) -> (0, W, pi) with W < 2R.  The heading turns by pi: total >= pi R.  The forward-only path is the RLR loop of length
    R (pi + 4 acos((W + 2R) / 4R)) > pi R (tests/test_dubins_host.py derives it); a reversing vehicle does better, so the shortest path has
    a cusp.  The mirror image (0, -W, pi) has the same length."""
    for W, R in ((3.2, 8.0), (3.2, 2.0), (10.0, 25.0), (1.0, 8.0)):
        f, t = [[0, 0, 0]], [[0, W, np.pi]]
        w, seg, tot = host_solve(f, t, R)
        dub = dubins_total(f, t, R)
        assert tot[0] >= np.pi * R - P_TOL and tot[0] < dub[0] - 1e-3, (W, R, tot, dub)
        sg = np.sign(seg[0][seg[0] != 0])
        assert (sg[1:] != sg[:-1]).sum() >= 1                       # at least one cusp
        x, y, h = integrate(f, R, w, seg)
        assert abs(x[0]) <= P_TOL and abs(y[0] - W) <= P_TOL and abs(wrap(np.float64(h[0]) - np.pi)) <= H_TOL
        w2, seg2, tot2 = host_solve(f, [[0, -W, np.pi]], R)
        assert abs(tot2[0] - tot[0]) <= P_TOL
        print(f'W = {W} R = {R}: RS {tot[0]:.6f} m (pi R = {np.pi * R:.6f}), Dubins {dub[0]:.6f} m, word {w[0]} = {BASES[w[0] >> 2]}')


def test_non_finite_pairs_are_nan_per_pair():
    f = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, np.nan], [0, 0, 0], [0, 0, 0], [5.0, 5.0, 1.0]], dtype=np.float64)
    t = np.array([[10, 0, 0], [10, 0, 0], [10, 0, 0], [10, 0, 0], [10, -np.inf, 0], [10, 0, np.inf], [9.0, 5.0, 1.0]], dtype=np.float64)
    w, seg, tot = host_solve(f, t, 8.0)
    assert list(w) == [0, -1, -1, -1, -1, -1, w[6]] and w[6] >= 0
    assert np.isnan(tot[1:6]).all() and np.isnan(seg[1:6]).all()
    assert tot[0] == 10.0 and np.isfinite(tot[6]) and np.isfinite(seg[[0, 6]]).all()


# ---- properties over random pairs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('near', [False, True])
@pytest.mark.parametrize('R', RADII)
def test_chosen_word_closes_is_consistent_and_bounded(R, near):
    rng = np.random.default_rng(1)
    frm, to = random_pairs(rng, N_RANDOM, R, near)
    w, seg, tot = host_solve(frm, to, R)
    assert ((w >= 0) & (w < 48)).all()
    # closure
    x, y, h = integrate(frm, R, w, seg)
    ex, ey, eh = np.abs(x - to[:, 0]).max(), np.abs(y - to[:, 1]).max(), np.abs(wrap((h - to[:, 2]).astype(np.float64))).max()
    print(f'R = {R} near = {near}: closure {ex:.2e} {ey:.2e} m, {eh:.2e} rad; bases won {np.bincount(w >> 2, minlength=12)}')
    assert ex <= P_TOL and ey <= P_TOL and eh <= H_TOL
    # segment consistency
    a = np.abs(seg)
    assert np.array_equal(tot, (((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]) + a[:, 4])
    assert (seg[np.arange(5)[None, :] >= N_SEG[w][:, None]] == 0).all()
    assert (a[TURNS[w] != 0] <= np.pi * R).all()
    nz = seg != 0
    assert (np.sign(seg)[nz] == GEARS[w][nz]).all()                 # the sign of a segment is the table's gear
    # lower bounds
    assert (tot >= np.hypot(to[:, 0] - frm[:, 0], to[:, 1] - frm[:, 1]) - P_TOL).all()
    assert (tot >= R * np.abs(wrap(to[:, 2] - frm[:, 2])) - P_TOL).all()
    # upper bounds: the forward-only path, and the forward-only path of the vehicle turned round (driven all in reverse)
    turned = lambda p: np.column_stack((p[:, 0], p[:, 1], p[:, 2] + np.pi))
    d_fwd, d_rev = dubins_total(frm, to, R), dubins_total(turned(frm), turned(to), R)
    assert (tot <= d_fwd + P_TOL).all() and (tot <= d_rev + P_TOL).all()
    if near:
        assert (np.bincount(w >> 2, minlength=12) > 0).all()        # every base word is exercised


@pytest.mark.parametrize('near', [False, True])
@pytest.mark.parametrize('R', RADII)
def test_restatement_agrees(R, near):
    rng = np.random.default_rng(3)
    frm, to = random_pairs(rng, N_RANDOM, R, near)
    w, seg, tot = host_solve(frm, to, R)
    for dtype in (np.float64, np.longdouble):
        cand, edge = restate(frm, to, R, dtype)
        cand = cand.astype(np.float64)
        assert (tot[:, None] <= cand + P_TOL).all(), dtype
        n_edge = int(edge.sum())
        print(f'R = {R} near = {near} {np.dtype(dtype).name}: {n_edge} of {len(tot)} pairs within {EDGE} of a domain edge')
        assert n_edge <= FRAGILE_CAP * len(tot)
        diff = np.abs(tot - cand.min(1))[~edge]
        assert diff.max() <= P_TOL, (dtype, diff.max())
        # ties go to the lowest word: no lower word is shorter than the winner by more than the tolerance
        lower = np.where(np.arange(48)[None, :] < w[:, None], cand, np.inf).min(1)
        assert (lower >= tot - P_TOL).all()


@pytest.mark.parametrize('R', RADII)
def test_length_is_a_metric(R):
    rng = np.random.default_rng(5)
    worst_sym, tight = 0.0, np.inf
    for near in (False, True):
        a, c = random_pairs(rng, N_RANDOM, R, near)
        d_ac, d_ca = host_solve(a, c, R)[2], host_solve(c, a, R)[2]
        worst_sym = max(worst_sym, np.abs(d_ac - d_ca).max())
        assert np.abs(d_ac - d_ca).max() <= P_TOL
        # detours: b anywhere, b near a, b near c, b on the way
        n = len(a)
        def around(p):
            r, ang = rng.uniform(0, 4 * R, n), rng.uniform(-np.pi, np.pi, n)
            return np.column_stack((p[:, 0] + r * np.cos(ang), p[:, 1] + r * np.sin(ang), rng.uniform(-np.pi, np.pi, n)))
        lam = rng.uniform(0, 1, n)[:, None]
        mid = around(a * (1 - lam) + c * lam)
        for b in (random_pairs(rng, n, R, False)[0], around(a), around(c), mid):
            slack = host_solve(a, b, R)[2] + host_solve(b, c, R)[2] - d_ac
            tight = min(tight, slack.min())
            assert (slack >= -3 * P_TOL).all(), (near, slack.min())
    print(f'R = {R}: |d(a,b) - d(b,a)| <= {worst_sym:.2e} m; tightest triangle slack {tight:.3e} m')


@pytest.mark.parametrize('near', [False, True])
@pytest.mark.parametrize('R', RADII)
def test_invariance_under_rigid_motion_mirroring_and_time_flip(R, near):
    rng = np.random.default_rng(2)
    frm, to = random_pairs(rng, N_RANDOM, R, near)
    w, seg, tot = host_solve(frm, to, R)
    srt = np.sort(restate(frm, to, R)[0].astype(np.float64), 1)
    clear = srt[:, 1] - srt[:, 0] > 1e-6             # the two shortest candidates differ: the word is determined

    def moved(p, ang, tx, ty):
        c, s = np.cos(ang), np.sin(ang)
        return np.column_stack((c * p[:, 0] - s * p[:, 1] + tx, s * p[:, 0] + c * p[:, 1] + ty, p[:, 2] + ang))
    for ang, tx, ty in ((0.0, 1000.0, -2000.0), (1.0, 0.0, 0.0), (-2.5, 300.0, 700.0)):
        w2, _, tot2 = host_solve(moved(frm, ang, tx, ty), moved(to, ang, tx, ty), R)
        assert np.abs(tot2 - tot).max() <= P_TOL, (ang, np.abs(tot2 - tot).max())
        assert np.array_equal(w2[clear], w[clear])
    # mirroring in the x axis: L <-> R, word ^ 2
    mir = lambda p: np.column_stack((p[:, 0], -p[:, 1], -p[:, 2]))
    w3, seg3, tot3 = host_solve(mir(frm), mir(to), R)
    assert np.abs(tot3 - tot).max() <= P_TOL
    assert np.array_equal(w3[clear], w[clear] ^ 2)
    assert np.abs(seg3 - seg)[clear].max() <= P_TOL
    # time-flip: the goal mirrored in the start's lateral axis (x -> -x, phi -> -phi in the start frame): every gear reversed, word ^ 1
    c0, s0 = np.cos(frm[:, 2]), np.sin(frm[:, 2])
    dx, dy = to[:, 0] - frm[:, 0], to[:, 1] - frm[:, 1]
    lx, ly = dx * c0 + dy * s0, -dx * s0 + dy * c0
    flipped = np.column_stack((frm[:, 0] - lx * c0 - ly * s0, frm[:, 1] - lx * s0 + ly * c0, 2 * frm[:, 2] - to[:, 2]))
    w4, seg4, tot4 = host_solve(frm, flipped, R)
    assert np.abs(tot4 - tot).max() <= P_TOL
    assert np.array_equal(w4[clear], w[clear] ^ 1)
    assert np.abs(seg4 + seg)[clear].max() <= P_TOL
    print(f'R = {R} near = {near}: words compared on {clear.mean():.4f} of the pairs')
