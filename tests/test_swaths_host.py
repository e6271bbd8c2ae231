"""CPU-side tests of the polygon swaths: the four entries exist (header, ctypes binding, libfcpp.so; ABI version still 5), argument errors
need no device -- and the RULE, through fcpp_debug_swaths (csrc/fcpp_swathfn.h on the host: the very expressions the kernels run).

The checker is a numpy restatement of the rule written here from its statement in include/fcpp.h: the same fl() expressions, cos / sin from
numpy, the line count by a plain loop, the crossings of a line sorted with lexsort on (u, ring, edge).  It shares no code with the library.
Beside it stand answers known by hand at theta = 0 (where sine and cosine are exact), and properties that need no formula: every line
crosses every closed ring an even number of times, W x the summed length approaches the area, a rotated field has the same swaths.

Tolerances come from the project, not from what the code gives: end points and lengths 1e-9 m (tests/test_dubins_host.py; coordinates here
stay below 1e3 m and a crossing is three operations).  numpy's sin / cos may differ from the library's by an ulp, so a COUNT may differ only
where a vertex lies within an ulp of a line; the random cases below have no such knife edge (test_restatement_has_no_knife_edge asserts the
margin), the hand-made ones are used at theta = 0 or checked through rotation-invariant quantities."""
import ctypes as C
import re

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.support import check_entries, lib, p as _p          # noqa: F401 (lib: a fixture)

P_TOL = 1e-9
MAX_CROSSINGS = 64
THETAS = (0.0, 0.3, 1.1, 2.5)
WIDTHS = (3.2, 1.0, 0.37)

ENTRIES = {'fcpp_swath_scores': 17, 'fcpp_swath_counts': 16, 'fcpp_swath_fill': 20, 'fcpp_debug_swaths': 25}

RECT = [(0, 0), (10, 0), (10, 4), (0, 4)]
ELL = [(0, 0), (60, 0), (60, 20), (25, 20), (25, 50), (0, 50)]
HOLE = [(10, 5), (20, 5), (20, 15), (10, 15)]


def comb(teeth):
    """teeth of 10 m on a base of 10 m: (0,0) (W,0) (W,40) (W-10,40) (W-10,10) (W-20,10) (W-20,40) ... (10,40) (0,40)"""
    x = 10.0 * (2 * teeth - 1)
    pts = [(0.0, 0.0), (x, 0.0)]
    for t in range(teeth):
        pts += [(x, 40.0), (x - 10.0, 40.0)]
        x -= 10.0
        if t < teeth - 1:
            pts += [(x, 10.0), (x - 10.0, 10.0)]
            x -= 10.0
    return pts


COMB = comb(4)
OVER_COMB = comb(MAX_CROSSINGS // 2 + 8)          # 80 crossings on a line through the teeth


def star(seed, m):
    rng = np.random.default_rng(seed)
    a = np.sort(rng.uniform(0.0, 2.0 * np.pi, m))
    r = rng.uniform(40.0, 120.0, m)
    return np.column_stack([300.0 + r * np.cos(a), -120.0 + r * np.sin(a)])


def rings_of(field):
    """a field is an (m, 2) array / vertex list, or a list of rings -> list of (m, 2) float64 arrays"""
    if isinstance(field, np.ndarray) and field.ndim == 2:
        return [np.asarray(field, dtype=np.float64)]
    if len(field) and np.ndim(field[0]) == 1 and len(field[0]) == 2 and np.ndim(field[0][0]) == 0:
        return [np.asarray(field, dtype=np.float64).reshape(-1, 2)]
    return [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in field]


def pack(fields):
    ro, vo, xs, ys = [0], [0], [], []
    for f in fields:
        for r in rings_of(f):
            xs.append(r[:, 0])
            ys.append(r[:, 1])
            vo.append(vo[-1] + len(r))
        ro.append(len(vo) - 1)
    cat = lambda a: np.ascontiguousarray(np.concatenate(a)) if a else np.zeros(0)
    return np.asarray(ro, dtype=np.int64), np.asarray(vo, dtype=np.int64), cat(xs), cat(ys)


def host_scores(fields, angles, W, first=None, min_length=0.0, expect=0):
    """fcpp_debug_swaths, the angle list shared -> dict of (n, A) arrays"""
    lib = L.load()
    ro, vo, x, y = pack(fields)
    ang = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
    n, A = len(ro) - 1, len(ang)
    out = dict(n_swaths=np.full((n, A), -7, np.int32), n_lines=np.full((n, A), -7, np.int32), length=np.full((n, A), np.nan),
               status=np.full((n, A), -7, np.int32))
    rc = lib.fcpp_debug_swaths(n, _p(ro), len(vo) - 1, _p(vo), len(x), _p(x), _p(y), A, _p(ang), 0, float(W), float(W / 2 if first is None else first),
                               float(min_length), _p(out['n_swaths']), _p(out['n_lines']), _p(out['length']), _p(out['status']), None, 0,
                               None, None, None, None, None, None)
    assert rc == expect, lib.fcpp_last_error()
    return out


def host_cut(fields, angle, W, first=None, min_length=0.0):
    """fcpp_debug_swaths, an angle per field (or one for all) -> dict: offsets, a, b (m, 2), line, length (per swath), and per field n_swaths,
    n_lines, total, status"""
    lib = L.load()
    ro, vo, x, y = pack(fields)
    n = len(ro) - 1
    ang = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), (n,)))
    first = float(W / 2 if first is None else first)
    out = dict(n_swaths=np.zeros(n, np.int32), n_lines=np.zeros(n, np.int32), total=np.zeros(n), status=np.zeros(n, np.int32),
               offsets=np.zeros(n + 1, np.int64))
    head = (n, _p(ro), len(vo) - 1, _p(vo), len(x), _p(x), _p(y), 1, _p(ang), 1, float(W), first, float(min_length))
    rc = lib.fcpp_debug_swaths(*head, _p(out['n_swaths']), _p(out['n_lines']), _p(out['total']), _p(out['status']), _p(out['offsets']), 0,
                               None, None, None, None, None, None)
    assert rc == 0, lib.fcpp_last_error()
    m = int(out['offsets'][-1])
    rec = {k: np.full(m, np.nan) for k in ('ax', 'ay', 'bx', 'by', 'length')}
    rec['line'] = np.full(m, -1, np.int32)
    off2 = np.zeros(n + 1, np.int64)
    rc = lib.fcpp_debug_swaths(*head, None, None, None, None, _p(off2), m, _p(rec['ax']), _p(rec['ay']), _p(rec['bx']), _p(rec['by']),
                               _p(rec['line']), _p(rec['length']))
    assert rc == 0 and np.array_equal(off2, out['offsets'])
    out.update(rec)
    out['a'] = np.column_stack([rec['ax'], rec['ay']])
    out['b'] = np.column_stack([rec['bx'], rec['by']])
    return out


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def ref_swaths(field, theta, W, first=None, min_length=0.0):
    """The rule in numpy -> dict: K, line (m,), ua, ub, a (m, 2), b (m, 2), length (m,), crossings (per line), margin (the least distance of
    a vertex from a line, in w)"""
    first = W / 2 if first is None else first
    c, s = np.cos(np.float64(theta)), np.sin(np.float64(theta))
    up, wp, uq, wq, ring, edge = [], [], [], [], [], []
    for ri, r in enumerate(rings_of(field)):
        u = r[:, 0] * c + r[:, 1] * s
        w = -r[:, 0] * s + r[:, 1] * c
        up.append(u); wp.append(w); uq.append(np.roll(u, -1)); wq.append(np.roll(w, -1))
        ring.append(np.full(len(r), ri)); edge.append(np.arange(len(r)))
    up, wp, uq, wq, ring, edge = (np.concatenate(a) for a in (up, wp, uq, wq, ring, edge))
    w_min, w_max = wp.min(), wp.max()
    base = w_min + np.float64(first)
    K = 0
    while base + np.float64(K) * np.float64(W) < w_max:
        K += 1
    line, ua, ub, crossings, margin = [], [], [], [], np.inf
    for k in range(K):
        wk = base + np.float64(k) * np.float64(W)
        margin = min(margin, np.abs(wp - wk).min())
        m = (wp <= wk) != (wq <= wk)
        u = up[m] + (wk - wp[m]) / (wq[m] - wp[m]) * (uq[m] - up[m])
        u = u[np.lexsort((edge[m], ring[m], u))]
        crossings.append(len(u))
        for j in range(0, len(u) - 1, 2):
            if u[j + 1] - u[j] > min_length:
                line.append(k); ua.append(u[j]); ub.append(u[j + 1])
    line, ua, ub = np.asarray(line, dtype=np.int64), np.asarray(ua, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    wl = base + line.astype(np.float64) * np.float64(W)
    return dict(K=K, line=line, ua=ua, ub=ub, length=ub - ua, crossings=np.asarray(crossings, dtype=np.int64), margin=margin,
                a=np.column_stack([ua * c - wl * s, ua * s + wl * c]), b=np.column_stack([ub * c - wl * s, ub * s + wl * c]))


def area_perimeter(field):
    """even-odd area of well-nested rings (outer minus holes) and the perimeter of all rings"""
    area, per = 0.0, 0.0
    for i, r in enumerate(rings_of(field)):
        x, y = r[:, 0], r[:, 1]
        a = 0.5 * abs(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
        area += a if i == 0 else -a
        per += np.sum(np.hypot(np.roll(x, -1) - x, np.roll(y, -1) - y))
    return area, per


def rotated(field, phi):
    c, s = np.cos(phi), np.sin(phi)
    return [np.column_stack([r[:, 0] * c - r[:, 1] * s, r[:, 0] * s + r[:, 1] * c]) for r in rings_of(field)]


SHAPES = {'rect': RECT, 'ell': ELL, 'ell_hole': [ELL, HOLE], 'comb': COMB}
STARS = {'star7': star(7, 7), 'star300': star(300, 300)}


# ---- the entries exist ------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported(lib):
    header = check_entries(ENTRIES, lib)
    assert re.search(r'#define FCPP_SWATH_MAX_CROSSINGS %d\b' % MAX_CROSSINGS, header)
    for name in ('polygon_fields', 'swath_scores', 'best_swath_angle', 'polygon_swaths', 'swath_route', 'SwathSet'):
        assert hasattr(E, name), name


# ---- answers known by hand, theta = 0 -----------------------------------------------------------------------------------------------------
def _segments(cut, i=0):
    sl = slice(cut['offsets'][i], cut['offsets'][i + 1])
    return [(int(k), float(a), float(b)) for k, a, b in zip(cut['line'][sl], cut['ax'][sl], cut['bx'][sl])]


def test_rectangle_known_answer():
    cut = host_cut([RECT], 0.0, 1.0, first=0.5)
    assert cut['status'][0] == 0 and cut['n_lines'][0] == 4 and cut['n_swaths'][0] == 4
    assert _segments(cut) == [(k, 0.0, 10.0) for k in range(4)]
    assert np.array_equal(cut['ay'], [0.5, 1.5, 2.5, 3.5]) and np.array_equal(cut['by'], cut['ay'])
    assert np.array_equal(cut['length'], [10.0] * 4) and cut['total'][0] == 40.0


def test_ell_known_answer_lines_through_vertices_and_along_edges():
    cut = host_cut([ELL], 0.0, 5.0, first=0.0)
    assert cut['status'][0] == 0 and cut['n_lines'][0] == 10 and cut['n_swaths'][0] == 10
    assert _segments(cut) == [(k, 0.0, 60.0) for k in range(4)] + [(k, 0.0, 25.0) for k in range(4, 10)]
    assert np.array_equal(cut['ay'], 5.0 * np.arange(10))


def test_ell_with_hole_known_answer():
    cut = host_cut([[ELL, HOLE]], 0.0, 5.0, first=0.0)
    assert cut['status'][0] == 0 and cut['n_lines'][0] == 10 and cut['n_swaths'][0] == 12
    seg = _segments(cut)
    assert [s for s in seg if s[0] == 1] == [(1, 0.0, 10.0), (1, 20.0, 60.0)]
    assert [s for s in seg if s[0] == 2] == [(2, 0.0, 10.0), (2, 20.0, 60.0)]
    assert [s for s in seg if s[0] == 3] == [(3, 0.0, 60.0)]                      # y = 15 lies along the hole's top edge: one piece
    # either orientation of either ring: the same swaths
    flipped = host_cut([[ELL[::-1], HOLE]], 0.0, 5.0, first=0.0)
    assert _segments(flipped) == seg
    assert _segments(host_cut([[ELL, HOLE[::-1]]], 0.0, 5.0, first=0.0)) == seg


def test_comb_known_answer():
    cut = host_cut([COMB], 0.0, 5.0, first=0.0)
    assert cut['status'][0] == 0 and cut['n_lines'][0] == 8 and cut['n_swaths'][0] == 26
    seg = _segments(cut)
    assert [s for s in seg if s[0] == 2] == [(2, 0.0, 10.0), (2, 20.0, 30.0), (2, 40.0, 50.0), (2, 60.0, 70.0)]
    assert [s for s in seg if s[0] < 2] == [(0, 0.0, 70.0), (1, 0.0, 70.0)]


# ---- the restatement: parity, no knife edge; the library against it ---------------------------------------------------------------------------
CASES = [(name, th, W) for name in list(SHAPES) + list(STARS) for th in THETAS for W in WIDTHS]


@pytest.fixture(scope='module')
def reference():
    """the restatement on every case, computed once and left unchanged"""
    both = dict(SHAPES, **STARS)
    return {(name, th, W): ref_swaths(both[name], th, W) for name, th, W in CASES}


def test_restatement_every_line_has_an_even_number_of_crossings(reference):
    for key, ref in reference.items():
        assert np.all(ref['crossings'] % 2 == 0), key
        assert np.all(ref['crossings'] <= MAX_CROSSINGS), key


def test_restatement_has_no_knife_edge(reference):
    """no vertex of a star lies within 1e-9 m of a line (an ulp of sin / cos moves w by ~1e-13 m), so the counts cannot hinge on whose
    sine it is; first = W / 2 keeps the lines off w_min"""
    for (name, th, W), ref in reference.items():
        if name in STARS:
            assert ref['margin'] > 1e-9, (name, th, W, ref['margin'])


def test_host_agrees_with_the_restatement(reference):
    both = dict(SHAPES, **STARS)
    for th in THETAS:
        for W in WIDTHS:
            names = [n for n in both if n in STARS or th == 0.0 or reference[(n, th, W)]['margin'] > 1e-9]
            cut = host_cut([both[n] for n in names], th, W)
            for i, name in enumerate(names):
                ref = reference[(name, th, W)]
                sl = slice(cut['offsets'][i], cut['offsets'][i + 1])
                assert cut['status'][i] == 0 and cut['n_lines'][i] == ref['K'], (name, th, W)
                assert cut['n_swaths'][i] == len(ref['line']) == sl.stop - sl.start, (name, th, W)
                assert np.array_equal(cut['line'][sl], ref['line']), (name, th, W)
                assert np.abs(cut['a'][sl] - ref['a']).max() <= P_TOL and np.abs(cut['b'][sl] - ref['b']).max() <= P_TOL, (name, th, W)
                assert np.abs(cut['length'][sl] - ref['length']).max() <= P_TOL, (name, th, W)
                # the sum: any order of m non-negative terms lies within 2 (m - 1) 2^-53 of any other, plus the terms' own tolerance
                m = len(ref['line'])
                assert abs(cut['total'][i] - ref['length'].sum()) <= m * P_TOL + 2 * m * 2.0 ** -53 * ref['length'].sum(), (name, th, W)


def test_per_line_counts_are_pairs_of_the_crossings(reference):
    """with min_length = 0 a line of 2 p crossings gives at most p swaths, and exactly p where no two crossings coincide"""
    for name in STARS:
        for th in THETAS:
            ref = reference[(name, th, 3.2)]
            cut = host_cut([STARS[name]], th, 3.2)
            per_line = np.bincount(cut['line'], minlength=ref['K'])
            assert np.array_equal(per_line, ref['crossings'] // 2), (name, th)


# ---- area ------------------------------------------------------------------------------------------------------------------------------------
def test_area_bound():
    """first = W / 2: |W * sum(length) - area| <= perimeter * W (holes included in the perimeter): a condition, not a tolerance"""
    fields = dict(SHAPES, star300=STARS['star300'])
    for th in THETAS:
        for W in WIDTHS:
            sc = host_scores(list(fields.values()), [th], W)
            for i, (name, f) in enumerate(fields.items()):
                area, per = area_perimeter(f)
                assert sc['status'][i, 0] == 0
                assert abs(W * sc['length'][i, 0] - area) <= per * W, (name, th, W, W * sc['length'][i, 0], area)


# ---- rotation ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('phi', [0.7, 2.0])
def test_rotation_invariance(phi):
    th, W, first = 0.3, 3.2, 1.6
    base = host_cut(list(SHAPES.values()), th, W, first)
    rot = host_cut([rotated(f, phi) for f in SHAPES.values()], th + phi, W, first)
    assert np.array_equal(base['n_lines'], rot['n_lines']) and np.array_equal(base['n_swaths'], rot['n_swaths'])
    assert np.array_equal(base['line'], rot['line'])
    assert np.abs(base['length'] - rot['length']).max() <= P_TOL


# ---- filters and statuses ----------------------------------------------------------------------------------------------------------------------
def test_min_length_drops_the_teeth():
    cut = host_cut([COMB], 0.0, 5.0, first=0.0, min_length=12.0)
    assert cut['n_lines'][0] == 8 and _segments(cut) == [(0, 0.0, 70.0), (1, 0.0, 70.0)]
    assert len(_segments(host_cut([COMB], 0.0, 5.0, first=0.0, min_length=10.0))) == 2          # strictly longer
    assert len(_segments(host_cut([COMB], 0.0, 5.0, first=0.0, min_length=9.999))) == 26


def test_statuses_leave_the_neighbours_alone():
    nan_field = np.array(ELL, dtype=np.float64)
    nan_field[2, 1] = np.nan
    two = [ELL, [(1.0, 1.0), (2.0, 2.0)]]
    alone = host_cut([ELL, [ELL, HOLE], COMB], 0.0, 5.0, first=0.0)
    mixed = host_cut([ELL, OVER_COMB, [ELL, HOLE], nan_field, two, COMB], 0.0, 5.0, first=0.0)
    assert mixed['status'].tolist() == [0, L.EUNSUPPORTED, 0, L.EINVAL, L.EINVAL, 0]
    for i in (1, 3, 4):
        assert mixed['n_swaths'][i] == 0 and mixed['n_lines'][i] == 0 and mixed['total'][i] == 0.0
        assert mixed['offsets'][i + 1] == mixed['offsets'][i]
    for i, j in ((0, 0), (1, 2), (2, 5)):
        assert _segments(alone, i) == _segments(mixed, j)
        assert alone['total'][i] == mixed['total'][j]
    # the over-cap comb is fine at a width whose only line stays in the base
    assert host_cut([OVER_COMB], 0.0, 39.0, first=5.0)['status'][0] == 0
    assert host_scores([OVER_COMB], [0.0], 5.0, first=0.0)['status'][0, 0] == L.EUNSUPPORTED
    # exactly the cap passes: 32 teeth are 64 crossings
    at_cap = host_cut([comb(MAX_CROSSINGS // 2)], 0.0, 5.0, first=0.0)
    assert at_cap['status'][0] == 0 and at_cap['n_swaths'][0] == 2 + 6 * (MAX_CROSSINGS // 2)


def test_degenerate_fields():
    thin = [(0.0, 0.0), (50.0, 0.0), (50.0, 1.0), (0.0, 1.0)]
    cut = host_cut([thin, thin, []], 0.0, 3.2, first=1.6)
    assert cut['n_lines'].tolist()[:2] == [0, 0] and cut['status'].tolist() == [0, 0, L.EINVAL]        # narrower than `first`: no line
    one = host_cut([thin], 0.0, 3.2, first=0.5)
    assert one['n_lines'][0] == 1 and _segments(one) == [(0, 0.0, 50.0)]


def test_argument_errors(lib):
    ro, vo, x, y = pack([ELL])
    ang = np.zeros(1)
    ns = np.zeros(1, np.int32)

    def call(n=1, ro=ro, nr=1, vo=vo, nv=6, x=x, y=y, A=1, ang=ang, W=5.0, first=0.0, min_length=0.0):
        return lib.fcpp_debug_swaths(n, _p(ro), nr, _p(vo), nv, _p(x), _p(y), A, _p(ang), 0, W, first, min_length, _p(ns), None, None, None, None, 0,
                                     None, None, None, None, None, None)
    assert call() == 0
    for kw in (dict(W=0.0), dict(W=-1.0), dict(W=np.inf), dict(W=np.nan), dict(first=5.0), dict(first=-0.1), dict(first=np.nan),
               dict(min_length=-1.0), dict(min_length=np.inf), dict(min_length=np.nan), dict(ang=np.array([np.nan])),
               dict(ang=np.array([np.inf])), dict(ro=None), dict(vo=None), dict(x=None), dict(ang=None)):
        assert call(**kw) == L.EINVAL, kw
    for kw in (dict(n=-1), dict(nr=-1), dict(nv=-1), dict(A=-1), dict(ro=np.array([1, 1], np.int64)), dict(ro=np.array([0, 2], np.int64)),
               dict(vo=np.array([0, 5], np.int64)), dict(vo=np.array([0, 7], np.int64)), dict(nv=7),
               dict(n=2, ro=np.array([0, 1, 0], np.int64)), dict(nr=2, vo=np.array([0, 7, 6], np.int64), ro=np.array([0, 2], np.int64))):
        assert call(**kw) == L.ESIZE, kw
    # the device entries check the same things before they touch a device: a NULL context first
    assert lib.fcpp_swath_scores(None, 1, None, 1, None, 6, None, None, 1, None, 5.0, 0.0, 0.0, None, None, None, None) == L.EINVAL
    assert lib.fcpp_swath_counts(None, 1, None, 1, None, 6, None, None, None, 5.0, 0.0, 0.0, None, None, None, None) == L.EINVAL
    assert lib.fcpp_swath_fill(None, 1, None, 1, None, 6, None, None, None, 5.0, 0.0, 0.0, None, 0, None, None, None, None, None, None) == L.EINVAL


# ---- consistency: the scores are the cut's counts ----------------------------------------------------------------------------------------------
def test_scores_equal_the_cut():
    fields = [ELL, [ELL, HOLE], COMB, STARS['star7'], STARS['star300'], OVER_COMB, RECT]
    angles = np.array([0.0, 0.3, 1.1, 2.5, -0.9, 3.1])
    sc = host_scores(fields, angles, 3.2, first=1.0, min_length=2.0)
    for j, th in enumerate(angles):
        cut = host_cut(fields, th, 3.2, first=1.0, min_length=2.0)
        assert np.array_equal(sc['n_swaths'][:, j], cut['n_swaths']) and np.array_equal(sc['n_lines'][:, j], cut['n_lines'])
        assert np.array_equal(sc['status'][:, j], cut['status'])
        assert np.array_equal(sc['length'][:, j].view(np.int64), cut['total'].view(np.int64))
        assert np.array_equal(np.diff(cut['offsets']), cut['n_swaths'])
        # the total against the records: the stated order is ONE order of these terms
        for i in range(len(fields)):
            sl = slice(cut['offsets'][i], cut['offsets'][i + 1])
            m, tot = sl.stop - sl.start, cut['length'][sl].sum()
            assert abs(cut['total'][i] - tot) <= 2 * max(m - 1, 0) * 2.0 ** -53 * tot

