"""CPU-side tests of the PRICED transit block: the entries exist, argument errors need no device -- and the RULE, through
fcpp_debug_route_transit_priced (priced_transit of csrc/fcpp_solveclearfn.h on the host: the expressions the kernels run).

  * composition: the twin equals, byte for byte, the block put together here from the EXISTING twins -- fcpp_debug_route_transit for the
    entries within one swath, fcpp_debug_conn_solve_clear on every canonical pair's poses for the rest: len where rank >= 0, len + penalty
    where it is -1, written to both mirrored entries, K likewise -- and the four consequences the rule text names hold against
    fcpp_debug_route_transit and fcpp_debug_route_transit_clear;
  * recorded figures: what the router (fcpp_debug_route, S = 8) drives WITH RESHAPING on the penalty matrix and on the priced one, six
    scenes, full precision recorded from the twin and held to the figures of the change's description to 1e-3 m;
  * edges: m = 0 and 1, a field over the cap, invalid region fields, penalty 0, a field alone and as field 40 of 65, a start in the pond.
"""
import inspect

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.support import check_entries, p as _p
from tests.test_clearance_host import INSET_SQUARE, PENALTY, REGION, WORK, WORK_R, clearance, host_transit_clear
from tests.test_field_paths_clear_host import ALL_CLEAR, NAN_REGION, NO_RING, REGION_DUBINS, REGION_RS
from tests.test_route_host import FIELDS, HOLED_SQUARE, bits, cut_with_angle, host_route, host_transit, oriented_poses, t_offsets
from tests.test_solve_clear_host import host_solve_clear
from tests.test_swaths_host import pack

ENTRIES = {'fcpp_route_transit_priced': 24, 'fcpp_ctx_route_priced_passes': 3, 'fcpp_debug_route_transit_priced': 21}
W = 4.0


def grown(ring, d):
    """a simple ring with every edge moved outwards by d, neighbours joined where the moved edges meet (a mitre)"""
    r = np.asarray(ring, dtype=np.float64)
    nxt, prv = np.roll(r, -1, axis=0), np.roll(r, 1, axis=0)
    ccw = np.sum(r[:, 0] * nxt[:, 1] - nxt[:, 0] * r[:, 1]) > 0
    out = []
    for a, v, b in zip(prv, r, nxt):
        e0, e1 = (v - a) / np.linalg.norm(v - a), (b - v) / np.linalg.norm(b - v)
        n0, n1 = np.array([e0[1], -e0[0]]), np.array([e1[1], -e1[0]])          # the right-hand normals: outwards on a counter-clockwise ring
        if not ccw:
            n0, n1 = -n0, -n1
        out.append(v + d * (n0 + n1) / (1.0 + n0 @ n1))
    return np.asarray(out)


ELL_HOLE_REGION = [grown(FIELDS['ell_hole'][0], 2.0), np.asarray(FIELDS['ell_hole'][1], dtype=np.float64)]      # the pond keeps its bank
COMB_REGION = [grown(FIELDS['comb'], 2.0)]

# name -> (work, region, R, mode); W = 4, angle 0.  The first six are the rows of the recorded figures.
SCENES = {
    'inset_rs_6': (INSET_SQUARE, HOLED_SQUARE, 6.0, 1),
    'inset_rs_3': (INSET_SQUARE, HOLED_SQUARE, 3.0, 1),
    'inset_rs_2': (INSET_SQUARE, HOLED_SQUARE, 2.0, 1),
    'holed_rs_6': (HOLED_SQUARE, REGION_RS, 6.0, 1),
    'holed_dubins_6': (HOLED_SQUARE, REGION_DUBINS, 6.0, 0),
    'inset_dubins_2': (INSET_SQUARE, HOLED_SQUARE, 2.0, 0),
    'pentagon_dubins': (WORK, REGION, WORK_R, 0),
    'pentagon_rs': (WORK, REGION, WORK_R, 1),
    'ell_hole_dubins': (FIELDS['ell_hole'], ELL_HOLE_REGION, 6.0, 0),
    'ell_hole_rs': (FIELDS['ell_hole'], ELL_HOLE_REGION, 6.0, 1),
    'comb_dubins': (FIELDS['comb'], COMB_REGION, 6.0, 0),
    'comb_rs': (FIELDS['comb'], COMB_REGION, 6.0, 1),
}
TABLE = ('inset_rs_6', 'inset_rs_3', 'inset_rs_2', 'holed_rs_6', 'holed_dubins_6', 'inset_dubins_2')


def host_transit_priced(cut, regions, radius, mode, penalty=PENALTY, expect=0, with_k=True, fill=-7.0, region=None):
    """fcpp_debug_route_transit_priced on a host_cut() and one region per field -> (T, K, toff); T and K pre-filled: T is out only"""
    lib = L.load()
    soff = cut['offsets']
    toff = t_offsets(soff)
    ro, vo, x, y = pack(regions) if region is None else region
    ax, ay, bx, by = (np.ascontiguousarray(cut[k]) for k in ('ax', 'ay', 'bx', 'by'))
    T, K = np.full(int(toff[-1]), fill), np.full(int(toff[-1]), 77, np.int8)
    rc = lib.fcpp_debug_route_transit_priced(len(soff) - 1, _p(soff), int(soff[-1]), _p(ax), _p(ay), _p(bx), _p(by), _p(cut['angle']), float(radius),
                                             mode, _p(toff), int(toff[-1]), _p(ro), len(vo) - 1, _p(vo), len(x), _p(x), _p(y), float(penalty), _p(T),
                                             _p(K) if with_k else None)
    assert rc == expect, lib.fcpp_last_error()
    return T, K, toff


def canonical_pairs(N):
    return [(p, q) for p in range(N) for q in range(N) if (p >> 1) != (q >> 1) and p * N + q <= (q ^ 1) * N + (p ^ 1)]


def composed_priced(cut, regions, radius, mode, penalty=PENALTY):
    """the block from the existing twins -> (T, K, toff, listed): listed counts the canonical pairs of a valid field whose shortest word
    starts inside and crosses"""
    T, toff = host_transit(cut, radius, mode)
    K = np.zeros(len(T), np.int8)
    listed = 0
    for i in range(len(cut['offsets']) - 1):
        N = 2 * int(cut['offsets'][i + 1] - cut['offsets'][i])
        if toff[i + 1] == toff[i] or N < 4:
            continue
        ent, ext = oriented_poses(cut, i)
        pq = canonical_pairs(N)
        p, q = np.array([a for a, _ in pq]), np.array([b for _, b in pq])
        r = host_solve_clear(mode, ext[p], ent[q], radius, i, regions)
        v = np.where(r['rank'] >= 0, r['len'], r['len'] + penalty)
        Tb, Kb = T[toff[i]:toff[i + 1]].reshape(N, N), K[toff[i]:toff[i + 1]].reshape(N, N)
        assert r['rank'].max() < 48
        Tb[p, q] = v; Tb[q ^ 1, p ^ 1] = v
        Kb[p, q] = r['rank']; Kb[q ^ 1, p ^ 1] = r['rank']
        c = clearance(ext[p], ent[q], regions, i, radius, mode)
        listed += int(np.count_nonzero((c['inside'] == 1) & (c['crossings'] > 0)))
    return T, K, toff, listed


def same_block_bytes(a, b):
    assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), np.flatnonzero(a.view(np.uint8) != b.view(np.uint8))[:8]


def check_consequences(cut, regions, radius, mode, T, K, toff, penalty=PENALTY):
    T0, _ = host_transit(cut, radius, mode)
    Tp = T0.copy()
    B = host_transit_clear(cut, regions, Tp, toff, radius, mode, penalty)
    assert np.array_equal(bits(T[K == 0]), bits(T0[K == 0]))
    assert np.array_equal(bits(T[K == -1]), bits(Tp[K == -1]))
    assert np.array_equal(K != 0, B == 1)
    # (priced <= penalised needs a penalty beyond the detour of a clear word: with penalty 0 the penalised block is the plain one)
    assert np.all(T0 <= T) and (penalty == 0.0 or np.all(T <= Tp))
    for i in range(len(cut['offsets']) - 1):
        N = 2 * int(cut['offsets'][i + 1] - cut['offsets'][i])
        if toff[i + 1] == toff[i]:
            continue
        t, k = T[toff[i]:toff[i + 1]].reshape(N, N), K[toff[i]:toff[i + 1]].reshape(N, N)
        p, q = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
        assert np.array_equal(bits(t), bits(t[q ^ 1, p ^ 1])) and np.array_equal(k, k[q ^ 1, p ^ 1])
        same = (p >> 1) == (q >> 1)
        assert np.all(np.isposinf(t[same])) and not k[same].any()


def scene_cut(name):
    work, region, radius, mode = SCENES[name]
    return cut_with_angle([work], 0.0, W), [region], radius, mode


# ---- 1. the entries --------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    check_entries(ENTRIES)
    for fn in (E.swath_transit, E.route_swaths, E.plan_polygon_fields):
        assert inspect.signature(fn).parameters['price_clear'].default is False
    import dataclasses
    assert [f.name for f in dataclasses.fields(E.SwathRoute)][-1] == 'reshaped' and E.SwathRoute.__dataclass_fields__['reshaped'].default is None
    with pytest.raises(ValueError):
        E.route_swaths(None, 6.0, price_clear=True)
    with pytest.raises(ValueError):
        E.swath_transit(None, 6.0, price_clear=True)
    with pytest.raises(ValueError):
        E.plan_polygon_fields([HOLED_SQUARE], 4.0, 6.0, 0.5, [0.0], clear_of='boundary', price_clear=True)
    with pytest.raises(ValueError):
        E.plan_polygon_fields([HOLED_SQUARE], 4.0, 6.0, 0.5, [0.0], reshape=True, price_clear=True)


def test_call_errors_need_no_device():
    lib = L.load()
    cut = cut_with_angle([HOLED_SQUARE], [0.0], W)
    soff, nt = cut['offsets'], int(cut['offsets'][-1])
    toff = t_offsets(soff)
    tt = int(toff[-1])
    T, K = np.zeros(tt), np.zeros(tt, np.int8)
    ax, ay, bx, by = (np.ascontiguousarray(cut[k]) for k in ('ax', 'ay', 'bx', 'by'))
    ro, vo, x, y = pack([HOLED_SQUARE])

    def call(n=1, soff=soff, nt=nt, ax=ax, ang=cut['angle'], radius=6.0, mode=0, toff=toff, tt=tt, ro=ro, nr=len(vo) - 1, vo=vo, nv=len(x), x=x,
             penalty=PENALTY, T=T, K=K):
        return lib.fcpp_debug_route_transit_priced(n, _p(soff), nt, _p(ax), _p(ay), _p(bx), _p(by), _p(ang), float(radius), mode, _p(toff), tt, _p(ro), nr,
                                                   _p(vo), nv, _p(x), _p(y), float(penalty), _p(T), _p(K))
    assert call() == 0 and call(K=None) == 0 and call(penalty=0.0) == 0
    for kw in (dict(radius=0.0), dict(radius=np.nan), dict(mode=2), dict(soff=None), dict(toff=None), dict(ax=None), dict(ang=None), dict(T=None),
               dict(ro=None), dict(vo=None), dict(x=None), dict(penalty=-1.0), dict(penalty=np.inf), dict(penalty=np.nan),
               dict(ang=np.array([np.nan]))):
        assert call(**kw) == L.EINVAL, kw
    for kw in (dict(n=-1), dict(nt=-1), dict(tt=-1), dict(nr=-1), dict(nv=-1), dict(nr=5), dict(soff=np.array([1, nt], np.int64)),
               dict(toff=np.array([0, tt - 4], np.int64), tt=tt - 4), dict(tt=tt + 1), dict(ro=np.array([1, 2], np.int64))):
        assert call(**kw) == L.ESIZE, kw
    head = (1, _p(soff), _p(soff), nt, _p(ax), _p(ay), _p(bx), _p(by), _p(cut['angle']), 6.0, 0, _p(toff), _p(toff), tt, _p(ro), len(vo) - 1, _p(vo),
            len(x), _p(x), _p(y), PENALTY, _p(T), _p(K))
    assert lib.fcpp_route_transit_priced(None, *head) == L.EINVAL
    assert lib.fcpp_ctx_route_priced_passes(None, None, None) == L.EINVAL


# ---- 2. composition, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SCENES))
def test_twin_equals_the_composition_of_the_existing_twins(name):
    cut, regions, radius, mode = scene_cut(name)
    T, K, toff = host_transit_priced(cut, regions, radius, mode)
    Tc, Kc, _, listed = composed_priced(cut, regions, radius, mode)
    same_block_bytes(T, Tc)
    same_block_bytes(K, Kc)
    check_consequences(cut, regions, radius, mode, T, K, toff)
    n_pairs = len(canonical_pairs(2 * int(cut['offsets'][1])))
    print(f'{name}: {len(T)} entries, {n_pairs} canonical pairs, {listed} listed; entries K = -1: {np.count_nonzero(K == -1)}, K > 0: '
          f'{np.count_nonzero(K > 0)}, largest K {K.max()}')
    if name in TABLE:
        # between 460 and 726 of the 784 entries have a blocked shortest word; for 142 .. 218 of them another word is clear, but for the
        # Dubins turns at R = 2 in the inset square, where it is 4 (seen on the twin)
        rescued = np.count_nonzero(K > 0)
        assert len(T) == 784 and 460 <= np.count_nonzero(K != 0) <= 726 and (142 <= rescued <= 218 or (name == 'inset_dubins_2' and rescued == 4))


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('radius', [6.0, 3.0])
def test_inset_square_dubins_has_no_rescued_entry_and_reeds_shepp_has(mode, radius):
    cut = cut_with_angle([INSET_SQUARE], 0.0, W)
    T, K, toff = host_transit_priced(cut, [HOLED_SQUARE], radius, mode)
    Tp, _ = host_transit(cut, radius, mode)
    host_transit_clear(cut, [HOLED_SQUARE], Tp, toff, radius, mode, PENALTY)
    if mode == 0:
        assert not (K > 0).any() and np.array_equal(bits(T), bits(Tp))                  # penalty and priced are the same matrix
    else:
        assert (K > 0).any() and not np.array_equal(bits(T), bits(Tp))


# ---- 3. recorded figures ---------------------------------------------------------------------------------------------------------------
# (penalty: length, blocked), (priced: length, blocked): the figures of the change's description, to 1e-3 m ...
DESCRIBED = {
    'inset_rs_6': ((170.7504, 0), (161.8702, 0)),
    'inset_rs_3': ((167.6601, 0), (133.5520, 0)),
    'inset_rs_2': ((212.9189, 0), (105.9088, 0)),
    'holed_rs_6': ((198.5378, 0), (196.1477, 0)),
    'holed_dubins_6': ((278.5520, 3), (269.5486, 3)),
    'inset_dubins_2': ((102.3982, 12), (167.5310, 11)),
}


def driven_reshaped(cut, route, region, radius, mode):
    """the legs of `route` as driven with reshaping -> (summed len of fcpp_debug_conn_solve_clear, legs of rank -1, legs of rank > 0)"""
    ent, ext = oriented_poses(cut, 0)
    route = np.asarray(route, dtype=np.int64)
    r = host_solve_clear(mode, ext[route[:-1]], ent[route[1:]], radius, 0, [region])
    return float(r['len'].sum()), int(np.count_nonzero(r['rank'] < 0)), int(np.count_nonzero(r['rank'] > 0))


def routed_both(name):
    cut, regions, radius, mode = scene_cut(name)
    assert int(cut['offsets'][1]) == 14
    Tp, toff = host_transit(cut, radius, mode)
    host_transit_clear(cut, regions, Tp, toff, radius, mode, PENALTY)
    Tq, _, _ = host_transit_priced(cut, regions, radius, mode)
    out = []
    for T in (Tp, Tq):
        res = host_route(cut['offsets'], T, toff, S=8)
        assert res['status'][0] == 0
        out.append((float(res['cost'][0]),) + driven_reshaped(cut, res['route'], regions[0], radius, mode))
    return out


@pytest.mark.parametrize('name', TABLE)
def test_recorded_figures_priced_route_drives_no_longer_and_blocks_no_more(name):
    (cost_p, len_p, blk_p, _), (cost_q, len_q, blk_q, resh_q) = routed_both(name)
    print(f'{name}: penalty matrix {len_p!r} m, {blk_p} blocked; priced matrix {len_q!r} m, {blk_q} blocked, {resh_q} reshaped; '
          f'|cost - driven| priced {abs(cost_q - len_q):.3g}')
    (want_len_p, want_blk_p), (want_len_q, want_blk_q) = DESCRIBED[name]
    assert abs(len_p - want_len_p) <= 1e-3 and abs(len_q - want_len_q) <= 1e-3 and (blk_p, blk_q) == (want_blk_p, want_blk_q)
    assert abs(len_p - RECORDED[name][0]) <= 1e-9 and abs(len_q - RECORDED[name][1]) <= 1e-9
    assert blk_q <= blk_p
    if blk_q == blk_p:
        assert len_q < len_p
    if blk_q == 0:
        # the priced matrix holds what is driven: the router's cost is the driven length (seen: at most 3e-14)
        assert abs(cost_q - len_q) <= 1e-9


# ... and in full precision as the host twin gives them: (penalty matrix, priced matrix) driven length [m]
RECORDED = {
    'inset_rs_6': (170.75037418543062, 161.87019827158377),
    'inset_rs_3': (167.66014279404217, 133.5520454835079),
    'inset_rs_2': (212.9189131549674, 105.90878388074124),
    'holed_rs_6': (198.53777627849308, 196.14772709887092),
    'holed_dubins_6': (278.55201225835924, 269.54856178981146),
    'inset_dubins_2': (102.39822368615506, 167.5309649148734),
}


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------------
def strip(k):
    return [(0, 0), (10, 0), (10, W * k), (0, W * k)]


@pytest.mark.parametrize('mode', [0, 1])
def test_no_swath_one_swath_and_a_field_over_the_cap(mode):
    fields = [[(0, 0), (10, 0), (10, 1), (0, 1)], strip(1), strip(513), strip(3)]
    cut = cut_with_angle(fields, 0.0, W)
    assert list(np.diff(cut['offsets'])) == [0, 1, 513, 3]
    regions = [[(-20, -20), (30, -20), (30, 2100), (-20, 2100)]] * 4
    T, K, toff = host_transit_priced(cut, regions, 6.0, mode)
    assert list(toff) == [0, 0, 4, 4, 40]                                              # no block for m = 0 and for m = 513: nothing written
    assert np.all(np.isposinf(T[:4])) and not K[:4].any()                               # m = 1: one swath, all +inf, K = 0
    Tc, Kc, _, _ = composed_priced(cut, regions, 6.0, mode)
    same_block_bytes(T, Tc)
    same_block_bytes(K, Kc)
    # and a batch of the over-the-cap field alone has nothing to write at all
    alone = cut_with_angle([strip(513)], 0.0, W)
    T, K, toff = host_transit_priced(alone, regions[:1], 6.0, mode)
    assert len(T) == 0 and list(toff) == [0, 0]


@pytest.mark.parametrize('bad', ['nan', 'no_ring'])
@pytest.mark.parametrize('mode', [0, 1])
def test_an_invalid_region_field_prices_every_pair_plain_plus_penalty(mode, bad):
    cut = cut_with_angle([HOLED_SQUARE, HOLED_SQUARE], 0.0, W)
    good = REGION_RS if mode else REGION_DUBINS
    regions = [NAN_REGION if bad == 'nan' else NO_RING, good]
    T, K, toff = host_transit_priced(cut, regions, 6.0, mode)
    T0, _ = host_transit(cut, 6.0, mode)
    N = 28
    t, k, t0 = (a[toff[0]:toff[1]].reshape(N, N) for a in (T, K, T0))
    p, q = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    same = (p >> 1) == (q >> 1)
    assert np.all(k[~same] == -1) and np.array_equal(bits(t[~same]), bits(t0[~same] + PENALTY)) and not k[same].any() and np.all(np.isposinf(t[same]))
    # the neighbour is unaffected: what it is alone
    alone = cut_with_angle([HOLED_SQUARE], 0.0, W)
    Ta, Ka, _ = host_transit_priced(alone, [good], 6.0, mode)
    same_block_bytes(T[toff[1]:], Ta)
    same_block_bytes(K[toff[1]:], Ka)
    assert (Ka > 0).any()


@pytest.mark.parametrize('mode', [0, 1])
def test_penalty_zero_all_clear_and_k_null(mode):
    cut = cut_with_angle([INSET_SQUARE], 0.0, W)
    T0, _ = host_transit(cut, 6.0, mode)
    Tz, Kz, toff = host_transit_priced(cut, [HOLED_SQUARE], 6.0, mode, penalty=0.0)
    Tp, Kp, _ = host_transit_priced(cut, [HOLED_SQUARE], 6.0, mode)
    assert np.array_equal(Kz, Kp) and np.array_equal(bits(Tz[Kz <= 0]), bits(T0[Kz <= 0])) and np.array_equal(bits(Tz[Kz > 0]), bits(Tp[Kz > 0]))
    check_consequences(cut, [HOLED_SQUARE], 6.0, mode, Tz, Kz, toff, penalty=0.0)
    Tn, Kn, _ = host_transit_priced(cut, [HOLED_SQUARE], 6.0, mode, with_k=False)
    same_block_bytes(Tn, Tp)
    assert np.all(Kn == 77)
    Ta, Ka, _ = host_transit_priced(cut, [ALL_CLEAR], 6.0, mode)
    assert not Ka.any() and np.array_equal(bits(Ta), bits(T0))


@pytest.mark.parametrize('mode', [0, 1])
def test_a_field_alone_equals_the_same_field_as_field_40_of_65(mode):
    works = [strip(1 + (j % 4)) for j in range(65)]
    regions = [[(-20, -20), (30, -20), (30, 40), (-20, 40)]] * 65
    works[40], regions[40] = INSET_SQUARE, HOLED_SQUARE
    cut = cut_with_angle(works, 0.0, W)
    T, K, toff = host_transit_priced(cut, regions, 3.0, mode)
    alone = cut_with_angle([INSET_SQUARE], 0.0, W)
    Ta, Ka, _ = host_transit_priced(alone, [HOLED_SQUARE], 3.0, mode)
    same_block_bytes(T[toff[40]:toff[41]], Ta)
    same_block_bytes(K[toff[40]:toff[41]], Ka)
    assert (Ka == -1).any() and (Ka == 0).any() and ((Ka > 0).any() or mode == 0)


@pytest.mark.parametrize('mode', [0, 1])
def test_a_start_pose_in_the_pond_is_rank_minus_one_without_listing(mode):
    # HOLED_SQUARE's own swaths against a region whose pond reaches 1 m beyond the hole: the swath ends at the hole lie IN the pond
    cut = cut_with_angle([HOLED_SQUARE], 0.0, W)
    region = [REGION_RS[0], [(11, 11), (29, 11), (29, 29), (11, 29)]]
    T, K, toff = host_transit_priced(cut, [region], 6.0, mode)
    Tc, Kc, _, listed = composed_priced(cut, [region], 6.0, mode)
    same_block_bytes(T, Tc)
    same_block_bytes(K, Kc)
    ent, ext = oriented_poses(cut, 0)
    pq = canonical_pairs(len(ent))
    p, q = np.array([a for a, _ in pq]), np.array([b for _, b in pq])
    c = clearance(ext[p], ent[q], [region], 0, 6.0, mode)
    in_pond = c['inside'] == 0
    assert in_pond.sum() >= 50 and (c['crossings'][in_pond] > 0).any()
    k = K.reshape(len(ent), len(ent))[p, q]
    assert np.all(k[in_pond] == -1)                                                      # whatever the other words do
    assert listed == np.count_nonzero(~in_pond & (c['crossings'] > 0))
