"""GPU tests of the connector clearance (run with -m gpu on an MI355X): fcpp_conn_clear and fcpp_route_transit_clear give what their host
twins give -- integers exactly, first_s and T bit for bit, both modes -- on the smallest shapes that can go wrong: a triangle, a square with
a triangular hole, a field of FCPP_CLEAR_EDGE_CHUNK + 1 edges with the swaths inside it (a second LDS chunk that holds one edge, on which the start points'
parity and the right-hand turns' crossings hang), a field whose first chunk a turn skips by its box, fields of 0, 1, 2 and 33 swaths (66
oriented swaths: the canonical pairs of a row straddle a 64-lane boundary), a batch with a field without rings and an invalid one in the
middle, n = 0, 1, 65 paths with pair_field unsorted and with -1; a region of 259 rings (the ring loop's second round of 256) whose last
rings decide answers, intact and with the LAST ring spoilt.  Then the engine's layers on top of them."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.test_clearance_host import (MANY_RINGS, MANY_RINGS_CUT, PENALTY, REGION, SQUARE_HOLE, WORK, WORK_R, bits, clearance, driven_blocked,
                                       host_clear, host_solve, host_transit_clear, many_ring_pairs, many_ring_region, many_ring_work)
from tests.test_route_host import cut_with_angle, host_transit
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu

TRIANGLE = [(0, 0), (30, 2), (12, 28)]
SQUARE_TRI = [[(0, 0), (30, 0), (30, 30), (0, 30)], [(9, 8), (21, 9), (14, 20)]]
RING257 = [(15 + 16 * np.cos(2 * np.pi * k / (L.CLEAR_EDGE_CHUNK + 1)), 15 + 16 * np.sin(2 * np.pi * k / (L.CLEAR_EDGE_CHUNK + 1)))
           for k in range(L.CLEAR_EDGE_CHUNK + 1)]
NO_RINGS = []
INVALID = [[(0, 0), (30, 0), (np.nan, 30)]]
FIVE = [TRIANGLE, NO_RINGS, SQUARE_TRI, INVALID, RING257]


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture
def gpu():
    import torch
    ctx = E.get_context(None)
    ctx.bind_stream()
    return ctx, torch.device('cuda', ctx.device)


def random_pairs(seed, n):
    rng = np.random.default_rng(seed)
    frm = np.column_stack([rng.uniform(1, 29, n), rng.uniform(1, 29, n), rng.uniform(-np.pi, np.pi, n)])
    to = np.column_stack([rng.uniform(1, 29, n), rng.uniform(1, 29, n), rng.uniform(-np.pi, np.pi, n)])
    return frm, to


def device_clear(gpu, mode, frm, radius, word, seg, pair_field, fields):
    import torch
    ctx, dev = gpu
    n = len(frm)
    ro, vo, x, y = (_t(a, dev) for a in pack(fields))
    f = [_t(frm[:, k], dev) for k in range(3)]
    w, s, pf = _t(word.astype(np.int32), dev), _t(seg, dev), _t(np.asarray(pair_field, dtype=np.int64), dev)
    out = dict(crossings=torch.full((n,), -7, dtype=torch.int32, device=dev), inside=torch.full((n,), -7, dtype=torch.int8, device=dev),
               first_s=torch.full((n,), -7.0, dtype=torch.float64, device=dev),
               field_status=torch.full((len(fields),), -7, dtype=torch.int32, device=dev))
    L.check(ctx.lib.fcpp_conn_clear(ctx.handle, mode, n, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), float(radius), _ptr(w), _ptr(s), _ptr(pf), len(fields),
                                    _ptr(ro), int(vo.numel()) - 1, _ptr(vo), int(x.numel()), _ptr(x), _ptr(y), *[_ptr(out[k]) for k in out]))
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [0, 1, 65])
def test_elementwise_equals_the_host_twin(gpu, mode, n):
    R = 4.0
    frm, to = random_pairs(7 + n + mode, n)
    rng = np.random.default_rng(n)
    pair_field = rng.integers(-1, len(FIVE), n)                     # unsorted, with -1
    if n == 65:
        pair_field[:5] = [4, -1, 0, 2, 4]
        to[7, 0] = np.nan                                           # an unsolved pair
    word, seg, _ = host_solve(frm, to, R, mode)
    want = host_clear(mode, frm, R, word, seg, pair_field, FIVE)
    got = device_clear(gpu, mode, frm, R, word, seg, pair_field, FIVE)
    assert np.array_equal(want['field_status'], [0, L.EINVAL, 0, L.EINVAL, 0])
    for k in ('crossings', 'inside', 'field_status'):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got['first_s']), bits(want['first_s']))
    if n == 65:
        # every outcome occurs: clear, crossed, started outside, no region, bad field, unsolved -- and against the field of 257 edges
        assert want['clear'].any() and (want['crossings'] > 0).any() and ((want['inside'] == 0) & (want['crossings'] > 0)).any()
        assert np.isnan(want['first_s']).sum() >= 3 and (want['crossings'][pair_field == 4] > 0).any()


# works of 0, 1, 2 and 33 swaths at W = 4 (lines at 2, 6, ..: a height of 1, 3, 7, 132) inside their regions
def _work(h, x0=2.0, y0=2.0, w=26.0):
    return [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)]


def _gon(n, cx, cy, r):
    return [(cx + r * np.cos(2 * np.pi * k / n), cy + r * np.sin(2 * np.pi * k / n)) for k in range(n)]


def _rect_right_side_last(x0, y0, x1, y1):
    """a rectangle whose LAST edge (vertex 3 -> vertex 0) is its right side: the edge every ray S + (t, 0) from inside crosses"""
    return [(x1, y0), (x0, y0), (x0, y1), (x1, y1)]


# Two regions whose edges do not fit ONE LDS chunk, with the swaths strictly inside them.
# SECOND_ONE: a pond of CHUNK - 3 vertices out of every connector's reach, then the boundary: CHUNK + 1 edges, the second chunk holds ONE
#   edge, the boundary's right side.  Every start point's parity hangs on it (it is the only edge their rays meet), and so do
#   the crossings of the turns at the swaths' right ends, which lie 3.5, 6.4 and 9.3 m from it (a slanted work area).
# FIRST_SKIPPED: a pond of exactly CHUNK vertices beside the left swath ends fills the first chunk, the boundary is the second.  The turns
#   at the left ends cross the pond; for a turn at the right ends (x = 60) the first chunk's box (x <= 19) meets neither the path's box nor
#   the start point's ray: the chunk is skipped.
SLANTED = [(20, 20), (62, 20), (54, 31), (20, 31)]
SECOND_ONE = [_gon(L.CLEAR_EDGE_CHUNK - 3, 8, 46, 3), _rect_right_side_last(0, 0, 64, 52)]
SECOND_ONE_MOVED = [SECOND_ONE[0], _rect_right_side_last(0, 0, 90, 52)]             # the right side out of every turn's reach
FIRST_SKIPPED = [_gon(L.CLEAR_EDGE_CHUNK, 15, 30, 4), _rect_right_side_last(-10, 0, 90, 60)]
WORKS = [_work(1), _work(3), _work(7), _work(132), _work(7), _work(7), SLANTED, _work(19, 20.0, 20.0, 40.0)]
REGIONS = [TRIANGLE, [(-5, -5), (40, -5), (40, 12), (-5, 12)], NO_RINGS, [[(-8, -8), (38, -8), (38, 142), (-8, 142)], [(9, 60), (21, 61), (14, 72)]],
           INVALID, RING257, SECOND_ONE, FIRST_SKIPPED]
N_SWATHS = [0, 1, 2, 33, 2, 2, 3, 5]


@pytest.fixture(scope='module')
def transit_case():
    """the cut and per mode the host twin's T (plain and penalised) and B -- computed once, left unchanged"""
    cut = cut_with_angle(WORKS, 0.0, 4.0)
    assert np.diff(cut['offsets']).tolist() == N_SWATHS
    per_mode = {}
    for mode in (0, 1):
        T0, toff = host_transit(cut, 6.0, mode)
        Tp = T0.copy()
        B = host_transit_clear(cut, REGIONS, Tp, toff, 6.0, mode, PENALTY)
        per_mode[mode] = (T0, Tp, B, toff)
    return cut, per_mode


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('penalty', [PENALTY, 0.0])
def test_transit_block_equals_the_host_twin(gpu, transit_case, mode, penalty):
    import torch
    ctx, dev = gpu
    cut, per_mode = transit_case
    T0, Tp, B, toff = per_mode[mode]
    soff = cut['offsets']
    ro, vo, x, y = (_t(a, dev) for a in pack(REGIONS))
    d = {k: _t(cut[k], dev) for k in ('ax', 'ay', 'bx', 'by', 'angle')}
    soff_d, toff_d = _t(soff, dev), _t(toff, dev)
    T = _t(T0.copy(), dev)
    Bd = torch.full((int(toff[-1]),), 7, dtype=torch.uint8, device=dev)
    L.check(ctx.lib.fcpp_route_transit_clear(ctx.handle, len(soff) - 1, _ptr(soff_d), soff.ctypes.data, int(soff[-1]), _ptr(d['ax']), _ptr(d['ay']),
                                             _ptr(d['bx']), _ptr(d['by']), _ptr(d['angle']), 6.0, mode, _ptr(toff_d), None, int(toff[-1]), _ptr(ro),
                                             int(vo.numel()) - 1, _ptr(vo), int(x.numel()), _ptr(x), _ptr(y), float(penalty), _ptr(T), _ptr(Bd)))
    assert np.array_equal(Bd.cpu().numpy(), B)
    assert np.array_equal(bits(T.cpu().numpy()), bits(Tp if penalty else T0))
    # the cases are what they are meant to be: blocked and clear pairs in the field of 33 swaths, everything blocked where the region is bad
    blocks = [B[toff[i]:toff[i + 1]] for i in range(len(soff) - 1)]
    assert blocks[0].size == 0 and blocks[1].size == 4 and blocks[3].size == 66 * 66
    assert 0 < blocks[3].sum() < blocks[3].size - 2 * 66 and blocks[2].sum() == blocks[4].sum() == 16 - 8 and 0 < blocks[5].sum()


def _host_B(work, region, mode, penalty=0.0):
    cut = cut_with_angle([work], 0.0, 4.0)
    T, toff = host_transit(cut, 6.0, mode)
    N = 2 * int(cut['offsets'][1])
    return host_transit_clear(cut, [region], T, toff, 6.0, mode, penalty).reshape(N, N), T.reshape(N, N), cut


@pytest.mark.parametrize('mode', [0, 1])
def test_the_second_lds_chunk_decides_results(transit_case, mode):
    """the host twin's side of the two-chunk fields: what the device is compared with above DEPENDS on the edges staged second"""
    _, per_mode = transit_case
    _, _, B, toff = per_mode[mode]
    assert sum(len(r) for r in SECOND_ONE) == L.CLEAR_EDGE_CHUNK + 1 and sum(len(r) for r in FIRST_SKIPPED) == L.CLEAR_EDGE_CHUNK + 4
    b, _, cut = _host_B(SLANTED, SECOND_ONE, mode)
    N = b.shape[0]
    assert np.array_equal(b.reshape(-1), B[toff[6]:toff[7]])
    p, q = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    other = (p >> 1) != (q >> 1)
    # parity: of the edges a start point's ray meets, the only one is the one edge of the second chunk -- clear pairs exist only if it
    # is counted, and with that side drawn LEFT of the swaths every pair is blocked
    assert (b[other] == 0).any() and (b[other] == 1).any()
    assert _host_B(SLANTED, [SECOND_ONE[0], _rect_right_side_last(0, 0, 10, 52)], mode)[0][other].all()
    # crossings: with that edge moved out of reach, pairs that were blocked are clear
    moved = _host_B(SLANTED, SECOND_ONE_MOVED, mode)[0]
    assert ((b == 1) & (moved == 0)).any() and not moved[other].any()
    # the first chunk is the pond alone: it blocks turns at the left ends, and a turn between two right ends cannot see it
    c, T, cut = _host_B(WORKS[7], FIRST_SKIPPED, mode)
    assert np.array_equal(c.reshape(-1), B[toff[7]:toff[8]])
    bare = _host_B(WORKS[7], [FIRST_SKIPPED[1]], mode)[0]
    assert ((c == 1) & (bare == 0)).any() and not bare.any()
    pond_x1 = max(x for x, _ in FIRST_SKIPPED[0])
    right = [(2 * s, 2 * t + 1) for s in range(5) for t in range(5) if s != t]            # leaves at b (x = 60), enters at b
    assert all(cut['bx'][s >> 1] == 60.0 for s, _ in right)
    assert any(c[s, t] == 0 and 60.0 - T[s, t] > pond_x1 + 6.0 for s, t in right)        # the whole path stays right of the pond's box


# ---- a region of 259 rings: the second round of the ring loop ---------------------------------------------------------------------------------
# (tests/test_clearance_host.py builds the region, checks it against the chord oracle and asserts that rings 256 .. 258 decide answers)
def many_ring_regions():
    """the region, its two copies with the LAST ring spoilt, and the region without its last three rings"""
    return [MANY_RINGS, many_ring_region('short'), MANY_RINGS_CUT, many_ring_region('nan')]


@pytest.mark.parametrize('mode', [0, 1])
def test_region_of_259_rings_elementwise(gpu, mode):
    R = 4.0
    frm, to = many_ring_pairs()
    n = len(frm)
    frm, to, pair_field = np.tile(frm, (4, 1)), np.tile(to, (4, 1)), np.repeat(np.arange(4), n)
    word, seg, _ = host_solve(frm, to, R, mode)
    fields = many_ring_regions()
    want = host_clear(mode, frm, R, word, seg, pair_field, fields)
    assert want['field_status'].tolist() == [0, L.EINVAL, 0, L.EINVAL]
    full, cut = want['crossings'][:n], want['crossings'][2 * n:3 * n]
    assert (full != cut).sum() >= 3 and want['clear'][:n].sum() >= 20 and not want['clear'][n:2 * n].any() and not want['clear'][3 * n:].any()
    got = device_clear(gpu, mode, frm, R, word, seg, pair_field, fields)
    for k in ('crossings', 'inside', 'field_status'):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got['first_s']), bits(want['first_s']))


@pytest.fixture(scope='module')
def many_ring_transit():
    cut = cut_with_angle([many_ring_work()] * 4, 0.0, 4.0)
    assert np.diff(cut['offsets']).tolist() == [2] * 4
    per_mode = {}
    for mode in (0, 1):
        T0, toff = host_transit(cut, 6.0, mode)
        Tp = T0.copy()
        B = host_transit_clear(cut, many_ring_regions(), Tp, toff, 6.0, mode, PENALTY)
        per_mode[mode] = (T0, Tp, B, toff)
    return cut, per_mode


@pytest.mark.parametrize('mode', [0, 1])
def test_region_of_259_rings_transit_block(gpu, many_ring_transit, mode):
    """the ring sizes are read 256 at a time: a LAST ring of two vertices blocks the whole field only if round two reads it; the edges of
    rings 256 .. 258 sit in the fourth edge chunk with their ring found by bisection over 259 offsets"""
    import torch
    ctx, dev = gpu
    cut, per_mode = many_ring_transit
    T0, Tp, B, toff = per_mode[mode]
    b = B.reshape(4, 4, 4)
    other = (np.arange(4)[:, None] >> 1) != (np.arange(4)[None, :] >> 1)
    assert (b[0] != b[2]).sum() >= 2 and (b[0][other] == 0).any() and b[1][other].all() and b[3][other].all() and not b[2][other].all()
    soff = cut['offsets']
    ro, vo, x, y = (_t(a, dev) for a in pack(many_ring_regions()))
    d = {k: _t(cut[k], dev) for k in ('ax', 'ay', 'bx', 'by', 'angle')}
    soff_d, toff_d = _t(soff, dev), _t(toff, dev)
    T = _t(T0.copy(), dev)
    Bd = torch.full((int(toff[-1]),), 7, dtype=torch.uint8, device=dev)
    L.check(ctx.lib.fcpp_route_transit_clear(ctx.handle, len(soff) - 1, _ptr(soff_d), soff.ctypes.data, int(soff[-1]), _ptr(d['ax']), _ptr(d['ay']),
                                             _ptr(d['bx']), _ptr(d['by']), _ptr(d['angle']), 6.0, mode, _ptr(toff_d), None, int(toff[-1]), _ptr(ro),
                                             int(vo.numel()) - 1, _ptr(vo), int(x.numel()), _ptr(x), _ptr(y), PENALTY, _ptr(T), _ptr(Bd)))
    assert np.array_equal(Bd.cpu().numpy(), B)
    assert np.array_equal(bits(T.cpu().numpy()), bits(Tp))


# ---- the engine's layers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reversing', [False, True])
def test_connector_clearance(reversing):
    frm, to = random_pairs(3, 40)
    pair_field = np.arange(40) % 3 - 1
    fields = [SQUARE_HOLE, SQUARE_TRI]
    c = E.connector_clearance(frm, to, fields, pair_field, 4.0, reversing=reversing)
    want = clearance(frm, to, fields, pair_field, 4.0, int(reversing))
    assert np.array_equal(c.clear.cpu().numpy(), want['clear']) and np.array_equal(c.crossings.cpu().numpy(), want['crossings'])
    assert np.array_equal(c.inside.cpu().numpy(), want['inside']) and np.array_equal(bits(c.first_s.cpu().numpy()), bits(want['first_s']))
    assert np.array_equal(bits(c.length.cpu().numpy()), bits(want['length'])) and c.field_status.cpu().tolist() == [0, 0]
    assert want['clear'].any() and not want['clear'].all()


def _swaths(fields, W=4.0):
    return E.polygon_swaths(fields, 0.0, W)


@pytest.mark.parametrize('reversing', [False, True])
def test_swath_transit_with_clear_of(transit_case, reversing):
    cut, per_mode = transit_case
    T0, Tp, B, toff = per_mode[int(reversing)]
    ss = _swaths(WORKS)
    assert np.array_equal(ss.offsets_host, cut['offsets'])
    plain = E.swath_transit(ss, 6.0, reversing)
    again = E.swath_transit(ss, 6.0, reversing)
    assert len(plain) == 2 and np.array_equal(bits(plain[0].cpu().numpy()), bits(T0)) and np.array_equal(bits(again[0].cpu().numpy()), bits(T0))
    T, off, Bd = E.swath_transit(ss, 6.0, reversing, clear_of=REGIONS)
    assert np.array_equal(off, toff) and np.array_equal(Bd.cpu().numpy(), B) and np.array_equal(bits(T.cpu().numpy()), bits(Tp))


@pytest.mark.parametrize('reversing', [False, True])
def test_route_swaths_avoids_the_pond(reversing):
    import torch
    mode = int(reversing)
    cut = cut_with_angle([WORK], 0.0, 4.0)
    ss = _swaths([WORK])
    plain, again = E.route_swaths(ss, WORK_R, reversing=reversing), E.route_swaths(ss, WORK_R, reversing=reversing)
    assert plain.blocked is None and plain.blocked_stored is None and plain.length is None
    for k in ('order', 'cost', 'stored_cost', 'winner', 'sweeps', 'status', 'tours', 'costs'):
        a, b = getattr(plain, k), getattr(again, k)
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), k
    routed = E.route_swaths(ss, WORK_R, reversing=reversing, clear_of=[REGION])
    assert plain.order.cpu().tolist() == [1, 2, 5] and routed.order.cpu().tolist() == [0, 3, 4]
    assert routed.blocked.cpu().tolist() == [0] and routed.blocked.dtype == torch.int32
    stored = [2 * k + (k & 1) for k in range(3)]
    assert routed.blocked_stored.cpu().tolist() == [driven_blocked(cut, 0, stored, REGION, WORK_R, mode)[0]]
    assert float(routed.cost[0]) < PENALTY and abs(float(routed.length[0]) - float(routed.cost[0])) <= 1e-9
    assert float(routed.length[0]) > float(plain.cost[0]) + 1.0
    # a penalty of 0 reports and routes as without
    free = E.route_swaths(ss, WORK_R, reversing=reversing, clear_of=[REGION], blocked_penalty=0.0)
    assert free.order.cpu().tolist() == [1, 2, 5] and free.blocked.cpu().tolist() == [driven_blocked(cut, 0, [1, 2, 5], REGION, WORK_R, mode)[0]] == [1]


THREE = [[[(0, 0), (60, 0), (60, 40), (0, 40)], [(25, 15), (35, 15), (35, 25), (25, 25)]],
         [(0, 0), (50, 0), (50, 30), (20, 30), (20, 50), (0, 50)],
         [(0, 0), (45, 5), (40, 45), (5, 40)]]


@pytest.mark.parametrize('reversing', [False, True])
def test_field_path_clearance_counts_equal_the_routes(reversing):
    n = len(THREE)
    work = E.headland(E.polygon_fields(THREE), 4.0, 1)[1]
    ss = E.polygon_swaths(work, 0.3, 4.0)
    entry = np.array([[2.0, 2.0, 0.5]] * n)
    exit_ = np.array([[3.0, 3.0, -2.0]] * n)
    route = E.route_swaths(ss, 5.0, reversing=reversing, entry=entry, exit=exit_, spacing=0.5, clear_of=THREE)
    c = E.field_path_clearance(ss, THREE, 5.0, 0.5, reversing=reversing, order=route, entry=entry, exit=exit_)
    m = np.diff(ss.offsets_host)
    assert (m > 2).all() and int(c.field.numel()) == int((m + 1).sum())
    assert np.array_equal(c.blocked.cpu().numpy(), route.blocked.cpu().numpy())
    assert np.array_equal(np.bincount(c.field.cpu().numpy()[~c.clear.cpu().numpy()], minlength=n), c.blocked.cpu().numpy())
    assert np.array_equal(bits(c.length.cpu().numpy()), bits(route.length.cpu().numpy()))
    # the slots are the connector slots of FieldPaths.leg: even, 0 .. 2 m, ascending within a field
    slot, fld = c.slot.cpu().numpy(), c.field.cpu().numpy()
    for i in range(n):
        assert slot[fld == i].tolist() == list(range(0, 2 * m[i] + 1, 2))
    paths = E.field_paths(ss, 5.0, 0.5, reversing=reversing, order=route, entry=entry, exit=exit_)
    assert np.allclose(c.length.cpu().numpy(), paths.transit_length.cpu().numpy(), rtol=0, atol=1e-9)
    # the stored order's count is the stored order's clearance
    stored = E.field_path_clearance(ss, THREE, 5.0, 0.5, reversing=reversing, entry=entry, exit=exit_)
    assert np.array_equal(stored.blocked.cpu().numpy(), route.blocked_stored.cpu().numpy())
    assert (route.blocked.cpu().numpy() <= route.blocked_stored.cpu().numpy()).all()


def test_plan_polygon_fields_with_and_without_clear_of():
    import torch
    args = dict(width=4.0, radius=5.0, spacing=0.5, angles=[0.0, 0.7, 1.4])
    a, b = E.plan_polygon_fields(THREE, **args), E.plan_polygon_fields(THREE, **args)
    assert a.clearance is None and a.route.blocked is None
    for k in ('x', 'y', 'heading', 'kappa'):
        assert torch.equal(getattr(a.paths, k).view(torch.int64), getattr(b.paths, k).view(torch.int64)), k
    assert torch.equal(a.route.order, b.route.order) and torch.equal(a.paths.offsets, b.paths.offsets)
    p = E.plan_polygon_fields(THREE, clear_of='boundary', **args)
    q = E.plan_polygon_fields(THREE, clear_of=THREE, **args)
    assert p.clearance is not None and torch.equal(p.clearance.blocked, p.route.blocked) and torch.equal(p.route.order, q.route.order)
    assert torch.equal(p.clearance.clear, q.clearance.clear)
    assert (p.route.blocked <= p.route.blocked_stored).all() and (p.paths.status == 0).all()
    # the plan's clearance is field_path_clearance of the path it drives, and an order that is no permutation is refused
    own = E.field_path_clearance(p.swaths, THREE, 5.0, 0.5, order=p.route)
    assert torch.equal(own.clear, p.clearance.clear) and torch.equal(own.slot, p.clearance.slot) and torch.equal(own.blocked, p.clearance.blocked)
    assert torch.equal(own.first_s.view(torch.int64), p.clearance.first_s.view(torch.int64))
    twice = p.route.order.clone()
    twice[1] = twice[0]
    with pytest.raises(ValueError):
        E.field_path_clearance(p.swaths, THREE, 5.0, 0.5, order=twice)
    # the legs tested are the connectors the path drives
    assert np.allclose(p.clearance.length.cpu().numpy(), p.paths.transit_length.cpu().numpy(), rtol=0, atol=1e-9)
