"""The clear connectors on the device (run with -m gpu on an MI355X): fcpp_conn_solve_clear equals its host twin bit for bit in every output,
for both modes, at the sizes where a wavefront or a workgroup ends, against regions of 3 and of FCPP_CLEAR_EDGE_CHUNK - 1 / + 0 / + 1 edges,
with pair_field grouped and shuffled and -1 / out-of-range entries mixed in; the list between the two passes (nothing listed: the second
launch is skipped; everything listed; one pair at a wavefront's edge); a region of 259 rings; and engine.clear_connectors against the ABI.
The field-path entries of the issue (fcpp_field_path_counts_clear / _fill_clear, reshape=) are not part of this change."""
import ctypes as C

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.test_clearance_host import bits
from tests.test_solve_clear_host import NSEG, U_TURN, U_WALL, host_solve_clear
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu

R = 4.0
OUTS = (('word', np.int32), ('seg', np.float64), ('len', np.float64), ('rank', np.int32), ('crossings', np.int32), ('field_status', np.int32))


def _gon(n, cx, cy, r):
    return [(cx + r * np.cos(2 * np.pi * k / n), cy + r * np.sin(2 * np.pi * k / n)) for k in range(n)]


TRIANGLE = [(0, 0), (30, 2), (12, 28)]
SQUARE_TRI = [[(0, 0), (30, 0), (30, 30), (0, 30)], [(9, 8), (21, 9), (14, 20)]]
INVALID = [[(0, 0), (30, 0), (np.nan, 30)]]
FIELDS = [TRIANGLE, _gon(L.CLEAR_EDGE_CHUNK - 1, 15, 15, 16), [], _gon(L.CLEAR_EDGE_CHUNK, 15, 15, 16), SQUARE_TRI, INVALID,
          _gon(L.CLEAR_EDGE_CHUNK + 1, 15, 15, 16)]


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


def passes(ctx):
    listed, launches = C.c_int64(-1), C.c_int64(-1)
    L.check(ctx.lib.fcpp_ctx_solve_clear_passes(ctx.handle, C.byref(listed), C.byref(launches)))
    return listed.value, launches.value


def device_solve_clear(gpu, mode, frm, to, radius, pair_field, fields):
    import torch
    ctx, dev = gpu
    n = len(frm)
    ro, vo, x, y = (_t(a, dev) for a in pack(fields))
    cols = [_t(p[:, k], dev) for p in (frm, to) for k in range(3)]
    pf = _t(np.array(np.broadcast_to(np.asarray(pair_field, dtype=np.int64), (n,))), dev)
    out = dict(word=torch.full((n,), -9, dtype=torch.int32, device=dev), seg=torch.full((n, NSEG[mode]), -9.0, dtype=torch.float64, device=dev),
               len=torch.full((n,), -9.0, dtype=torch.float64, device=dev), rank=torch.full((n,), -9, dtype=torch.int32, device=dev),
               crossings=torch.full((n,), -9, dtype=torch.int32, device=dev),
               field_status=torch.full((len(fields),), -9, dtype=torch.int32, device=dev))
    L.check(ctx.lib.fcpp_conn_solve_clear(ctx.handle, mode, n, *[_ptr(c) for c in cols], float(radius), _ptr(pf), len(fields), _ptr(ro),
                                          int(vo.numel()) - 1, _ptr(vo), int(x.numel()), _ptr(x), _ptr(y), *[_ptr(out[k]) for k, _ in OUTS]))
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want):
    for k in ('word', 'rank', 'crossings', 'field_status'):
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:8])
    for k in ('seg', 'len'):
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, np.argwhere(bits(got[k]) != bits(want[k]))[:8])


def random_pairs(seed, n):
    rng = np.random.default_rng(seed)
    frm = np.column_stack([rng.uniform(3, 27, n), rng.uniform(3, 27, n), rng.uniform(-np.pi, np.pi, n)])
    d, a = rng.uniform(2.0, 14.0, n), rng.uniform(-np.pi, np.pi, n)
    to = np.column_stack([np.clip(frm[:, 0] + d * np.cos(a), 2, 28), np.clip(frm[:, 1] + d * np.sin(a), 2, 28), rng.uniform(-np.pi, np.pi, n)])
    return frm, to


# ---- 1. device equals host twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize('grouped', [True, False])
def test_device_equals_the_host_twin(gpu, mode, n, grouped):
    frm, to = random_pairs(3 + n + mode, n)
    rng = np.random.default_rng(n)
    pair_field = rng.integers(-1, len(FIELDS) + 1, n)                   # -1 and len(FIELDS): no region, out of range
    if n == 1:
        pair_field[:] = 4
    if n >= 63:
        pair_field[:9] = [6, -1, 0, 4, 3, 1, -2, 7, 5]
        to[11, 0] = np.nan                                              # unsolved pairs
        frm[12, 2] = np.nan
    if grouped:
        o = np.argsort(pair_field, kind='stable')
        frm, to, pair_field = frm[o], to[o], pair_field[o]
    want = host_solve_clear(mode, frm, to, R, pair_field, FIELDS)
    got = device_solve_clear(gpu, mode, frm, to, R, pair_field, FIELDS)
    same(got, want)
    assert np.array_equal(want['field_status'], [0, 0, L.EINVAL, 0, 0, L.EINVAL, 0])
    if n >= 257:
        # every kind of result occurs, and the big regions decide some of each
        big = np.isin(pair_field, (1, 3, 6))
        assert (want['rank'] >= 1).any() and (want['rank'][big] == -1).any() and (want['rank'][big] == 0).any()
        assert n < 1000 or (want['rank'][big] >= 1).any()
        assert ((want['rank'] == -1) & (want['crossings'] > 0)).any() and (want['word'] == -1).sum() == 2
        listed, _ = passes(gpu[0])
        assert listed >= np.count_nonzero(want['rank'] >= 1)


@pytest.mark.parametrize('mode', [0, 1])
def test_region_of_259_rings(gpu, mode):
    """the region of tests/test_clearance_host.py whose rings 256 .. 258 decide answers, its copies with the LAST ring spoilt, and the
    region without those rings: ranks, words and crossings as the twin gives them, and the spoilt regions' status"""
    from tests.test_clearance_host import MANY_RINGS, MANY_RINGS_CUT, many_ring_pairs, many_ring_region
    fields = [MANY_RINGS, many_ring_region('short'), MANY_RINGS_CUT, many_ring_region('nan')]
    frm, to = many_ring_pairs()
    n = len(frm)
    frm, to, pair_field = np.tile(frm, (4, 1)), np.tile(to, (4, 1)), np.repeat(np.arange(4), n)
    want = host_solve_clear(mode, frm, to, R, pair_field, fields)
    assert want['field_status'].tolist() == [0, L.EINVAL, 0, L.EINVAL]
    full, cut = want['rank'][:n], want['rank'][2 * n:3 * n]
    assert (full != cut).sum() >= 2 and (full == 0).sum() >= 20 and (full >= 1).any() and (full == -1).any()
    same(device_solve_clear(gpu, mode, frm, to, R, pair_field, fields), want)


# ---- 2. the list between the passes --------------------------------------------------------------------------------------------------
WIDE = [(-40, -40), (40, -40), (40, 40), (-40, 40)]


def _batch(n, blocked):
    """n pairs in WIDE-sized fields: straight 2 m moves, clear of field 0 (WIDE); the pairs named in `blocked` are the U-turn beside the wall of
    tests/test_solve_clear_host.py against field 1 (U_WALL), which the first pass has to list"""
    rng = np.random.default_rng(n)
    frm = np.column_stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-np.pi, np.pi, n)])
    to = np.column_stack([frm[:, 0] + 2.0 * np.cos(frm[:, 2]), frm[:, 1] + 2.0 * np.sin(frm[:, 2]), frm[:, 2]])
    pf = np.zeros(n, np.int64)
    for i in blocked:
        frm[i], to[i], pf[i] = U_TURN[0][0], U_TURN[1][0], 1
    return frm, to, pf


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n, blocked', [(200, ()), (70, tuple(range(70))), (65, (64,)), (129, (63, 64, 128))])
def test_the_list_between_the_passes(gpu, mode, n, blocked):
    frm, to, pf = _batch(n, blocked)
    want = host_solve_clear(mode, frm, to, 6.0, pf, [WIDE, U_WALL])
    _, before = passes(gpu[0])
    got = device_solve_clear(gpu, mode, frm, to, 6.0, pf, [WIDE, U_WALL])
    listed, after = passes(gpu[0])
    same(got, want)
    rest = np.setdiff1d(np.arange(n), blocked)
    assert (want['rank'][rest] == 0).all()
    assert (want['rank'][list(blocked)] >= 1).all()                      # the mirror word rescues the U-turn
    assert listed == len(blocked)                                        # exactly the pairs whose shortest word is inside and crosses
    assert after - before == (1 if blocked else 0)                       # nothing listed: the second launch is skipped


# ---- 5. engine -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reversing', [False, True])
def test_clear_connectors_against_the_abi(reversing):
    import torch
    mode = 1 if reversing else 0
    frm, to = random_pairs(77, 300)
    pair_field = np.random.default_rng(5).integers(-1, len(FIELDS), 300)
    want = host_solve_clear(mode, frm, to, R, pair_field, FIELDS)
    c = E.clear_connectors(frm, to, FIELDS, pair_field, R, reversing=reversing)
    got = dict(word=c.word, seg=c.seg, len=c.length, rank=c.rank, crossings=c.crossings, field_status=c.field_status)
    same({k: v.cpu().numpy() for k, v in got.items()}, want)
    solve = E.rs_solve if reversing else E.dubins_solve
    assert torch.equal(c.shortest_length, solve(frm, to, R)[2])
    assert bool((c.length >= c.shortest_length).all()) and bool((c.length[c.rank >= 1] > 0).all()) and bool((c.rank >= 1).any())
    # the chosen words through the existing samplers: every path starts at its start pose and ends on its goal
    out = c.paths(0.25)
    x, y, off = out[0].cpu().numpy(), out[1].cpu().numpy(), out[-1].cpu().numpy()
    assert len(off) == 301 and off[-1] == len(x)
    assert np.allclose(x[off[:-1]], frm[:, 0], atol=1e-9) and np.allclose(y[off[:-1]], frm[:, 1], atol=1e-9)
    assert np.allclose(x[off[1:] - 1], to[:, 0], atol=1e-9) and np.allclose(y[off[1:] - 1], to[:, 1], atol=1e-9)
    # and through the existing clearance: rank >= 0 is clear, rank -1 (a solved pair in a valid field) is not
    word, seg = c.word, c.seg
    ctx = E.get_context(None)
    dev = word.device
    ro, vo, fx, fy = (_t(a, dev) for a in pack(FIELDS))
    f = [_t(frm[:, k], dev) for k in range(3)]
    crossings = torch.empty(300, dtype=torch.int32, device=dev)
    inside = torch.empty(300, dtype=torch.int8, device=dev)
    L.check(ctx.lib.fcpp_conn_clear(ctx.handle, mode, 300, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), R, _ptr(word), _ptr(seg), _ptr(_t(pair_field.astype(np.int64), dev)),
                                    len(FIELDS), _ptr(ro), int(vo.numel()) - 1, _ptr(vo), int(fx.numel()), _ptr(fx), _ptr(fy), _ptr(crossings),
                                    _ptr(inside), None, None))
    clear = ((inside == 1) & (crossings == 0)).cpu().numpy()
    assert np.array_equal(clear, want['rank'] >= 0)
