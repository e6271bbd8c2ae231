"""The STEP (fcpp_batch_run, fcpp_batch_plan and its direct step) and the remaining device entries on watched buffers (run with -m gpu on an
MI355X): every point written, none beside it.

In mode 1 the step's points are a partition handed to five kernels (k_plan_quiet_spans, k_plan_quiet, k_plan_sparse, k_plan_sparse_fields
with its fused spans, k_plan_fused); the tilers cut it on the host and on the device, the direct step from the counting pass's packs.  The
other step tests compare against the oracle, and one path against another, on memory that is recycled between the two sides: a point that
nobody writes may still hold the right bits of the run before.  Here, in three ways, it cannot:

  1 the step on an arena (tests/guarded.py): fcpp_batch_run called directly with x, y, kappa, v (float64 slots at = 8 mod 16), flagseg (a uint32
    slot at = 4 mod 8) and the statistics rows (int64) of ONE guarded arena, pre-filled with 0x5A, guards of 0xA5 around every slot, in mode
    1 and in mode 0.  The expected bits are the same batch's run of that mode into ordinary allocations PRE-FILLED with the byte 0xC3, of
    which no element may be left, and which are compared with the oracle by tests/test_gpu_parity.py's comparisons at its tolerances.  The
    cases' stage_points() and point_split() are asserted, and together they give every one of the five point stages work.
  2 the one-call plan and its direct step into arena memory that was poisoned with 0x5A and freed: first fit hands the same place back, the
    32 elements behind every array stay poisoned, none of the points does, and the direct step's bits are the checker's (FCPP_DIRECT=0).
  3 the remaining batch entries and the old standalone operators, each once through the arena: fcpp_batch_connectors and fcpp_corner_turns
    with a mask of the elements they must leave alone, fcpp_batch_trajectory, fcpp_verify, fcpp_validate, fcpp_cover_grid, fcpp_fresnel,
    fcpp_straight_segments; entries whose outputs may be NULL once with all of them and once with one.
tests/test_guarded_host.py shows on the CPU what the arena's check catches."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import oracle as orc
from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from field_coverage_path_planning_amd import workloads as WL
from tests import test_gpu_parity as T
from tests.guarded import Arena
from tests.support import np_of as _np
from tests.test_gpu_cover import _box
from tests.test_gpu_guarded import PATH_LENS, gpu, paths      # noqa: F401  (gpu, paths: fixtures)

pytestmark = pytest.mark.gpu

POINT_ARRAYS = ('x', 'y', 'kappa', 'v', 'flagseg')
POINT_STAGES = ('k_plan_quiet_spans', 'k_plan_quiet', 'k_plan_sparse', 'k_plan_sparse_fields', 'k_plan_fused')
C3_F64 = np.frombuffer(bytes([0xC3] * 8), dtype=np.int64)[0]
C3_U32 = np.frombuffer(bytes([0xC3] * 4), dtype=np.uint32)[0]
SLOW_VP = T.DEFAULT_VP[:6] + [0.01] + T.DEFAULT_VP[7:]          # max_longitudinal_accel = 0.01: no turn is closed form


# ---- 1: the step on an arena ------------------------------------------------------------------------------------------------------------
def _small_rectangles():
    """24 rectangles of 90 .. 300 m (more than the 16 fields below which a batch is set up by the host), two fields that raise in the middle
    (MLP:597-598: 15 x 200 m, 10 x 10 m: no points, a statistics row of zeros)"""
    rng = np.random.default_rng(2025)
    LH = [(float(a), float(b)) for a, b in rng.uniform(90.0, 300.0, size=(24, 2))]
    LH[11], LH[12] = (15.0, 200.0), (10.0, 10.0)
    specs = [E.FieldSpec(field_length=a, field_width=b) for a, b in LH]
    ofs = [orc.make_field(L=a, H=b) for a, b in LH]
    return specs, ofs


def _dense_rectangles():
    LH = [(200.0, 150.0, None), (150.0, 100.0, (140.0, 90.0)), (120.0, 90.0, None)]
    specs = [E.FieldSpec(field_length=a, field_width=b, start_point=s) for a, b, s in LH]
    ofs = [orc.make_field(L=a, H=b, start=s) for a, b, s in LH]
    return specs, ofs


def _obstacle_fields():
    """tests/test_gpu_parity.py's fields with obstacles inside the work area: a rectangle, and a tilted parallelogram whose U-turns leave it"""
    return T._clip_fields()


# name -> (fields, vehicle, options, setup, FCPP_FIELD_WORK, tolerances, the point stages that must have points (others: any))
CASES = {
    'default, device setup': (_small_rectangles, T.DEFAULT_VP, {}, 'device', None, 'default', ('k_plan_quiet_spans', 'k_plan_sparse_fields')),
    'FCPP_FIELD_WORK=0, host setup': (_small_rectangles, T.DEFAULT_VP, {}, 'host', '0', 'default', ('k_plan_quiet_spans', 'k_plan_sparse')),
    'dense 0.1 m': (_dense_rectangles, T.DEFAULT_VP, dict(sample_spacing=0.1), 'host', None, 'dense', ('k_plan_quiet_spans', 'k_plan_quiet', 'k_plan_fused')),
    'a_lon 0.01': (_small_rectangles, SLOW_VP, {}, 'device', None, 'default', ('k_plan_sparse',)),
    'obstacles, flagged': (_obstacle_fields, T.DEFAULT_VP, {}, 'host', None, 'default', ('k_plan_quiet_spans', 'k_plan_sparse', 'k_plan_sparse_fields')),
    'obstacles, avoided': (_obstacle_fields, T.DEFAULT_VP, dict(avoid_obstacles=True), 'host', None, 'dense', ('k_plan_sparse',)),
    'clothoid turns': (_small_rectangles, T.DEFAULT_VP, dict(turn_model=1), 'device', None, 'dense', ('k_plan_quiet_spans', 'k_plan_sparse_fields')),
}


class Case:
    """a case's batch (created ONCE), the oracle's plans, and per mode the step's result in ordinary allocations pre-filled with 0xC3"""

    def __init__(self, name):
        import torch
        make, vp, opt, setup, field_work, tols, self.stages = CASES[name]
        self.name = name
        specs, ofs = make()
        o = E.make_options(**opt)
        ctx = E.get_context()
        if field_work is not None:
            os.environ['FCPP_FIELD_WORK'] = field_work          # (read when a batch is created)
        # 'device' is what 'auto' chooses for these batches: the path is asserted, not forced
        ctx.set_setup('host' if setup == 'host' else 'auto')
        try:
            self.batch = E.Batch(specs, T._veh(vp), o)
        finally:
            ctx.set_setup('auto')
            if field_work is not None:
                del os.environ['FCPP_FIELD_WORK']
        assert self.batch.setup_path() == setup, name
        self.plans = T._oracle_plans(ofs, vp, o)
        self.tols = T._dense_tols(opt) if tols == 'dense' else (T.XY_TOL, T.K_TOL, T.V_TOL)
        self.dev = torch.device('cuda', ctx.device)
        self._want = {}

    def filled(self):
        """six ordinary tensors, one per array, every byte 0xC3"""
        import torch
        b, n = self.batch, self.batch.total_points
        raw = lambda nbytes: torch.full((nbytes,), 0xC3, dtype=torch.uint8, device=self.dev)
        return tuple(raw(8 * n).view(torch.float64) for _ in range(4)) + (raw(4 * n).view(torch.int32),
                                                                           raw(8 * b.n_fields * L.STATS_WORDS).view(torch.int64).view(b.n_fields, L.STATS_WORDS))

    def want(self, mode):
        """-> {array: bits} of the step in mode `mode` into pre-filled ordinary allocations: nothing of the pre-fill is left, and the values are
        the oracle's (tests/test_gpu_parity.py's comparisons and tolerances)"""
        if mode not in self._want:
            import torch
            res = self.batch.run(self.filled(), mode=mode)
            torch.cuda.synchronize()
            out = {k: _np(getattr(res, k)) for k in POINT_ARRAYS[:4]}
            out['flagseg'] = _np(res.flagseg).view(np.uint32)
            out['stats'] = _np(res.stats_raw).reshape(-1)
            for k, a in out.items():
                left = np.flatnonzero((a.view(np.int64) if a.dtype != np.uint32 else a) == (C3_U32 if a.dtype == np.uint32 else C3_F64))
                assert left.size == 0, '%s, mode %d: %d elements of %s were not written, the first %d' % (self.name, mode, left.size, k, left[0])
            T._compare_result_with_oracle(self.batch, res, self.plans, *self.tols)
            self._want[mode] = out
        return self._want[mode]


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope='module', autouse=True)
def _close_cases():
    yield
    for c in _cases.values():
        c.batch.close()
    _cases.clear()


def _stage_points(batch):
    """stage_points() of the fused pipeline, whichever mode ran last"""
    keep, batch._last_mode = batch._last_mode, 1
    try:
        return batch.stage_points()
    finally:
        batch._last_mode = keep


@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('name', list(CASES))
def test_step_on_an_arena(gpu, name, mode):
    c = _case(name)
    b, n = c.batch, c.batch.total_points
    assert 0 < n <= 300_000
    want = c.want(mode)
    A = Arena()
    for k in POINT_ARRAYS[:4]:
        A.output(k, np.float64, n)
    A.output('flagseg', np.uint32, n).output('stats', np.int64, b.n_fields * L.STATS_WORDS).build(gpu.dev)
    assert all(A.address(k) % 16 == 8 for k in POINT_ARRAYS[:4] + ('stats',)) and A.address('flagseg') % 8 == 4
    gpu.ctx.bind_stream()
    gpu.ok(gpu.lib.fcpp_batch_run(b.handle, *[A.ptr(k) for k in POINT_ARRAYS], A.ptr('stats'), mode))
    A.check(want)


@pytest.mark.parametrize('name', list(CASES))
def test_the_cases_are_what_they_claim(name):
    """a condition on the inputs: the split of the points among the fused pipeline's kernels, and what each case is there for"""
    c = _case(name)
    b = c.batch
    sp, (quiet, general) = _stage_points(b), b.point_split()
    print('\n%s: %d points, stage_points %r, point_split %r, reduce_classes %r' % (name, b.total_points, sp, (quiet, general), b.reduce_classes()))
    assert sp['k_reduce_stats'] == b.total_points == quiet + general
    assert sum(sp[k] for k in POINT_STAGES) == b.total_points          # a partition
    assert all(sp[k] >= 0 for k in POINT_STAGES)
    for k in c.stages:
        assert sp[k] > 0, (name, k, sp)
    info = b.info.array
    if name == 'default, device setup':
        ok = info['status'] == 0
        assert not ok[11] and not ok[12] and ok.sum() == 22 and (info['n_main'] + info['n_head'])[~ok].sum() == 0
        assert not c.want(1)['stats'].reshape(-1, L.STATS_WORDS)[[11, 12]].any()
        # fields begin on even AND on odd global point indices (the quiet writer pairs its stores from an even index on: its `odd` branch)
        assert set(info['point_offset'][ok] % 2) == {0, 1}
    if name == 'FCPP_FIELD_WORK=0, host setup':
        assert sp['k_plan_sparse_fields'] == 0 and sum(b.reduce_classes()) >= 22          # every field with points reduced by k_reduce_stats
    if name == 'a_lon 0.01':
        assert quiet == 0          # no closed-form span, no closed-form run
    if name.startswith('obstacles'):
        st = c.want(1)['stats'].reshape(-1, L.STATS_WORDS)
        fs = c.want(1)['flagseg']
        assert st[1, 10] > 0 and int(((fs & L.FLAG_OUTSIDE) != 0).sum()) == st[:, 10].sum()          # the skewed field's path leaves its polygon
        if name.endswith('avoided'):
            assert b.options.obstacle_mode == L.OBSTACLES_AVOID and int(((fs & L.KIND_MASK) == L.KIND_DETOUR).sum()) > 0


def test_every_point_stage_has_points_in_some_case():
    total = dict.fromkeys(POINT_STAGES, 0)
    for name in CASES:
        sp = _stage_points(_case(name).batch)
        for k in POINT_STAGES:
            total[k] += sp[k]
    assert all(total[k] > 0 for k in POINT_STAGES), total


# ---- 2: the one-call plan and the direct step on poisoned arena memory -----------------------------------------------------------------------
TAIL = 32
LANE = 64 << 20


def _view(ptr, n, typestr, dev):
    import torch
    return torch.as_tensor(E._ArenaArrays._View(None, ptr, n, typestr), device=dev)


def _views(ptrs, n, dev):
    return [_view(p, n, '<f8' if k < 4 else '<i4', dev) for k, p in enumerate(ptrs)]


def _poison(gpu, n):
    """five arena arrays of n points filled with 0x5A and freed again -> their addresses"""
    import torch
    ptrs = [C.c_void_p() for _ in range(5)]
    gpu.ok(gpu.lib.fcpp_outputs_alloc(gpu.h, n, 0, *[C.byref(q) for q in ptrs]))
    ptrs = [q.value for q in ptrs]
    lane, pitch, _ = gpu.ctx.outputs_info()
    assert all(ptrs[k + 1] - ptrs[k] == pitch for k in range(4)), 'the arrays come from the arena'
    for t in _views(ptrs, n, gpu.dev):
        t.view(torch.uint8).fill_(0x5A)
    gpu.ok(gpu.lib.fcpp_outputs_free(gpu.h, C.c_void_p(ptrs[0])))
    assert gpu.ctx.outputs_info()[2] == 0
    return ptrs


def _plan_call(gpu, table, stats_ptr, direct):
    """fcpp_batch_plan itself (E.Batch.plan brings no statistics records of the caller's) -> (batch handle, the five addresses, points)"""
    arr, polys, _keep = E.pack_fields(table)
    veh, opt = E.make_vehicle(), E.make_options()
    h, tot = C.c_void_p(), C.c_int64()
    ptrs = [C.c_void_p() for _ in range(5)]
    if not direct:
        os.environ['FCPP_DIRECT'] = '0'          # (read per call)
    try:
        gpu.ctx.bind_stream()
        gpu.ok(gpu.lib.fcpp_batch_plan(gpu.h, C.byref(veh), C.byref(opt), len(table), arr, C.byref(polys), stats_ptr, C.byref(h),
                                       *[C.byref(q) for q in ptrs], C.byref(tot)))
    finally:
        if not direct:
            del os.environ['FCPP_DIRECT']
    return h, [q.value for q in ptrs], tot.value


def _poisoned_plan(gpu, n_fields, direct, stats_arena=None):
    """poison, plan, look -> {array: the first total_points elements}, 'stats' among them; the tails and the placement are asserted here"""
    import torch
    table = E.FieldTable.from_rectangles(WL.cfg1_batch(n_fields))
    n = int(E.plan_points(table, E.make_vehicle(), E.make_options()).sum())
    poisoned = _poison(gpu, n + TAIL)
    counts = gpu.ctx.direct_counts()
    h, ptrs, total = _plan_call(gpu, table, stats_arena.ptr('stats') if stats_arena else None, direct)
    try:
        steps, taken, fills = gpu.ctx.direct_counts()
        if direct:
            assert (steps, taken, fills) == (counts[0] + 1, counts[1] + 1, counts[2]), 'the call took the direct step: no fill pass, no run'
        else:
            assert steps == counts[0], 'FCPP_DIRECT=0 launches no direct step'
        assert total == n and ptrs == poisoned, 'first fit: the arrays lie where the poisoned ones lay'
        torch.cuda.synchronize()
        got = {}
        for name, t in zip(POINT_ARRAYS, _views(ptrs, n + TAIL, gpu.dev)):
            a = _np(t)
            a = a.view(np.uint32) if name == 'flagseg' else a
            bits = a.view(np.int64) if name != 'flagseg' else a
            pattern = np.frombuffer(bytes([0x5A] * a.itemsize), dtype=bits.dtype)[0]
            left = np.flatnonzero(bits[:n] == pattern)
            assert left.size == 0, '%s: %d of %d points still hold the poison, the first element %d' % (name, left.size, n, left[0])
            hit = np.flatnonzero(bits[n:] != pattern)
            assert hit.size == 0, '%s: element %d behind the end was written' % (name, hit[0])
            got[name] = a[:n].copy()
        if stats_arena is None:
            sp = C.c_void_p()
            gpu.ok(gpu.lib.fcpp_batch_own_stats(h, C.byref(sp)))
            got['stats'] = _np(_view(sp.value, n_fields * L.STATS_WORDS, '<i8', gpu.dev)).copy()
    finally:
        gpu.ok(gpu.lib.fcpp_batch_destroy(h))
        gpu.ok(gpu.lib.fcpp_outputs_free(gpu.h, C.c_void_p(ptrs[0])))
    return got


@pytest.fixture
def small_arena(gpu):
    """a small output arena; whatever earlier tests left of plan results is collected first (no live allocation may remain)"""
    gc.collect()
    gpu.ctx.reserve_outputs(lane_gib=LANE / 2**30, pitch_gib=LANE / 2**30)
    try:
        assert gpu.ctx.outputs_info() == (LANE, LANE, 0)
        yield gpu
    finally:
        gc.collect()
        L.check(gpu.lib.fcpp_ctx_reserve_outputs(gpu.h, 4096, 4096))       # (back to next to nothing for the tests that follow)


@pytest.mark.parametrize('n_fields', [16, 65])
def test_plan_and_direct_step_on_poisoned_arena_memory(small_arena, n_fields):
    gpu = small_arena
    # the checker, run the same way: it also leaves the context's verdict "qualifies" for the direct call
    want = _poisoned_plan(gpu, n_fields, direct=False)
    got = _poisoned_plan(gpu, n_fields, direct=True)
    for k in POINT_ARRAYS + ('stats',):
        bad = np.flatnonzero(got[k].view(np.int64 if k != 'flagseg' else np.uint32) != want[k].view(np.int64 if k != 'flagseg' else np.uint32))
        assert bad.size == 0, '%s: %d elements differ from the checker, the first element %d' % (k, bad.size, bad[0])
    # a caller's statistics records, from a guarded arena
    A = Arena().output('stats', np.int64, n_fields * L.STATS_WORDS).build(gpu.dev)
    got = _poisoned_plan(gpu, n_fields, direct=True, stats_arena=A)
    A.check({'stats': want['stats']})
    for k in POINT_ARRAYS:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


# ---- 3: the remaining batch entries and the old operators -------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pointed_batch():
    """fields with and without kept start / end points, one that raises, one whose points lie outside (not kept) -> (batch, result arrays)"""
    import torch
    specs = [E.FieldSpec(field_length=200.0, field_width=100.0, start_point=(10.0, 10.0), end_point=(190.0, 90.0)),
             E.FieldSpec(field_length=120.0, field_width=80.0),
             E.FieldSpec(field_length=15.0, field_width=200.0, start_point=(1.0, 1.0)),
             E.FieldSpec(field_length=150.0, field_width=90.0, start_point=(100.0, 50.0)),
             E.FieldSpec(field_length=120.0, field_width=80.0, start_point=(500.0, 10.0), end_point=(60.0, 40.0)),
             E.FieldSpec(field_length=95.0, field_width=130.0, end_point=(5.0, 120.0))]
    b = E.Batch(specs, E.make_vehicle(), E.make_options())
    r = b.run()
    torch.cuda.synchronize()
    yield b, r
    b.close()


def test_batch_connectors(gpu, pointed_batch):
    b, _ = pointed_batch
    info = b.info.array
    ok = info['status'] == 0          # (field 2 raises: its start point is kept on record, its row is not written)
    kept = {'approach': ok & (info['start_kept'] != 0), 'departure': ok & (info['end_kept'] != 0)}
    assert not ok[2] and info['start_kept'][2] != 0 and kept['approach'].tolist() == [True, False, False, True, False, False] and kept['departure'].tolist() == [True, False, False, False, True, True]
    ap, dp = b.connectors()
    want = {'approach': _np(ap).reshape(-1), 'departure': _np(dp).reshape(-1)}
    for k in want:      # (the engine pre-fills with NaN: exactly the rows of fields without a kept point stay NaN)
        assert np.array_equal(np.isnan(want[k]).reshape(b.n_fields, 100).all(axis=1), ~kept[k]) and not np.isnan(want[k].reshape(b.n_fields, 100)[kept[k]]).any()
    for outs in (('approach', 'departure'), ('departure',)):
        A = Arena()
        for k in outs:
            A.output(k, np.float64, b.n_fields * 100, keep=np.repeat(~kept[k], 100))
        A.build(gpu.dev)
        gpu.ctx.bind_stream()
        gpu.ok(gpu.lib.fcpp_batch_connectors(b.handle, A.ptr('approach'), A.ptr('departure')))
        A.check({k: want[k] for k in outs})


def test_batch_trajectory(gpu, pointed_batch):
    b, r = pointed_batch
    s, t, h, totals = (_np(a) for a in r.trajectory())
    want = {'s': s, 't': t, 'heading': h, 'totals': totals.reshape(-1)}
    names = ('s', 't', 'heading', 'totals')
    n = b.total_points
    for outs in (names, ('totals',), ('s',)):
        A = Arena().input('x', _np(r.x)).input('y', _np(r.y)).input('v', _np(r.v)).input('fs', _np(r.flagseg).view(np.uint32))
        for k in outs:
            A.output(k, np.float64, 4 * b.n_fields if k == 'totals' else n)
        A.build(gpu.dev)
        gpu.ctx.bind_stream()
        gpu.ok(gpu.lib.fcpp_batch_trajectory(b.handle, A.ptr('x'), A.ptr('y'), A.ptr('v'), A.ptr('fs'), *[A.ptr(k) for k in names]))
        A.check({k: want[k] for k in outs})


def _raw_stats(d):
    """the statistics records of engine.verify / engine.validate back as the words the library wrote"""
    return np.column_stack([np.ascontiguousarray(d[n]).view(np.int64) for n, _ in L.FieldStats._fields_]).reshape(-1)


def test_verify(gpu, paths):
    off, x, y, v, fs = paths
    veh = E.make_vehicle()
    want = _raw_stats(E.verify(x, y, v, veh, offsets=off))
    n_paths = len(off) - 1
    assert n_paths == len(PATH_LENS)
    for with_host in (True, False):
        A = Arena().input('off', off).input('x', x).input('y', y).input('v', v).output('stats', np.int64, n_paths * L.STATS_WORDS).build(gpu.dev)
        gpu.ok(gpu.lib.fcpp_verify(gpu.h, C.byref(veh), n_paths, A.ptr('off'), len(x), A.ptr('x'), A.ptr('y'), A.ptr('v'), A.ptr('stats'),
                                   E._host_ptr(off if with_host else None)))
        A.check({'stats': want})


def test_validate(gpu, paths):
    off, x, y, v, fs = paths
    veh, opt = E.make_vehicle(), E.make_options(geofence_tol=1e-6)
    n_paths = len(off) - 1
    # a geofence per path: a box that cuts 30 % off the path's extent in x (a path of no points: any box), and two obstacles where the
    # two longest paths spend their time
    fields = []
    for a, b in zip(off[:-1], off[1:]):
        px, py = (x[a:b], y[a:b]) if b > a else (np.zeros(1), np.zeros(1))
        x0, x1, y0, y1 = px.min() - 0.5, px.max() - 0.3 * np.ptp(px) + 0.5, py.min() - 0.5, py.max() + 0.5
        fields.append([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])
    (bx, by), (tx, ty) = (np.median(a[off[9]:off[10]]) for a in (x, y)), (np.median(a[off[7]:off[8]]) for a in (x, y))
    obstacles = [[(bx - 3.0, by - 3.0), (bx + 3.0, by - 3.0), (bx + 3.0, by + 3.0), (bx - 3.0, by + 3.0)], [(tx - 2.0, ty - 1.5), (tx + 2.0, ty - 1.0), (tx, ty + 2.0)]]
    flags, st = E.validate(x, y, v, veh, field_polygons=fields, obstacles=obstacles, offsets=off)
    want = {'flags': _np(flags).view(np.uint32), 'stats': _raw_stats(st)}
    assert st['n_outside'].sum() > 0 and st['n_in_obstacle'].sum() > 0
    fp, keep1 = E._polys(fields)
    ob, keep2 = E._polys(obstacles)
    for with_host in (True, False):
        A = Arena().input('off', off).input('x', x).input('y', y).input('v', v)
        A.output('flags', np.uint32, len(x)).output('stats', np.int64, n_paths * L.STATS_WORDS).build(gpu.dev)
        gpu.ok(gpu.lib.fcpp_validate(gpu.h, C.byref(veh), C.byref(opt), n_paths, A.ptr('off'), len(x), A.ptr('x'), A.ptr('y'), A.ptr('v'), C.byref(fp),
                                     C.byref(ob), None, A.ptr('flags'), A.ptr('stats'), E._host_ptr(off if with_host else None)))
        A.check(want)


def test_cover_grid(gpu):
    """three jobs of tests/test_gpu_cover.py's ragged shapes (one row of lanes; more than a tile both ways; exactly a tile), cell corners and
    centres, strict and closed, one with a region: flag bytes and counts are the oracle's, with the grid and with the counts alone"""
    rng = np.random.default_rng(78)
    jobs, pts, want_c, want_g, first, gfirst = [], [], [], [], 0, 0
    for n, (nx, ny) in enumerate([(1, 70), (65, 130), (64, 64)]):
        res = (0.1, 0.25, 0.037)[n]
        ox, oy = rng.uniform(-50, 50, 2)
        w, h = nx * res, ny * res
        na, nb = (7, 2, 40)[n], (0, 25, 2)[n]
        a = np.column_stack([rng.uniform(ox - 0.2 * w, ox + 1.2 * w, na), rng.uniform(oy - 0.2 * h, oy + 1.2 * h, na)])
        if na > 5:
            a[3] = a[2]                               # a zero-length segment
        b = np.column_stack([rng.uniform(ox, ox + w, nb), rng.uniform(oy, oy + h, nb)])
        radius = float(rng.uniform(0.05, 0.3) * max(w, h))
        shift, strict = (0.5 if n % 2 else 0.0), n != 0
        region = (_box(ox + 0.1 * w, oy + 0.1 * h, ox + 0.9 * w, oy + 0.8 * h), _box(ox + 0.3 * w, oy + 0.3 * h, ox + 0.6 * w, oy + 0.5 * h)) if n == 1 else None
        jobs.append(E.make_cover_job(ox, oy, res, nx, ny, radius, na, nb, pts_first=first, grid_first=gfirst, shift=shift, strict=strict,
                                     outer=region[0] if region else None, inner=region[1] if region else None))
        wc, wg = orc.cover_grid(ox, oy, res, shift, radius, nx, ny, a, b, strict=strict, region=(list(region[0]) + list(region[1])) if region else None)
        want_c.append(np.asarray(wc, dtype=np.int64))
        want_g.append(np.asarray(wg, dtype=np.uint8).reshape(-1))
        pts += [a, b]
        first += na + nb
        gfirst += nx * ny
    xy = np.vstack(pts)
    want = {'grid': np.concatenate(want_g), 'counts': np.concatenate(want_c)}
    assert (want['counts'].reshape(-1, 3)[:, 0] > 0).all() and (want['grid'] != 0).any() and (want['grid'] == 0).any()
    for outs in (('grid', 'counts'), ('counts',)):
        if 'grid' not in outs:
            for j in jobs:
                j.grid_first = -1
        A = Arena().input('px', xy[:, 0]).input('py', xy[:, 1])
        if 'grid' in outs:
            A.output('grid', np.uint8, gfirst)
        A.output('counts', np.int64, 3 * len(jobs)).build(gpu.dev)
        arr = (L.CoverJob * len(jobs))(*jobs)
        gpu.ok(gpu.lib.fcpp_cover_grid(gpu.h, len(jobs), arr, len(xy), A.ptr('px'), A.ptr('py'), A.ptr('grid'), A.ptr('counts')))
        A.check({k: want[k] for k in outs})


@pytest.mark.parametrize('n', [1, 65, 257])
def test_fresnel_and_straight_segments(gpu, n):
    import torch
    rng = np.random.default_rng(300 + n)
    t = rng.uniform(-6.0, 6.0, n)
    c, s = E.fresnel(t)
    A = Arena().input('t', t).output('c', np.float64, n).output('s', np.float64, n).build(gpu.dev)
    gpu.ok(gpu.lib.fcpp_fresnel(gpu.h, n, A.ptr('t'), A.ptr('c'), A.ptr('s')))
    A.check({'c': _np(c), 's': _np(s)})
    segs = rng.uniform(-100.0, 100.0, (n, 4))
    for n_points in (2, 50):
        out = E.straight_segments(segs, n_points)
        A = Arena().input('seg', segs).output('out', np.float64, n * n_points * 2).build(gpu.dev)
        gpu.ok(gpu.lib.fcpp_straight_segments(gpu.h, n, A.ptr('seg'), n_points, A.ptr('out')))
        torch.cuda.synchronize()
        A.check({'out': _np(out).reshape(-1)})


def test_corner_turns(gpu, golden_cover):
    """the golden scenarios' corners, each with and without its reverse fill, mixed: a row holds counts[2k] + counts[2k+1] points, the rest of
    its `stride` points is left alone"""
    g = golden_cover
    names = ['working_width', 'min_turn_radius', 'max_work_speed_kmh', 'max_headland_speed_kmh', 'headland_turn_speed_kmh',
             'max_lateral_accel', 'max_longitudinal_accel', 'safety_factor']
    for name in g['names']:
        Lf, Hf = (float(a) for a in g[f'{name}/LH'])
        veh = E.make_vehicle(**dict(zip(names, g[f'{name}/vp'])))
        corners = np.array([g[f'{name}/c{ci}/corner'] for ci in range(4)] * 2, dtype=np.float64)
        index = np.array([0, 1, 2, 3] * 2, dtype=np.int32)
        rev = np.array([1, 0, 1, 0, 0, 1, 0, 1], dtype=np.int32)
        got = E.corner_turns(corners, index, rev, veh, Lf, Hf)          # an ordinary call: the golden polylines' device bits
        stride = 15 + max(10, int(3.0 * veh.min_turn_radius / 0.5))
        out = np.zeros((8, stride, 2))
        keep = np.ones((8, stride, 2), dtype=bool)
        counts = np.zeros((8, 2), dtype=np.int32)
        for k, (turn, fill) in enumerate(got):
            assert len(turn) == 15 and (fill is not None) == bool(rev[k])
            np.testing.assert_allclose(turn, g[f'{name}/c{k % 4}/turn'], rtol=0, atol=1e-9)
            if fill is not None:
                np.testing.assert_allclose(fill, g[f'{name}/c{k % 4}/rev'].reshape(-1, 2), rtol=0, atol=1e-9)
            m = 15 + (len(fill) if fill is not None else 0)
            out[k, :m] = turn if fill is None else np.vstack([turn, fill])
            keep[k, :m] = False
            counts[k] = (15, m - 15)
        assert keep.any() and m < stride
        A = Arena().input('corners', corners).input('index', index).input('rev', rev)
        A.output('out', np.float64, 8 * stride * 2).output('counts', np.int32, 16).build(gpu.dev)
        gpu.ok(gpu.lib.fcpp_corner_turns(gpu.h, C.byref(veh), 8, A.ptr('corners'), A.ptr('index'), A.ptr('rev'), Lf, Hf, stride, A.ptr('out'), A.ptr('counts')))
        A.check({'out': out.reshape(-1), 'counts': counts.reshape(-1)}, keep={'out': keep.reshape(-1)})
