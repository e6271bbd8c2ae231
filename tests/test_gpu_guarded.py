"""GPU tests of the standalone device entries through the guarded arena (run with -m gpu on an MI355X).

Every other device test hands an operator outputs that torch.empty sized exactly and 512-byte aligned, and compares values.  Here the C
entries are called directly (ctx.lib) on slots carved out of ONE uint8 CUDA tensor (tests/guarded.py): 256 bytes of 0xA5 around every
slot, outputs pre-filled with 0x5A, every pointer only naturally aligned and never 16-byte aligned.  After each call: the guards are intact
(no write outside an output), the inputs have the bits that were put in, and every output element has the bits of the expected value --
none of which is the pre-fill pattern, so an element that was never written cannot pass.  tests/test_guarded_host.py shows on the CPU that
this check catches an off-by-one write on either side, a skipped last element and a touched input.

Expected values: the host twins (fcpp_debug_*) bit for bit where one exists; for the samplers and the older path operators the engine's
own call on the same inputs with ordinary allocations (other tests pin those values: what is new is that they do not depend on where the
buffers lie).  Each family is called with all its outputs and again with strict subsets NULL -- the narrowest type alone, the first float64
array alone: the outputs passed equal the full call's, and nothing else is written."""
import ctypes as C

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.guarded import Arena
from tests.support import bits as _bits, Gpu as BaseGpu, np_of as _np
from tests.test_dubins_host import host_solve as dubins_host
from tests.test_gpu_properties import ragged_paths
from tests.test_gpu_trajectory import _fsw
from tests.test_guarded_host import (PAIR_OUTS, R_CONN, RECORD_OUTS, ROUTE_OUTS, ROUTE_S, ROUTE_SUBSETS, SAMPLE_N, SCORE_ANGLES,
                                     SOLVE_N, SOLVE_SUBSETS, SPACING, assert_permutations, cols, guarded_route, matrix_poses, matrix_shapes, record_values,
                                     route_solve_arena, route_transit_arena, route_values, solve_arena, solve_pairs, swath_cases, swath_head,
                                     swath_inputs)
from tests.test_route_host import MIN_GAIN, host_route
from tests.test_route_host import R as R_ROUTE
from tests.test_rs_host import host_solve as rs_host
from tests.test_swaths_host import host_cut, host_scores

pytestmark = pytest.mark.gpu


class Gpu(BaseGpu):
    def ok(self, rc):
        assert rc == L.OK, self.lib.fcpp_last_error()


@pytest.fixture
def gpu():
    g = Gpu()
    g.ctx.bind_stream()
    return g


# ---- the connectors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reversing', [False, True], ids=['dubins', 'rs'])
@pytest.mark.parametrize('n', SOLVE_N)
def test_solve(gpu, n, reversing):
    frm, to = solve_pairs(n, reversing)
    word, seg, tot = (rs_host if reversing else dubins_host)(frm, to, R_CONN)
    want = {'word': word, 'seg': seg.reshape(-1), 'len': tot}
    fn = gpu.lib.fcpp_rs_solve if reversing else gpu.lib.fcpp_dubins_solve
    for outs in SOLVE_SUBSETS:
        A, args = solve_arena(frm, to, 5 if reversing else 3, outs, gpu.dev)
        gpu.ok(fn(gpu.h, n, *args))
        A.check({k: want[k] for k in outs})


@pytest.mark.parametrize('reversing', [False, True], ids=['dubins', 'rs'])
@pytest.mark.parametrize('shape', [0, 1, 2])
def test_matrix(gpu, shape, reversing):
    nf, nt = matrix_shapes(reversing)[shape]
    assert shape < 2 or (nf == 33 and nt == 257)          # one row over the row tile of 32, one column over the 256 lanes
    f, t = matrix_poses(nf, nt)
    # entry (i, j) has the bits of the pair solve
    word, _, tot = (rs_host if reversing else dubins_host)(np.repeat(f, nt, axis=0), np.tile(t, (nf, 1)), R_CONN)
    want = {'D': tot, 'word': word.astype(np.int8)}
    assert (word >= 0).all() and (nf * nt < 100 or len(np.unique(word)) >= 4)
    fn = gpu.lib.fcpp_rs_matrix if reversing else gpu.lib.fcpp_dubins_matrix
    for outs in (('D', 'word'), ('word',), ('D',)):
        A = Arena()
        for name, a in zip(('fx', 'fy', 'fh', 'tx', 'ty', 'th'), cols(f) + cols(t)):
            A.input(name, a)
        if 'D' in outs:
            A.output('D', np.float64, nf * nt)
        if 'word' in outs:
            A.output('word', np.int8, nf * nt)
        A.build(gpu.dev)
        gpu.ok(fn(gpu.h, nf, A.ptr('fx'), A.ptr('fy'), A.ptr('fh'), nt, A.ptr('tx'), A.ptr('ty'), A.ptr('th'), R_CONN, A.ptr('D'), A.ptr('word')))
        A.check({k: want[k] for k in outs})


@pytest.mark.parametrize('reversing', [False, True], ids=['dubins', 'rs'])
def test_counts_and_sample(gpu, reversing):
    n = SAMPLE_N
    frm, to = solve_pairs(n, reversing)
    word, seg, tot = (rs_host if reversing else dubins_host)(frm, to, R_CONN)
    o = (E._rs_paths if reversing else E._dubins_paths)(gpu.ctx, frm, to, R_CONN, SPACING)          # ordinary allocations
    assert np.array_equal(_np(o['word']), word) and np.array_equal(_bits(_np(o['seg'])), _bits(seg)) and np.array_equal(_bits(_np(o['length'])), _bits(tot))
    off = np.ascontiguousarray(o['offsets_host'], dtype=np.int64)
    m = int(off[-1])
    assert 2000 < m < 20000 and np.array_equal(_np(o['offsets']), off)
    if not reversing:      # the count rule on the host twin's lengths
        K = np.floor(tot / SPACING).astype(np.int64) + 1
        assert np.array_equal(np.diff(off), K + ((K - 1) * SPACING < tot))
    # the offsets, with and without the host copy
    for with_host in (True, False):
        A = Arena().input('word', word).input('seg', seg).input('len', tot).output('offsets', np.int64, n + 1).build(gpu.dev)
        oh = np.full(n + 1, -7, dtype=np.int64)
        hp = E._host_ptr(oh if with_host else None)
        if reversing:
            gpu.ok(gpu.lib.fcpp_rs_counts(gpu.h, n, A.ptr('word'), A.ptr('seg'), SPACING, A.ptr('offsets'), hp))
        else:
            gpu.ok(gpu.lib.fcpp_dubins_counts(gpu.h, n, A.ptr('len'), SPACING, A.ptr('offsets'), hp))
        A.check({'offsets': off})
        assert np.array_equal(oh, off) if with_host else (oh == -7).all()
    # the samples
    want = {k: _np(o[k]) for k in ('x', 'y', 'heading', 'kappa')}
    names = ['x', 'y', 'heading', 'kappa']
    subsets = [tuple(names), ('x',), ('kappa',)]
    if reversing:
        want['gear'] = _np(o['gear'])
        names.append('gear')
        subsets = [tuple(names), ('gear',), ('x',)]
        assert set(np.unique(want['gear'])) == {-1, 1}
    for k, outs in enumerate(subsets):
        A = Arena()
        for name, a in zip(('fx', 'fy', 'fh'), cols(frm)):
            A.input(name, a)
        A.input('word', word).input('seg', seg).input('offsets', off)
        for name in outs:
            A.output(name, np.int8 if name == 'gear' else np.float64, m)
        A.build(gpu.dev)
        head = (gpu.h, n, A.ptr('fx'), A.ptr('fy'), A.ptr('fh'), R_CONN, A.ptr('word'), A.ptr('seg'), SPACING, A.ptr('offsets'), m)
        hp = E._host_ptr(off if k else None)          # (the full call has the library read the offsets back from the arena)
        if reversing:
            gpu.ok(gpu.lib.fcpp_rs_sample(*head, *[A.ptr(x) for x in names], hp))
        else:
            gpu.ok(gpu.lib.fcpp_dubins_sample(*head, *[A.ptr(x) for x in names], hp))
        A.check({name: want[name] for name in outs})


# ---- the polygon swaths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', swath_cases(), ids=lambda c: c[0])
def test_swaths(gpu, case):
    what, fields, angles, W, first = case
    lib = gpu.lib
    # the scores: three angles shared by the fields
    sc = host_scores(fields, SCORE_ANGLES, W, first)
    for outs in (tuple(k for k, _ in PAIR_OUTS), ('status',), ('length',)):
        A = Arena()
        n, nr, nv = swath_inputs(A, fields, SCORE_ANGLES)
        for k, dt in PAIR_OUTS:
            if k in outs:
                A.output(k, dt, n * 3)
        A.build(gpu.dev)
        gpu.ok(lib.fcpp_swath_scores(gpu.h, *swath_head(A, n, nr, nv), 3, A.ptr('angles'), W, first, 0.0, *[A.ptr(k) for k, _ in PAIR_OUTS]))
        A.check({k: sc[k].reshape(-1) for k in outs})
    # the counts: an angle per field
    cut = host_cut(fields, angles, W, first)
    m = int(cut['offsets'][-1])
    want = {'offsets': cut['offsets'], 'n_lines': cut['n_lines'], 'status': cut['status']}
    for outs in (('offsets', 'n_lines', 'status'), ('offsets', 'status'), ('offsets',)):
        A = Arena()
        n, nr, nv = swath_inputs(A, fields, angles)
        for k in outs:
            A.output(k, np.int64 if k == 'offsets' else np.int32, n + 1 if k == 'offsets' else n)
        A.build(gpu.dev)
        oh = np.full(n + 1, -7, dtype=np.int64)
        gpu.ok(lib.fcpp_swath_counts(gpu.h, *swath_head(A, n, nr, nv), A.ptr('angles'), W, first, 0.0, A.ptr('offsets'),
                                     E._host_ptr(oh if len(outs) == 3 else None), A.ptr('n_lines'), A.ptr('status')))
        A.check({k: want[k] for k in outs})
        assert np.array_equal(oh, cut['offsets']) if len(outs) == 3 else (oh == -7).all()
    # the records
    rec = record_values(cut)
    for outs in (tuple(rec), ('line',), ('ax',)):
        A = Arena()
        n, nr, nv = swath_inputs(A, fields, angles)
        A.input('offsets', cut['offsets'])
        for k, dt in RECORD_OUTS:
            if k in outs:
                A.output(k, dt, m)
        A.build(gpu.dev)
        gpu.ok(lib.fcpp_swath_fill(gpu.h, *swath_head(A, n, nr, nv), A.ptr('angles'), W, first, 0.0, A.ptr('offsets'), m,
                                   *[A.ptr(k) for k, _ in RECORD_OUTS]))
        A.check({k: rec[k] for k in outs})


# ---- the swath router -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1])
def test_route(gpu, guarded_route, mode):
    cut, per_mode = guarded_route
    T, toff, En, Xn = per_mode[mode]
    soff = cut['offsets']
    n, nt, tt = len(soff) - 1, int(soff[-1]), int(toff[-1])
    HP = E._host_ptr
    # (mode 1 has the library read both offset tables back from the arena)
    soff_h, toff_h = (HP(soff), HP(toff)) if mode == 0 else (HP(None), HP(None))
    A = route_transit_arena(cut, toff, gpu.dev)
    gpu.ok(gpu.lib.fcpp_route_transit(gpu.h, n, A.ptr('soff'), soff_h, nt, A.ptr('ax'), A.ptr('ay'), A.ptr('bx'), A.ptr('by'), A.ptr('angle'), R_ROUTE,
                                      mode, A.ptr('toff'), toff_h, tt, A.ptr('T')))
    A.check({'T': T})
    for with_ends in (True, False):
        E_, X_ = (En, Xn) if with_ends else (None, None)
        res = host_route(soff, T, toff, E_, X_, S=ROUTE_S, max_sweeps=3)
        want = route_values(res)
        assert np.all(res['status'] == 0) and res['sweeps'].max() >= 1
        assert_permutations(res['tours'], soff)
        for outs in ROUTE_SUBSETS if with_ends else ROUTE_SUBSETS[:1]:
            A = route_solve_arena(soff, toff, T, E_, X_, outs, gpu.dev)
            gpu.ok(gpu.lib.fcpp_route_solve(gpu.h, n, A.ptr('soff'), soff_h, nt, A.ptr('toff'), toff_h, tt, A.ptr('T'), A.ptr('E'), A.ptr('X'), ROUTE_S,
                                            MIN_GAIN, 3, *[A.ptr(k) for k, _ in ROUTE_OUTS]))
            A.check({k: want[k] for k in outs})


# ---- the path operators: trajectory, fixed-rate samples, curvature, speed plan -------------------------------------------------------------
PATH_LENS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000)      # empty, one point, one step; both sides of the 64-lane and 256-thread edges; two tiles
DT = 0.5


@pytest.fixture(scope='module')
def paths():
    """the ragged batch generator of tests/test_gpu_properties.py at the lengths above, with flag words as tests/test_gpu_trajectory.py makes
    them (some points of kind REVERSE)"""
    off = np.concatenate([[0], np.cumsum(PATH_LENS)]).astype(np.int64)
    xy, v = ragged_paths(PATH_LENS, 77, 0.4, 12)
    kinds = np.random.default_rng(78).choice([L.KIND_SWATH, L.KIND_UTURN, L.KIND_REVERSE], size=len(v))
    return off, np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1]), v, _fsw(kinds)


def _path_inputs(A, paths, extra=()):
    off, x, y, v, fs = paths
    A.input('off', off).input('x', x).input('y', y).input('v', v).input('fs', fs)
    for name, a in extra:
        A.input(name, a)
    return len(off) - 1, len(x)


def test_trajectory(gpu, paths):
    off, x, y, v, fs = paths
    s, t, h, totals = (_np(a) for a in E.trajectory(x, y, v, flagseg=fs, offsets=off))
    want = {'s': s, 't': t, 'heading': h, 'totals': totals.reshape(-1)}
    names = ('s', 't', 'heading', 'totals')
    for outs in (names, ('totals',), ('s',), ('heading',)):
        A = Arena()
        n_paths, n = _path_inputs(A, paths)
        for k in outs:
            A.output(k, np.float64, 2 * n_paths if k == 'totals' else n)
        A.build(gpu.dev)
        # (the subsets have the library read the offsets back from the arena)
        gpu.ok(gpu.lib.fcpp_trajectory(gpu.h, n_paths, A.ptr('off'), n, A.ptr('x'), A.ptr('y'), A.ptr('v'), A.ptr('fs'), *[A.ptr(k) for k in names],
                                       E._host_ptr(off if outs == names else None)))
        A.check({k: want[k] for k in outs})


def test_trajectory_counts_and_sample(gpu, paths):
    off, x, y, v, fs = paths
    traj = E.trajectory(x, y, v, flagseg=fs, offsets=off)
    smp = E.trajectory_sample(x, y, v, DT, flagseg=fs, offsets=off, include_end=True, traj=traj)
    s, t, h, totals = (_np(a) for a in traj)
    oo = np.ascontiguousarray(smp['out_offsets_host'], dtype=np.int64)
    k = int(oo[-1])
    n_paths = len(off) - 1
    assert k > 1000 and (np.diff(oo) >= 1).all()
    for with_host in (True, False):
        A = Arena().input('totals', totals).output('out_offsets', np.int64, n_paths + 1).build(gpu.dev)
        oh = np.full(n_paths + 1, -7, dtype=np.int64)
        gpu.ok(gpu.lib.fcpp_trajectory_counts(gpu.h, n_paths, A.ptr('totals'), DT, 1, A.ptr('out_offsets'), E._host_ptr(oh if with_host else None)))
        A.check({'out_offsets': oo})
        assert np.array_equal(oh, oo) if with_host else (oh == -7).all()
    outs_all = (('xs', 'x', np.float64), ('ys', 'y', np.float64), ('vs', 'v', np.float64), ('ss', 's', np.float64), ('hs', 'heading', np.float64),
                ('flagseg_s', 'flagseg', np.uint32), ('src_index', 'src_index', np.int64))
    want = {name: _np(smp[key]).view(dt) for name, key, dt in outs_all}
    assert (want['src_index'] == -1).sum() == 1 and np.isnan(want['xs']).sum() == 1          # the empty path's one sample
    for outs in (tuple(n for n, _, _ in outs_all), ('flagseg_s',), ('xs',)):
        A = Arena()
        _, n = _path_inputs(A, paths, (('s', s), ('t', t), ('heading', h), ('out_offsets', oo)))
        for name, _, dt in outs_all:
            if name in outs:
                A.output(name, dt, k)
        A.build(gpu.dev)
        full = len(outs) > 1
        gpu.ok(gpu.lib.fcpp_trajectory_sample(gpu.h, n_paths, A.ptr('off'), n, A.ptr('x'), A.ptr('y'), A.ptr('v'), A.ptr('s'), A.ptr('t'), A.ptr('heading'),
                                              A.ptr('fs'), DT, 1, A.ptr('out_offsets'), k, *[A.ptr(name) for name, _, _ in outs_all],
                                              E._host_ptr(off if full else None), E._host_ptr(oo if full else None)))
        A.check({name: want[name] for name in outs})


def test_curvature(gpu, paths):
    """(one output: there is no NULL subset to call)"""
    off, x, y, v, fs = paths
    kap = _np(E.curvature(x, y, offsets=off))
    for with_host in (True, False):
        A = Arena().input('off', off).input('x', x).input('y', y).output('kappa', np.float64, len(x)).build(gpu.dev)
        gpu.ok(gpu.lib.fcpp_curvature(gpu.h, len(off) - 1, A.ptr('off'), len(x), A.ptr('x'), A.ptr('y'), A.ptr('kappa'), E._host_ptr(off if with_host else None)))
        A.check({'kappa': kap})


@pytest.mark.parametrize('clamp', [1, 0])
def test_speed_plan(gpu, paths, clamp):
    off, x, y, v, fs = paths
    veh = E.make_vehicle()
    out, nadj, kap = (_np(a) for a in E.speed_plan(x, y, v, veh, clamp=bool(clamp), offsets=off, want_kappa=True))
    want = {'v_out': out, 'kappa': kap, 'n_adjusted': nadj}
    assert clamp == 0 or nadj.sum() > 0
    for outs in (('v_out', 'kappa', 'n_adjusted'), ('v_out',), ('v_out', 'n_adjusted')):
        A = Arena().input('off', off).input('x', x).input('y', y).input('v', v)
        for k in outs:
            A.output(k, np.int64 if k == 'n_adjusted' else np.float64, len(off) - 1 if k == 'n_adjusted' else len(x))
        A.build(gpu.dev)
        gpu.ok(gpu.lib.fcpp_speed_plan(gpu.h, C.byref(veh), clamp, len(off) - 1, A.ptr('off'), len(x), A.ptr('x'), A.ptr('y'), A.ptr('v'), A.ptr('v_out'),
                                       A.ptr('kappa'), A.ptr('n_adjusted'), E._host_ptr(off if len(outs) == 3 else None)))
        A.check({k: want[k] for k in outs})
