"""GPU tests of the trajectory output (run with -m gpu on an MI355X): fcpp_trajectory / fcpp_batch_trajectory (arc length, time stamp and
heading per point) and fcpp_trajectory_counts / fcpp_trajectory_sample (the trajectory at a fixed time step), against a numpy restatement
kept in this file and the reference's own totals in tests/golden/golden_kernels.npz (len_m, time_s of twelve paths with duplicates and
jumps, tools/gen_golden.py:98-150).

Tolerances -- derived, not measured.  All terms of the sums are >= 0, so any summation order of n terms lies within (n - 1) * 2^-53 * sum
of the exact sum to first order; library and checker each carry that: |a - b| <= n_path * 2^-52 * total_path.  Where the checker sums in
long double only the library's half is spent (n_path * 2^-53 * total_path).  Heading: 1e-12 rad after wrapping the difference into
(-pi, pi] (one atan2 of bit-equal arguments on both sides).  Points whose outgoing chord is non-zero but shorter than 1e-9 m may be left
out of the heading comparison, at most 0.5 % of the points of a run (asserted); exact duplicates take the carried direction and ARE
compared.  Coordinates of samples: 1e-9 m, the project's coordinate tolerance."""
import ctypes as C

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.support import np_of as _np
from tests.test_abi_and_host import _specs_from_golden
from tests.test_gpu_parity import DEFAULT_VP, _random_fields, _veh

pytestmark = pytest.mark.gpu

H_TOL = 1e-12
XY_TOL = 1e-9
TINY_CHORD = 1e-9
TINY_CAP = 0.005


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------
def _ref_path(x, y, v, fs=None, wide=False):
    """-> s, t, heading, tiny (points whose outgoing chord is non-zero but shorter than TINY_CHORD) of ONE path"""
    n = len(x)
    acc = np.longdouble if wide else np.float64
    s, t, h, tiny = np.zeros(n, acc), np.zeros(n, acc), np.zeros(n), np.zeros(n, bool)
    if n < 2:
        return s, t, h, tiny
    dx, dy = np.diff(x), np.diff(y)
    d = np.sqrt(dx * dx + dy * dy)
    ms = np.maximum(((v[:-1] + v[1:]) / 2) / 3.6, 0.1)
    s[1:] = np.cumsum(d.astype(acc))
    t[1:] = np.cumsum((d / ms).astype(acc))
    valid = (dx != 0) | (dy != 0)
    step = np.maximum.accumulate(np.where(valid, np.arange(n - 1), -1))     # nearest earlier non-zero step
    step = np.append(step, step[-1])                                       # the last point: its incoming step
    if valid.any():
        step[step < 0] = np.argmax(valid)                                  # leading zero steps: the first non-zero one that follows
        h = np.arctan2(dy[step], dx[step])
        if fs is not None:
            rev = (np.asarray(fs).view(np.uint32) & L.KIND_MASK) == L.KIND_REVERSE
            h = np.where(rev, np.where(h > 0, h - np.pi, h + np.pi), h)
        tiny[:-1] = valid & (d < TINY_CHORD)
    return s, t, h, tiny


def _ref(x, y, v, offsets, fs=None, wide=False):
    outs = [_ref_path(x[a:b], y[a:b], v[a:b], None if fs is None else fs[a:b], wide) for a, b in zip(offsets[:-1], offsets[1:])]
    return [np.concatenate([o[k] for o in outs]) if outs else np.zeros(0) for k in range(4)]


def _wrap(d):
    return np.abs((d + np.pi) % (2 * np.pi) - np.pi)


def _check(x, y, v, offsets, got, fs=None, wide=False, what=''):
    """s, t, heading, totals of the library against the restatement, path by path with the derived bound"""
    s, t, h, totals = (np.asarray(a) for a in got)
    rs, rt, rh, tiny = _ref(x, y, v, offsets, fs, wide)
    eps = 2.0 ** -53 if wide else 2.0 ** -52
    for p, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        n = b - a
        if n == 0:
            assert totals[p, 0] == 0 and totals[p, 1] == 0, (what, p)
            continue
        assert s[a] == 0 and t[a] == 0, (what, p)
        for lib, ref, tot in ((s, rs, totals[p, 0]), (t, rt, totals[p, 1])):
            bound = n * eps * float(ref[b - 1])
            err = np.abs(lib[a:b].astype(ref.dtype) - ref[a:b]).max()
            print(f'{what} path {p}: n {n} total {float(ref[b - 1]):.6g} err {float(err):.3e} bound {bound:.3e}')
            assert err <= bound, (what, p, float(err), bound)
            assert tot == lib[b - 1], (what, p)                   # the total IS the last running value
            assert (np.diff(lib[a:b]) >= 0).all(), (what, p)      # exactly non-decreasing: all terms are >= 0
    assert tiny.sum() <= TINY_CAP * max(len(x), 1), (what, int(tiny.sum()))
    keep = ~tiny
    herr = _wrap(h[keep] - rh[keep])
    print(f'{what} heading: left out {int(tiny.sum())} of {len(x)}, max err {herr.max() if herr.size else 0.0:.3e}')
    assert (herr <= H_TOL).all(), (what, float(herr.max()))
    assert ((h > -np.pi - 1e-15) & (h <= np.pi)).all()
    return tiny


def _golden_paths(g):
    off = g['sp_offsets'].astype(np.int64)
    xy = g['sp_path']
    return off, np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1]), np.ascontiguousarray(g['sp_v_out'])


# ---- 1-3: the reference's totals, the running values ------------------------------------------------------------------------------
def test_reference_totals(golden_kernels):
    """the twelve golden paths in ONE call: totals and the last s / t of every path equal the reference's len_m / time_s"""
    g = golden_kernels
    off, x, y, v = _golden_paths(g)
    s, t, h, totals = (_np(a) for a in E.trajectory(x, y, v, offsets=off))
    assert len(off) - 1 == 12 and totals.shape == (12, 2)
    for p in range(12):
        n, last = off[p + 1] - off[p], off[p + 1] - 1
        for got, ref in ((totals[p, 0], g['len_m'][p]), (totals[p, 1], g['time_s'][p]), (s[last], g['len_m'][p]), (t[last], g['time_s'][p])):
            print(f'path {p}: n {n} got {got!r} reference {ref!r} bound {n * 2.0 ** -52 * ref:.3e}')
            assert abs(got - ref) <= n * 2.0 ** -52 * ref, p


def test_running_values_and_heading_on_the_golden_paths(golden_kernels):
    off, x, y, v = _golden_paths(golden_kernels)
    got = [_np(a) for a in E.trajectory(x, y, v, offsets=off)]
    tiny = _check(x, y, v, off, got, what='golden')
    assert not tiny.any()       # steps of >= 0.004 m plus exact duplicates (tools/gen_golden.py:100-110): nothing is left out
    # a device-resident offsets tensor (the library reads it back) gives the same bits
    import torch
    again = E.trajectory(x, y, v, offsets=torch.as_tensor(off, device='cuda'))
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.int64), _np(b).view(np.int64))


# ---- 4: heading rules ----------------------------------------------------------------------------------------------------------------
def _fsw(kinds):
    return np.asarray(kinds, dtype=np.uint32) | np.uint32(37 << L.INDEX_SHIFT)


def test_heading_rules():
    rng = np.random.default_rng(7)
    paths, flags = [], []
    # 0: leading duplicates, then +x, +y
    paths.append(np.array([[1, 1], [1, 1], [1, 1], [2, 1], [2, 3]], float)); flags.append([0] * 5)
    # 1: a run of duplicates that straddles a tile boundary (points 510-515; tiles are 512 points; 1100 points = 3 tiles of 367, 367, 366,
    #    so a second run sits on the real boundary 366 | 367 as well)
    th = np.cumsum(rng.normal(0, 0.1, 1100))
    p1 = np.cumsum(np.column_stack([np.cos(th), np.sin(th)]) * 0.7, axis=0)
    p1[511:516] = p1[510]
    p1[365:370] = p1[364]
    paths.append(p1); flags.append([0] * 1100)
    # 2: exactly two tiles of 512: duplicates across 510-515 ARE across the tile boundary 511 | 512
    th = np.cumsum(rng.normal(0, 0.1, 1024))
    p2 = np.cumsum(np.column_stack([np.cos(th), np.sin(th)]) * 0.3, axis=0)
    p2[511:516] = p2[510]
    paths.append(p2); flags.append([0] * 1024)
    # 3: all duplicates; 4: one point; 5: no point
    paths.append(np.tile([[5.0, -2.0]], (700, 1))); flags.append([0] * 700)
    paths.append(np.array([[3.0, 4.0]])); flags.append([0])
    paths.append(np.zeros((0, 2))); flags.append([])
    # 6: a reverse stretch and the +-pi seam: +x, +x (reverse: pi), -x (pi), -x reversed (0), +y reversed (-pi/2), -y reversed (pi/2)
    paths.append(np.array([[0, 0], [1, 0], [2, 0], [1, 0], [0, 0], [0, 1], [0, 0], [0, 0]], float))
    flags.append([0, L.KIND_REVERSE, 0, L.KIND_REVERSE, L.KIND_REVERSE, L.KIND_REVERSE, 0, L.KIND_REVERSE])
    # 7: leading duplicates longer than a tile: the first non-zero step lies two tiles further on
    p7 = np.tile([[9.0, 9.0]], (1300, 1)); p7[1200:] += np.column_stack([np.arange(100.0), -np.arange(100.0)])
    paths.append(p7); flags.append([L.KIND_REVERSE] * 1300)
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
    xy = np.vstack(paths)
    x, y = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
    v = rng.choice([2.5, 4.0, 9.0, 15.0], size=len(x))
    fs = _fsw(np.concatenate([np.asarray(f, dtype=np.uint32) for f in flags]))
    got = [_np(a) for a in E.trajectory(x, y, v, flagseg=fs, offsets=off)]
    _check(x, y, v, off, got, fs=fs, what='rules')
    h = got[2]
    hp = [h[a:b] for a, b in zip(off[:-1], off[1:])]
    near = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-15
    assert near(hp[0], [0, 0, 0, np.pi / 2, np.pi / 2])                # leading duplicates take the first step's +x
    # points 510 .. 514 (364 .. 368) leave by a zero step: the direction of the step that arrived at the run; 515 (369) has its own again
    assert (hp[1][510:515] == hp[1][509]).all() and (hp[1][364:369] == hp[1][363]).all()
    assert hp[1][515] != hp[1][509] and hp[1][369] != hp[1][363]
    assert (hp[2][510:515] == hp[2][509]).all() and hp[2][515] != hp[2][509]
    assert (hp[3] == 0).all() and hp[4][0] == 0 and len(hp[5]) == 0
    assert near(hp[6], [0.0, np.pi, np.pi, 0.0, -np.pi / 2, np.pi / 2, -np.pi / 2, np.pi / 2])
    assert near(hp[7], np.full(1300, 3 * np.pi / 4))
    # without the flag words nothing is turned
    h0 = _np(E.trajectory(x, y, v, offsets=off)[2])
    assert near(h0[off[6]:off[7]], [0.0, 0.0, np.pi, np.pi, np.pi / 2, -np.pi / 2, -np.pi / 2, -np.pi / 2])
    for k in (0, 1):
        assert np.array_equal(got[k].view(np.int64), _np(E.trajectory(x, y, v, offsets=off)[k]).view(np.int64))


# ---- 5: batch consistency ------------------------------------------------------------------------------------------------------------
def _check_batch(batch, res, what):
    s, t, h, totals = (_np(a) for a in res.trajectory())
    st = res.stats()
    x, y, v, fs = _np(res.x), _np(res.y), _np(res.v), _np(res.flagseg).view(np.uint32)
    off = res.path_offsets()
    assert off[-1] == batch.total_points and totals.shape == (batch.n_fields, 4)
    n_fail = 0
    for i in range(batch.n_fields):
        info = batch.info[i]
        assert (off[2 * i], off[2 * i + 1], off[2 * i + 2]) == (info.point_offset, info.point_offset + info.n_main,
                                                              info.point_offset + info.n_main + info.n_head) or info.status != 0
        if info.status != 0:
            n_fail += 1
            assert off[2 * i] == off[2 * i + 2] and (totals[i] == 0).all()
            continue
        for col, name, n in ((0, 'main_len_m', info.n_main), (1, 'main_time_s', info.n_main), (2, 'head_len_m', info.n_head),
                             (3, 'head_time_s', info.n_head)):
            ref = st[name][i]
            assert abs(totals[i, col] - ref) <= n * 2.0 ** -52 * ref, (what, i, name, totals[i, col], ref)
    _check(x, y, v, off, (s, t, h, totals.reshape(-1, 2)), fs=fs, what=what)
    return n_fail


@pytest.mark.parametrize('turn_model,spacing', [(L.TURN_ARC, 0.0), (L.TURN_ARC, 0.5), (L.TURN_CLOTHOID, 0.0), (L.TURN_CLOTHOID, 0.5)])
def test_batch_trajectory_matches_the_batch_statistics(golden_plans, turn_model, spacing):
    g = golden_plans
    names = [str(n) for n in g['names'] if tuple(g[f'{n}/vp']) == tuple(g[f"{g['names'][0]}/vp"]) and int(g[f'{n}/ring_order']) == 0]
    specs = [_specs_from_golden(g, n) for n in names]
    opt = E.make_options(turn_model, spacing)
    batch = E.Batch(specs, _veh(g[f'{names[0]}/vp']), opt)
    _check_batch(batch, batch.run(), f'golden plans {turn_model}/{spacing}')
    batch.close()
    # 256 random rectangles, some of them too small for their headland: those fail and are empty paths with zero totals
    specs, _ = _random_fields(4711, 256)
    for k in (5, 77, 200):
        specs[k] = E.FieldSpec(field_length=20.0, field_width=12.0)
    batch = E.Batch(specs, _veh(DEFAULT_VP), opt)
    n_fail = _check_batch(batch, batch.run(), f'random 256 {turn_model}/{spacing}')
    assert n_fail >= 3
    batch.close()


# ---- 6: a long path (the three-level spine) and determinism ------------------------------------------------------------------------
def test_long_path_and_determinism():
    """one path of 3.2e7 points = 62 500 tiles = 245 blocks of the spine: against the long-double checker; the same path as the middle
    one of a three-path call and a second run of the same call: bit-identical"""
    import torch
    n = 32_000_000
    i = np.arange(n, dtype=np.float64)
    r, th = 50.0 + 1e-5 * i, 2e-4 * i
    x, y = r * np.cos(th), r * np.sin(th)
    dup = np.arange(1_000_003, n, 1_000_003)
    x[dup], y[dup] = x[dup - 1], y[dup - 1]
    x[16_000_000:] += 25.0                                   # a jump
    v = np.random.default_rng(3).choice([2.5, 4.0, 9.0, 14.0, 15.0], size=n)
    off = np.array([0, n], dtype=np.int64)
    xd, yd, vd = (torch.as_tensor(a, device='cuda') for a in (x, y, v))
    one = E.trajectory(xd, yd, vd, offsets=off)
    _check(x, y, v, off, [_np(a) for a in one], wide=True, what='long')
    two = E.trajectory(xd, yd, vd, offsets=off)
    for a, b in zip(one, two):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    del two
    # embedded: 777 points in front, 1500 behind
    pre, post = 777, 1500
    off3 = np.array([0, pre, pre + n, pre + n + post], dtype=np.int64)
    pad = lambda a, lo, hi: torch.cat((torch.as_tensor(lo, device='cuda'), a, torch.as_tensor(hi, device='cuda')))
    rng = np.random.default_rng(4)
    x3 = pad(xd, rng.uniform(0, 100, pre), rng.uniform(0, 100, post))
    y3 = pad(yd, rng.uniform(0, 100, pre), rng.uniform(0, 100, post))
    v3 = pad(vd, rng.uniform(2, 15, pre), rng.uniform(2, 15, post))
    del xd, yd, vd
    emb = E.trajectory(x3, y3, v3, offsets=off3)
    for a, b in zip(one[:3], emb[:3]):
        assert torch.equal(a.view(torch.int64), b[pre:pre + n].view(torch.int64))
    assert torch.equal(one[3][0].view(torch.int64), emb[3][1].view(torch.int64))


# ---- 7: fixed-rate samples -------------------------------------------------------------------------------------------------------------
def _check_samples(x, y, v, off, fs, dt, include_end, what):
    s, t, h, totals = E.trajectory(x, y, v, flagseg=fs, offsets=off)
    smp = E.trajectory_sample(x, y, v, dt, flagseg=fs, offsets=off, include_end=include_end, traj=(s, t, h, totals))
    s, t, h, totals = (_np(a) for a in (s, t, h, totals))
    oo = smp['out_offsets_host']
    assert np.array_equal(oo, _np(smp['out_offsets']))
    xs, ys, vs, ss, hs, fss, src = (_np(smp[k]) for k in ('x', 'y', 'v', 's', 'heading', 'flagseg', 'src_index'))
    assert len(xs) == oo[-1]
    for p, (a, b) in enumerate(zip(off[:-1], off[1:])):
        n, T = b - a, totals[p, 1]
        K = int(np.floor(T / dt)) + 1
        extra = bool(include_end and (K - 1) * dt < T)
        assert oo[p + 1] - oo[p] == K + extra, (what, p)
        sl = slice(oo[p], oo[p + 1])
        if n == 0:
            assert K == 1 and np.isnan(xs[sl]).all() and src[oo[p]] == -1
            continue
        tk = np.arange(K + extra, dtype=np.float64) * dt
        if include_end:
            tk[-1] = T
        i = np.searchsorted(t[a:b], tk, side='right') - 1
        assert np.array_equal(src[sl], a + i), (what, p)
        j = np.minimum(i + 1, n - 1)
        den = t[a + j] - t[a + i]
        lam = np.where(j > i, (tk - t[a + i]) / np.where(den > 0, den, 1.0), 0.0)
        assert ((lam >= 0) & (lam <= 1)).all()
        for got, arr, tol in ((xs, x, XY_TOL), (ys, y, XY_TOL), (ss, s, XY_TOL), (vs, v, 1e-9)):
            ref = arr[a + i] + lam * (arr[a + j] - arr[a + i])
            assert np.abs(got[sl] - ref).max() <= tol, (what, p)
        assert np.array_equal(hs[sl], h[a + i]) and (fs is None or np.array_equal(fss[sl].view(np.uint32), fs[a + i]))
        # on the chord of its step
        cx, cy = x[a + j] - x[a + i], y[a + j] - y[a + i]
        chord = np.hypot(cx, cy)
        cross = np.abs(cx * (ys[sl] - y[a + i]) - cy * (xs[sl] - x[a + i]))
        assert (cross <= XY_TOL * np.maximum(chord, 1e-300)).all(), (what, p)
        assert (np.diff(ss[sl]) >= 0).all()
        assert (xs[oo[p]], ys[oo[p]], ss[oo[p]]) == (x[a], y[a], 0.0)
        if include_end:
            k = oo[p + 1] - 1
            assert (xs[k], ys[k], ss[k], vs[k], src[k]) == (x[b - 1], y[b - 1], s[b - 1], v[b - 1], b - 1), (what, p)
        if T == 0:
            assert K + extra == 1


@pytest.mark.parametrize('dt', [0.1, 1.0, 7.3])
def test_fixed_rate_samples(golden_kernels, dt):
    off, x, y, v = _golden_paths(golden_kernels)
    # the golden paths, plus a path whose total time is 0 (all duplicates), a one-point path and an empty one
    extra = np.array([[4.0, 4.0]] * 6 + [[1.0, 2.0]])
    off = np.concatenate([off, off[-1] + np.array([6, 7, 7])])
    x, y, v = np.concatenate([x, extra[:, 0]]), np.concatenate([y, extra[:, 1]]), np.concatenate([v, np.full(7, 9.0)])
    for include_end in (True, False):
        _check_samples(x, y, v, off, None, dt, include_end, f'golden dt {dt} end {include_end}')
    # one planned field through the batch surface
    batch = E.Batch([E.FieldSpec(field_length=300.0, field_width=120.0, start_point=(10.0, 10.0))], _veh(DEFAULT_VP), E.make_options())
    res = batch.run()
    smp = res.sample(dt)
    po = res.path_offsets()
    fs = _np(res.flagseg).view(np.uint32)
    _check_samples(_np(res.x), _np(res.y), _np(res.v), po, fs, dt, True, f'field dt {dt}')
    ref = E.trajectory_sample(res.x, res.y, res.v, dt, flagseg=res.flagseg, offsets=po)
    for k in ('x', 'y', 'v', 's', 'heading', 'src_index', 'out_offsets'):
        assert np.array_equal(_np(smp[k]), _np(ref[k])), k
    batch.close()


def many_paths_lens(n_paths):
    """lengths from {0, 1, 2, 3 .. 40} for 257 or 513 paths with empty paths in a row across path 256: the count scan (one workgroup of
    256, a path per thread per round) carries its running offset into round two over paths that add one sample each.  257: the one path
    of round two is empty; 513: round three's one path has 40 points, behind three empty ones"""
    rng = np.random.default_rng(n_paths)
    lens = np.where(rng.random(n_paths) < 0.25, rng.integers(0, 3, n_paths), rng.integers(3, 41, n_paths))
    lens[253:259] = 0
    if n_paths == 513:
        lens[509:512], lens[512] = 0, 40
    return lens


def check_many_paths_lens(n_paths, lens):
    assert len(lens) == n_paths > 256 and {0, 1, 2} <= set(lens.tolist()) and lens.max() == 40 and lens.min() == 0
    assert (lens[253:min(259, n_paths)] == 0).all() and lens[252] > 0 and (lens[:253] >= 3).sum() > 150
    if n_paths == 513:
        assert lens[259] > 0 and (lens[259:509] >= 3).sum() > 150 and lens[509:513].tolist() == [0, 0, 0, 40]


@pytest.mark.parametrize('n_paths', [257, 513])
def test_fixed_rate_samples_of_more_paths_than_a_workgroup(n_paths):
    """fcpp_trajectory_counts' own instantiation of the shared scan (the paths' total times) in its second and third round of 256 paths,
    and the sampler's bisection of a sample's path over 257 / 513 offsets with runs of equal ones (the inputs' side is asserted without a
    device in tests/test_trajectory_abi.py)"""
    from tests.test_gpu_properties import ragged_paths
    lens = many_paths_lens(n_paths)
    check_many_paths_lens(n_paths, lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    xy, v = ragged_paths(lens, n_paths, 0.4, 6)
    x, y = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
    for include_end in (True, False):
        _check_samples(x, y, v, off, None, 0.1, include_end, f'{n_paths} paths end {include_end}')


# ---- 8: argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors(golden_kernels):
    import torch
    off, x, y, v = _golden_paths(golden_kernels)
    ctx = E.get_context()
    lib = ctx.lib
    dev = torch.device('cuda', ctx.device)
    xd, yd, vd = (torch.as_tensor(a, device=dev) for a in (x, y, v))
    od = torch.as_tensor(off, device=dev)
    n, m = len(x), len(off) - 1
    P, HP = E._ptr, E._host_ptr
    ctx.bind_stream()
    # NULL outputs are skipped: totals alone, then s alone
    totals = torch.zeros((m, 2), dtype=torch.float64, device=dev)
    assert lib.fcpp_trajectory(ctx.handle, m, P(od), n, P(xd), P(yd), P(vd), None, None, None, None, P(totals), HP(off)) == L.OK
    s = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    assert lib.fcpp_trajectory(ctx.handle, m, P(od), n, P(xd), P(yd), P(vd), None, P(s), None, None, None, None) == L.OK
    full = E.trajectory(x, y, v, offsets=off)
    assert torch.equal(s, full[0]) and torch.equal(totals, full[3])
    # missing inputs, inconsistent offsets: nothing is written
    s.fill_(-1.0)
    assert lib.fcpp_trajectory(ctx.handle, m, P(od), n, None, P(yd), P(vd), None, P(s), None, None, None, HP(off)) == L.EINVAL
    assert lib.fcpp_trajectory(ctx.handle, m, None, n, P(xd), P(yd), P(vd), None, P(s), None, None, None, None) == L.EINVAL
    bad = off.copy(); bad[3], bad[4] = off[4], off[3]
    assert lib.fcpp_trajectory(ctx.handle, m, P(od), n, P(xd), P(yd), P(vd), None, P(s), None, None, None, HP(bad)) == L.ESIZE
    assert lib.fcpp_trajectory(ctx.handle, m, P(od), n - 1, P(xd), P(yd), P(vd), None, P(s), None, None, None, HP(off)) == L.ESIZE
    assert lib.fcpp_trajectory(ctx.handle, -1, P(od), n, P(xd), P(yd), P(vd), None, P(s), None, None, None, HP(off)) == L.ESIZE
    assert (s == -1.0).all()
    # counts: dt <= 0, a time that is not finite, 2^31 samples
    oo = torch.full((m + 1,), -7, dtype=torch.int64, device=dev)
    for dt in (0.0, -1.0, float('nan')):
        assert lib.fcpp_trajectory_counts(ctx.handle, m, P(totals), dt, 1, P(oo), None) == L.EINVAL
    assert (oo == -7).all()
    assert lib.fcpp_trajectory_counts(ctx.handle, m, P(totals), 1e-12, 1, P(oo), None) == L.ESIZE
    t_bad = totals.clone(); t_bad[2, 1] = float('inf')
    assert lib.fcpp_trajectory_counts(ctx.handle, m, P(t_bad), 1.0, 1, P(oo), None) == L.ESIZE
    oh = np.zeros(m + 1, dtype=np.int64)
    assert lib.fcpp_trajectory_counts(ctx.handle, m, P(totals), 1.0, 0, P(oo), HP(oh)) == L.OK
    assert np.array_equal(oh, _np(oo)) and np.array_equal(np.diff(oh), np.floor(_np(totals)[:, 1] / 1.0).astype(np.int64) + 1)
    # sample: dt <= 0, out_offsets that do not span the samples
    k = int(oh[-1])
    xs = torch.full((k,), -1.0, dtype=torch.float64, device=dev)
    args = lambda dt, oo_h, tot: (ctx.handle, m, P(od), n, P(xd), P(yd), P(vd), P(full[0]), P(full[1]), P(full[2]), None, dt, 0, P(oo), tot,
                                  P(xs), None, None, None, None, None, None, HP(off), HP(oo_h))
    assert lib.fcpp_trajectory_sample(*args(0.0, oh, k)) == L.EINVAL
    assert lib.fcpp_trajectory_sample(*args(1.0, oh, k + 1)) == L.ESIZE
    assert lib.fcpp_trajectory_sample(*args(1.0, oh[::-1].copy(), k)) == L.ESIZE
    assert (xs == -1.0).all()
    assert lib.fcpp_trajectory_sample(*args(1.0, oh, k)) == L.OK and not (xs == -1.0).any()
    assert lib.fcpp_trajectory_sample(*args(1.0, None, k)) == L.OK       # (the library reads out_offsets back itself)
    with pytest.raises(L.FcppError):
        E.trajectory_sample(x, y, v, 0.0, offsets=off)


# ---- 9: the planner mirror -------------------------------------------------------------------------------------------------------------
def test_mirror_result_carries_the_trajectory():
    from field_coverage_path_planning_amd.multi_layer_planner_v3 import TwoLayerPathPlannerV37, VehicleParams
    pl = TwoLayerPathPlannerV37(VehicleParams(), field_length=500.0, field_width=200.0)
    res = pl.plan_complete_coverage()
    new = {'arc_length', 'time', 'heading'}
    # the reference's result (MLP:451-459) and layer dictionaries (MLP:619-628, 886-895) ...
    ref_top = {'main_work', 'headland', 'approach_path', 'departure_path', 'total_time', 'version', 'features'}
    ref_main, ref_head = {'path', 'speeds', 'pattern', 'area', 'stats'}, {'path', 'speeds', 'area', 'stats'}
    # ... plus the extras this mirror has always returned beside them (its module docstring): nothing else may have appeared
    extra_top, extra_layer = {'validation', 'num_passes', 'num_loops', 'start_corner_index'}, {'kappa', 'flagseg'}
    assert set(res) == ref_top | extra_top
    assert set(res['main_work']) - new == ref_main | extra_layer and new <= set(res['main_work'])
    assert set(res['headland']) - new == ref_head | extra_layer and new <= set(res['headland'])
    for layer in ('main_work', 'headland'):
        d = res[layer]
        n = len(d['path'])
        for k in new:
            assert isinstance(d[k], np.ndarray) and len(d[k]) == n, (layer, k)
        hours = d['stats']['time_hours']
        assert abs(d['time'][-1] / 3600 - hours) <= n * 2.0 ** -52 * hours, layer
        assert abs(d['arc_length'][-1] / 1000 - d['stats']['path_length_km']) <= n * 2.0 ** -52 * d['stats']['path_length_km'], layer
        assert d['arc_length'][0] == 0 and d['time'][0] == 0
    tr = pl.trajectory(0.1)
    for layer in ('main_work', 'headland'):
        d, q = res[layer], tr[layer]
        assert len(q['time']) == int(np.floor(d['time'][-1] / 0.1)) + 1 + ((np.floor(d['time'][-1] / 0.1)) * 0.1 < d['time'][-1])
        assert np.array_equal(q['path'][-1], d['path'][-1]) and np.array_equal(q['path'][0], d['path'][0])
        assert q['time'][-1] == d['time'][-1] and (np.diff(q['arc_length']) >= 0).all()
        assert np.array_equal(q['src_index'], np.searchsorted(d['time'], q['time'], side='right') - 1)
    pl.close()
