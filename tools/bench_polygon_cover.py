"""Times the polygon coverage report (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum):
  (a) tools/bench_field_paths.py's batch: --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) planned by
      plan_polygon_fields at W = --width with the headland loops driven (Dubins; --reversing: Reeds-Shepp), all outside the timed
      windows; then fcpp_polygon_cover_sizes and fcpp_polygon_cover at --res, each on its own into buffers allocated before, counts only
      (the cells of 4096 such fields are gigabytes); and the host twin (fcpp_debug_polygon_cover) on the library's host threads
      (FCPP_THREADS, at most 16) on the FIRST --host-fields fields, once, its counts compared with the device's;
  (b) --rect-fields rectangles of 500 x 200 m under one boustrophedon polyline each (swaths W apart, a sample every --rect-spacing m),
      caps = 1, at --rect-res: fcpp_polygon_cover and fcpp_cover_grid (one job per field, the same cells: ox = gx, shift 0.5, region 0,
      strict) ALTERNATING within the same run, the spread between the repeats of each, and whether covered + spill equals cover_grid's
      covered count in every field.
Prints ONE JSON line (and writes it to --out).  Needs a GPU; bench.py's metric is not touched by this."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from field_coverage_path_planning_amd import _lib as L          # noqa: E402
from field_coverage_path_planning_amd import engine as E        # noqa: E402
from tools.bench_swaths import _stat, _timed, stars              # noqa: E402


def _event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _boustrophedon(w, h, W, spacing):
    ys = np.arange(W / 2, h, W)
    m = int(round(w / spacing)) + 1
    xs = np.linspace(0.0, w, m)
    rows = [np.column_stack([xs if k % 2 == 0 else xs[::-1], np.full(m, y)]) for k, y in enumerate(ys)]
    return np.concatenate(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=4096)
    ap.add_argument('--vertices', type=int, default=32)
    ap.add_argument('--angles', type=int, default=36)
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--res', type=float, default=0.25)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--spacing', type=float, default=0.5)
    ap.add_argument('--reversing', action='store_true')
    ap.add_argument('--host-fields', type=int, default=64)
    ap.add_argument('--rect-fields', type=int, default=4096)
    ap.add_argument('--rect-res', type=float, default=0.5)
    ap.add_argument('--rect-spacing', type=float, default=2.0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_polygon_cover needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, Wd, res, rev = args.fields, args.width, args.res, bool(args.reversing)
    rec = {'tool': 'bench_polygon_cover', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': Wd, 'res': res,
           'radius': args.radius, 'spacing': args.spacing, 'mode': 'reeds_shepp' if rev else 'dubins'}

    # ---- (a) the planned star batch ----
    if n > 0:
        polys = stars(np.random.default_rng(1), n, args.vertices)
        pf = E.polygon_fields(list(polys))
        plan = E.plan_polygon_fields(pf, Wd, args.radius, args.spacing, np.linspace(0.0, np.pi, args.angles, endpoint=False), reversing=rev,
                                     headland_paths=True)
        n_paths, total, poff, poff_h, x, y, work, pas, fpo, ids = E._cover_paths((plan.paths, plan.headland_paths), n, dev)
        dims = torch.empty((n, 4), dtype=torch.int64, device=dev)
        coff, coff_h = torch.empty(n + 1, dtype=torch.int64, device=dev), np.zeros(n + 1, dtype=np.int64)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty((n, 4), dtype=torch.int64, device=dev)
        head = (ctx.handle, *pf._head(), Wd, res)
        ctx.bind_stream()

        def sizes():
            L.check(lib.fcpp_polygon_cover_sizes(*head, P(dims), P(coff), HP(coff_h), P(status)))

        def cover():
            L.check(lib.fcpp_polygon_cover(*head, 0, n_paths, P(poff), HP(poff_h), total, P(x), P(y), P(work), P(pas), P(fpo), P(ids), P(coff), HP(coff_h),
                                           None, P(counts), P(status)))
        ts = _timed(torch, sizes, args.reps, args.warmup)
        tc = _timed(torch, cover, args.reps, args.warmup)
        cells = int(coff_h[-1])
        c = counts.cpu().numpy()
        nxny = dims[:, 2:].cpu().numpy()
        tiles = int((((nxny[:, 0] + 63) // 64) * ((nxny[:, 1] + 63) // 64)).sum())
        rec['batch'] = {'paths': n_paths, 'samples': total, 'working_samples': int(work.sum().item()), 'cells': cells, 'tiles': tiles,
                        'status_nonzero': int((status != 0).sum().item()), 'inside': int(c[:, 0].sum()), 'covered': int(c[:, 1].sum()),
                        'overlapped': int(c[:, 2].sum()), 'spill': int(c[:, 3].sum()), 'mean_rate': float(np.nanmean(c[:, 1] / np.maximum(c[:, 0], 1)))}
        rec['sizes_call'] = {'time': ts, 'fields_per_s': n / (ts['median_ms'] * 1e-3)}
        rec['cover_call'] = {'time': tc, 'cells_per_s': cells / (tc['median_ms'] * 1e-3), 'fields_per_s': n / (tc['median_ms'] * 1e-3)}
        rec['kernel_times'] = 'not measured (no trace in this run)'

        k = min(args.host_fields, n)
        if k > 0:
            ro, vo = pf.ring_offsets.cpu().numpy(), pf.vert_offsets.cpu().numpy()
            hx, hy = pf.x.cpu().numpy(), pf.y.cpu().numpy()
            nr, nv = int(ro[k]), int(vo[int(ro[k])])
            hfpo = np.ascontiguousarray(fpo.cpu().numpy()[:k + 1])
            arrs = [np.ascontiguousarray(t.cpu().numpy()) for t in (poff, x, y, work, pas, ids)]
            hp = lambda a: a.ctypes.data
            hcnt, hst = np.zeros((k, 4), np.int64), np.zeros(k, np.int32)
            rok, vok = np.ascontiguousarray(ro[:k + 1]), np.ascontiguousarray(vo[:nr + 1])
            t0 = time.perf_counter()
            rc = lib.fcpp_debug_polygon_cover(k, hp(rok), nr, hp(vok), nv, hp(hx), hp(hy), Wd, res, 0, n_paths, hp(arrs[0]), total, hp(arrs[1]), hp(arrs[2]),
                                              hp(arrs[3]), hp(arrs[4]), hp(hfpo), hp(arrs[5]), None, None, 0, None, hp(hcnt), hp(hst))
            t1 = time.perf_counter()
            assert rc == 0, lib.fcpp_last_error()
            per_field = (t1 - t0) * 1e3 / k
            rec['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'fields': k, 'ms': (t1 - t0) * 1e3,
                                'ms_per_field': per_field, 'device_counts_equal_host': bool(np.array_equal(hcnt, c[:k])),
                                'cover_call_ms_per_field': tc['median_ms'] / n, 'ratio_per_field': per_field / (tc['median_ms'] / n),
                                'note': 'the twin ran on the first %d fields only; the ratio compares time per field, nothing is extrapolated' % k}

    # ---- (b) rectangles: the new operator and fcpp_cover_grid over the same cells, alternating ----
    m = args.rect_fields
    if m > 0:
        rng = np.random.default_rng(2)
        org = rng.uniform(0.0, 5000.0, (m, 2))
        base = _boustrophedon(500.0, 200.0, Wd, args.rect_spacing)
        rect = np.asarray([(0.0, 0.0), (500.0, 0.0), (500.0, 200.0), (0.0, 200.0)])
        pf = E.polygon_fields([rect + o for o in org])
        pts = (base[None, :, :] + org[:, None, :]).reshape(-1, 2)
        px, py = (torch.as_tensor(np.ascontiguousarray(pts[:, k]), device=dev) for k in (0, 1))
        npt = len(base)
        poff_h = np.arange(m + 1, dtype=np.int64) * npt
        poff, fpo = torch.as_tensor(poff_h, device=dev), torch.arange(m + 1, dtype=torch.int64, device=dev)
        dims = torch.empty((m, 4), dtype=torch.int64, device=dev)
        coff, coff_h = torch.empty(m + 1, dtype=torch.int64, device=dev), np.zeros(m + 1, dtype=np.int64)
        status = torch.empty(m, dtype=torch.int32, device=dev)
        counts = torch.empty((m, 4), dtype=torch.int64, device=dev)
        head = (ctx.handle, *pf._head(), Wd, args.rect_res)
        ctx.bind_stream()
        L.check(lib.fcpp_polygon_cover_sizes(*head, P(dims), P(coff), HP(coff_h), P(status)))
        dh = dims.cpu().numpy()
        g = dh[:, :2].copy().view(np.float64)
        jobs = [E.make_cover_job(g[i, 0], g[i, 1], args.rect_res, dh[i, 2], dh[i, 3], Wd / 2, npt, pts_first=i * npt, shift=0.5, strict=True)
                for i in range(m)]
        arr = (L.CoverJob * m)(*jobs)
        old = torch.zeros((m, 3), dtype=torch.int64, device=dev)

        def new_op():
            L.check(lib.fcpp_polygon_cover(*head, 1, m, P(poff), HP(poff_h), m * npt, P(px), P(py), None, None, P(fpo), None, P(coff), HP(coff_h), None,
                                           P(counts), P(status)))

        def old_op():
            L.check(lib.fcpp_cover_grid(ctx.handle, m, arr, m * npt, P(px), P(py), None, P(old)))
        t_new, t_old = [], []
        for r in range(args.warmup + args.reps):
            a, b = _event_ms(torch, new_op), _event_ms(torch, old_op)
            if r >= args.warmup:
                t_new.append(a)
                t_old.append(b)
        sn, so = _stat(t_new), _stat(t_old)
        c, o = counts.cpu().numpy(), old.cpu().numpy()
        spread = max((sn['max_ms'] - sn['min_ms']) / sn['median_ms'], (so['max_ms'] - so['min_ms']) / so['median_ms'])
        rec['rectangles'] = {'fields': m, 'res': args.rect_res, 'spacing': args.rect_spacing, 'samples_per_field': npt, 'cells': int(coff_h[-1]),
                             'polygon_cover': sn, 'cover_grid': so, 'ratio_new_over_old': sn['median_ms'] / so['median_ms'],
                             'spread_between_repeats': spread, 'new_no_slower_beyond_spread': bool(sn['median_ms'] <= so['median_ms'] * (1.0 + spread)),
                             'counts_equal': bool(np.array_equal(c[:, 1] + c[:, 3], o[:, 1])), 'covered_plus_spill': int((c[:, 1] + c[:, 3]).sum()),
                             'cover_grid_covered': int(o[:, 1].sum())}

    out = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(out + '\n')
    print(out)


if __name__ == '__main__':
    main()
