"""Times the cell tour's entries (HIP events around each CALL, --reps repetitions after --warmup; median, minimum and maximum), in the
manner of tools/bench_cells.py:
  (a) the fields of tools/bench_cells.py -- --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) with one diamond pond
      each -- cut along --angle into 'extrema' cells (about 75 000 at the defaults), every cell cut into swaths of width --width at the
      better of the track angles {0, pi / 2} and routed with route_swaths(starts=--starts): the router's candidates are the variants;
  (b) fcpp_cell_tour_transit and fcpp_cell_tour_solve on them in cell_tour's chunks of at most 1 GiB of joint blocks, Dubins and
      Reeds-Shepp: the chunks' medians summed, fields/s, joint entries/s, the mean of cost / stored cost over the fields with a finite stored cost;
  (c) the same rule on the host, fcpp_debug_cell_tour (transit and solve in one call; the library deals the fields to its host threads,
      FCPP_THREADS = --threads) on the first --host-fields fields, every value checked equal to the device's.
The timed calls include the entries' own argument checks and their synchronisation; the kernels' own times are not separated from them,
which step holds a call is not measured, and neither is what the caps cost (a field beyond one keeps its stored order).
Prints ONE JSON line and writes it to --out (default profiles/cell_tour_bench.json).  Needs a GPU; bench.py's metric is not touched by this."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=4096)
    ap.add_argument('--vertices', type=int, default=32)
    ap.add_argument('--angle', type=float, default=0.3)
    ap.add_argument('--width', type=float, default=4.0)
    ap.add_argument('--radius', type=float, default=6.0)
    ap.add_argument('--starts', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--host-fields', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'cell_tour_bench.json'))
    args = ap.parse_args()
    os.environ.setdefault('FCPP_THREADS', str(max(1, args.threads)))          # (read once, when the library first deals fields out)
    from field_coverage_path_planning_amd import _lib as L
    from field_coverage_path_planning_amd import cells as CL
    from field_coverage_path_planning_amd import engine as E
    from tools.bench_swaths import _timed
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_cell_tour needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, m, S = args.fields, args.vertices, args.starts
    rec = {'tool': 'bench_cell_tour', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': m, 'pond_vertices': 4, 'cut_angle': args.angle,
           'events': 'extrema', 'width': args.width, 'radius': args.radius, 'starts': S,
           'not_measured': ['the kernels\' own times (the calls are timed, argument checks and synchronisation included)',
                            'which step holds a call', 'what the caps cost: a field beyond one keeps its stored order']}
    rng = np.random.default_rng(1)
    a = np.sort(rng.uniform(0.0, 2.0 * np.pi, (n, m)), axis=1)
    rad = rng.uniform(40.0, 120.0, (n, m))
    centre = rng.uniform(0.0, 5000.0, (n, 2))
    polys = np.stack([rad * np.cos(a), rad * np.sin(a)], axis=2) + centre[:, None, :]
    rx, ry = rng.uniform(4.0, 12.0, n), rng.uniform(4.0, 12.0, n)
    fields = []
    for k in range(n):
        cx, cy = centre[k]
        fields.append([polys[k], np.array([(cx + rx[k], cy), (cx, cy + ry[k]), (cx - rx[k], cy), (cx, cy - ry[k])])])
    cells = CL.field_cells(fields, args.angle, 'extrema', args.width ** 2)
    cf = cells.fields
    ang = torch.tensor([0.0, np.pi / 2], dtype=torch.float64, device=dev)
    idx, _ = E.best_swath_angle(cf, ang, args.width, 10.0)
    ss = E.polygon_swaths(cf, ang[idx.clamp(min=0)], args.width)
    coff_h = np.ascontiguousarray(cells.cell_offsets_host, dtype=np.int64)
    rec.update(cells=int(coff_h[-1]), swaths=int(ss.offsets_host[-1]))
    nh = max(1, min(n, args.host_fields))
    max_sweeps = 8 * int(np.diff(coff_h).max(initial=0)) + 8
    for name, reversing in (('dubins', False), ('reeds_shepp', True)):
        mode = 1 if reversing else 0
        route = E.route_swaths(ss, args.radius, reversing=reversing, starts=S)
        voff_h, pin, pout, w, sn = CL._tour_variants(ss, route)
        cols = [p[:, k].contiguous() for p in (pin, pout) for k in range(3)]
        size = CL._tour_block_sizes(coff_h, voff_h)
        n_cells, n_vars = int(coff_h[-1]), int(voff_h[-1])
        order, node = (torch.empty(n_cells, dtype=torch.int32, device=dev) for _ in range(2))
        cost, stored, joint = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        winner, sweeps, skipped, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        ctx.bind_stream()
        t_transit, t_solve, chunks = [], [], CL._tour_chunks(size, CL.TOUR_D_BUDGET)
        for lo, hi in chunks:
            c0, c1 = int(coff_h[lo]), int(coff_h[hi])
            v0, v1 = int(voff_h[c0]), int(voff_h[c1])
            co_h, vo_h = np.ascontiguousarray(coff_h[lo:hi + 1] - c0), np.ascontiguousarray(voff_h[c0:c1 + 1] - v0)
            do_h = np.concatenate([[0], np.cumsum(size[lo:hi])]).astype(np.int64)
            co, vo, do = (torch.as_tensor(x, device=dev) for x in (co_h, vo_h, do_h))
            d_total = int(do_h[-1])
            D = torch.empty(d_total, dtype=torch.float64, device=dev)
            head = (hi - lo, P(co), HP(co_h), c1 - c0, P(vo), HP(vo_h), v1 - v0)
            pc = [c[v0:v1] for c in cols]

            def transit():
                L.check(lib.fcpp_cell_tour_transit(ctx.handle, *head, *[P(c) for c in pc], args.radius, mode, P(do), HP(do_h), d_total, P(D)))

            def solve():
                L.check(lib.fcpp_cell_tour_solve(ctx.handle, *head, P(w[v0:v1]), P(sn[c0:c1]), P(do), HP(do_h), d_total, P(D), None, None, S, 1e-9, max_sweeps,
                                                 P(order[c0:c1]), P(node[c0:c1]), P(cost[lo:hi]), P(stored[lo:hi]), P(joint[lo:hi]), P(winner[lo:hi]),
                                                 P(sweeps[lo:hi]), P(skipped[lo:hi]), P(status[lo:hi]), None, None))
            t_transit.append(_timed(torch, transit, args.reps, args.warmup))
            t_solve.append(_timed(torch, solve, args.reps, args.warmup))
            print('%s: fields %d .. %d, transit %.1f ms, solve %.1f ms' % (name, lo, hi, t_transit[-1]['median_ms'], t_solve[-1]['median_ms']),
                  file=sys.stderr, flush=True)
        total = lambda ts, key: float(sum(t[key] for t in ts))
        tt = {k: total(t_transit, k) for k in ('median_ms', 'min_ms', 'max_ms')}
        ts = {k: total(t_solve, k) for k in ('median_ms', 'min_ms', 'max_ms')}
        fine = torch.isfinite(stored) & (status == 0) & (stored > 0)
        r = {'variants': n_vars, 'joint_entries': int(size.sum()), 'chunks': len(chunks), 'transit_time': tt, 'solve_time': ts,
             'fields_per_s': n / ((tt['median_ms'] + ts['median_ms']) * 1e-3), 'joint_entries_per_s': float(size.sum()) / (tt['median_ms'] * 1e-3),
             'unsupported_fields': int((status == L.EUNSUPPORTED).sum().item()), 'invalid_fields': int((status == L.EINVAL).sum().item()),
             'mean_cost_over_stored': float((cost[fine] / stored[fine]).mean().item()) if bool(fine.any()) else None,
             'fields_strictly_better': int((cost[fine] < stored[fine]).sum().item()), 'mean_sweeps': float(sweeps.to(torch.float64).mean().item())}
        # the host twin on the first nh fields, every value against the device's
        c1, v1 = int(coff_h[nh]), int(voff_h[int(coff_h[nh])])
        hco, hvo = np.ascontiguousarray(coff_h[:nh + 1]), np.ascontiguousarray(voff_h[:c1 + 1])
        hdo = np.concatenate([[0], np.cumsum(size[:nh])]).astype(np.int64)
        hp = [np.ascontiguousarray(c[:v1].cpu().numpy()) for c in cols]
        hw, hsn = np.ascontiguousarray(w[:v1].cpu().numpy()), np.ascontiguousarray(sn[:c1].cpu().numpy())
        ho, hn = np.zeros(c1, np.int32), np.zeros(c1, np.int32)
        hc, hs, hj = np.zeros(nh), np.zeros(nh), np.zeros(nh)
        hwin, hsw, hsk, hst = (np.zeros(nh, np.int32) for _ in range(4))
        p = lambda x: x.ctypes.data
        t0 = time.perf_counter()
        L.check(lib.fcpp_debug_cell_tour(nh, p(hco), c1, p(hvo), v1, *[p(x) for x in hp], p(hw), p(hsn), args.radius, mode, p(hdo), int(hdo[-1]), None, None,
                                         None, S, 1e-9, max_sweeps, p(ho), p(hn), p(hc), p(hs), p(hj), p(hwin), p(hsw), p(hsk), p(hst), None, None))
        dth = time.perf_counter() - t0
        b = lambda x: np.ascontiguousarray(x).view(np.int64)
        same = (np.array_equal(ho, order[:c1].cpu().numpy()) and np.array_equal(hn, node[:c1].cpu().numpy())
                and np.array_equal(b(hc), b(cost[:nh].cpu().numpy())) and np.array_equal(b(hs), b(stored[:nh].cpu().numpy()))
                and np.array_equal(b(hj), b(joint[:nh].cpu().numpy())) and np.array_equal(hwin, winner[:nh].cpu().numpy())
                and np.array_equal(hsw, sweeps[:nh].cpu().numpy()) and np.array_equal(hsk, skipped[:nh].cpu().numpy())
                and np.array_equal(hst, status[:nh].cpu().numpy()))
        r['host_twin'] = {'threads': int(os.environ['FCPP_THREADS']), 'fields': nh, 'seconds': dth, 'fields_per_s': nh / dth, 'values_equal_device': bool(same)}
        r['device_over_host_per_field'] = r['fields_per_s'] / (nh / dth)
        rec[name] = r
    out = json.dumps(rec)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(out + '\n')
    print(out)


if __name__ == '__main__':
    main()
