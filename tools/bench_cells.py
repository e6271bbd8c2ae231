"""Times the field cell entries (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum), in the manner
of tools/bench_inset.py:
  (a) fcpp_cells_counts and fcpp_cells_fill on --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) with one diamond
      pond each, cut angle --angle, min_area 0, in both modes: fields/s, cells/s, and ray-edge tests/s (every reflex vertex is tested against
      each of the field's E edges once to count and once to fill: the vertices x edges figure is an upper bound of that work);
  (b) the same rule on the host, fcpp_debug_cells (counts and fill in one call; the library deals the fields to its host threads,
      FCPP_THREADS = --threads) on the first --host-fields fields, its values checked equal to the device's.
The timed calls include the entries' own argument checks (the offsets and the angles are read back) and their synchronisation; the
kernels' own times are not separated from them, and the 1024-edge shape is not timed.
Prints ONE JSON line and writes it to --out (default profiles/cells_bench.json).  Needs a GPU; bench.py's metric is not touched by this."""
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--host-fields', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'cells_bench.json'))
    args = ap.parse_args()
    os.environ.setdefault('FCPP_THREADS', str(max(1, args.threads)))          # (read once, when the library first deals fields out)
    from field_coverage_path_planning_amd import _lib as L
    from field_coverage_path_planning_amd import engine as E
    from tools.bench_swaths import _timed
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_cells needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, m = args.fields, args.vertices
    rec = {'tool': 'bench_cells', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': m, 'pond_vertices': 4, 'cut_angle': args.angle,
           'min_area': 0.0, 'not_measured': ['the kernels\' own times (the calls are timed, argument checks and synchronisation included)',
                                             'the 1024-edge shape (four wavefronts a field)']}
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
    pf = E.polygon_fields(fields)
    ang = torch.full((n,), float(args.angle), dtype=torch.float64, device=dev)
    ctx.bind_stream()
    nh = max(1, min(n, args.host_fields))
    ro_h, vo_h = pf.ring_offsets.cpu().numpy(), pf.vert_offsets.cpu().numpy()
    x_h, y_h, ang_h = pf.x.cpu().numpy(), pf.y.cpu().numpy(), ang.cpu().numpy()
    for name, events in (('reflex', 0), ('extrema', 1)):
        co, cvo = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
        co_h, cvo_h = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        st, cuts, dropped = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        darea = torch.zeros(n, dtype=torch.float64, device=dev)
        head = (*pf._head(), P(ang), events, 0.0)

        def counts():
            L.check(lib.fcpp_cells_counts(ctx.handle, *head, P(co), HP(co_h), P(cvo), HP(cvo_h), P(st), P(cuts), P(dropped), P(darea)))
        tc = _timed(torch, counts, args.reps, args.warmup)
        C, V = int(co_h[-1]), int(cvo_h[-1])
        ovo = torch.empty(C + 1, dtype=torch.int64, device=dev)
        x, y = torch.empty(V, dtype=torch.float64, device=dev), torch.empty(V, dtype=torch.float64, device=dev)
        src, owner = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(C, dtype=torch.int32, device=dev)
        area = torch.empty(C, dtype=torch.float64, device=dev)

        def fill():
            L.check(lib.fcpp_cells_fill(ctx.handle, *head, P(co), P(cvo), C, V, P(ovo), P(x), P(y), P(src), P(owner), P(area)))
        tf = _timed(torch, fill, args.reps, args.warmup)
        total_ms = tc['median_ms'] + tf['median_ms']
        E_ = m + 4
        r = {'cells': C, 'cell_vertices': V, 'cuts': int(cuts.sum().item()), 'dropped': int(dropped.sum().item()), 'bad_fields': int((st != 0).sum().item()),
             'counts_time': tc, 'fill_time': tf, 'counts_plus_fill_ms': total_ms, 'fields_per_s': n / (total_ms * 1e-3), 'cells_per_s': C / (total_ms * 1e-3),
             'vertex_edge_tests_per_s_upper_bound': 2.0 * n * E_ * E_ / (total_ms * 1e-3)}
        # the host twin on the first nh fields: sizes, then the cells
        R, Vh = int(ro_h[nh]), int(vo_h[int(ro_h[nh])])
        hco, hcvo = np.zeros(nh + 1, np.int64), np.zeros(nh + 1, np.int64)
        hst, hcuts, hdrop, hdarea = np.zeros(nh, np.int32), np.zeros(nh, np.int32), np.zeros(nh, np.int32), np.zeros(nh)
        hhead = (nh, ro_h.ctypes.data, R, vo_h.ctypes.data, Vh, x_h.ctypes.data, y_h.ctypes.data, ang_h.ctypes.data, events, 0.0)
        t0 = time.perf_counter()
        L.check(lib.fcpp_debug_cells(*hhead, hco.ctypes.data, hcvo.ctypes.data, hst.ctypes.data, hcuts.ctypes.data, hdrop.ctypes.data, hdarea.ctypes.data,
                                     0, 0, None, None, None, None, None, None))
        hc, hv = int(hco[-1]), int(hcvo[-1])
        hovo, hx, hy = np.zeros(hc + 1, np.int64), np.zeros(hv), np.zeros(hv)
        hsrc, hown, harea = np.zeros(hv, np.int32), np.zeros(hc, np.int32), np.zeros(hc)
        L.check(lib.fcpp_debug_cells(*hhead, None, None, None, None, None, None, hc, hv, hovo.ctypes.data, hx.ctypes.data, hy.ctypes.data, hsrc.ctypes.data,
                                     hown.ctypes.data, harea.ctypes.data))
        dth = time.perf_counter() - t0
        same = (np.array_equal(hco, co_h[:nh + 1]) and np.array_equal(hovo, ovo[:hc + 1].cpu().numpy())
                and np.array_equal(hx.view(np.int64), x[:hv].cpu().numpy().view(np.int64)) and np.array_equal(hy.view(np.int64), y[:hv].cpu().numpy().view(np.int64))
                and np.array_equal(hsrc, src[:hv].cpu().numpy()) and np.array_equal(harea.view(np.int64), area[:hc].cpu().numpy().view(np.int64))
                and np.array_equal(hst, st[:nh].cpu().numpy()) and np.array_equal(hcuts, cuts[:nh].cpu().numpy()))
        r['host_twin'] = {'threads': int(os.environ['FCPP_THREADS']), 'fields': nh, 'seconds_two_calls': dth, 'fields_per_s': nh / (0.5 * dth),
                          'values_equal_device': bool(same)}
        r['device_over_host_per_field'] = (n / (total_ms * 1e-3)) / (nh / (0.5 * dth))
        rec[name] = r
    out = json.dumps(rec)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(out + '\n')
    print(out)


if __name__ == '__main__':
    main()
