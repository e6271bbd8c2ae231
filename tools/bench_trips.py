"""Times the service trips' entry (HIP events around each CALL of fcpp_trip_solve, --reps repetitions after --warmup; median, minimum and
maximum), in the manner of tools/bench_cell_tour.py:
  (a) the fields of tools/bench_route.py -- --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m), cut at W = --width,
      each at its best angle of --angles -- routed with route_swaths(starts=--starts) from and to the service pose, which stands at the
      lower left corner of each field's bounding box, heading east; the capacity is --share of each field's work (a fifth: five trips or so);
  (b) fcpp_trip_solve on route_swaths' chunks of at most 1 GiB of transit blocks, every candidate in both directions: the chunks' medians
      summed, fields/s, variants/s, the mean of extra / base, trips per field, the share of fields whose winner is not the router's own;
  (c) the same rule on the host, fcpp_debug_trip_solve (the library deals the fields to its host threads, FCPP_THREADS = --threads) on the
      first --host-fields fields, every value checked equal to the device's.
The transit blocks and the ways to and from the service pose are built outside the timed calls (tools/bench_route.py times them).  The
timed calls include the entry's own argument checks and its synchronisation; the kernel's own time is not separated from them, and what
the two sequential chains of a variant (P and base) cost within it is not measured.
Prints ONE JSON line and writes it to --out (default profiles/trips_bench.json).  Needs a GPU; bench.py's metric is not touched by this."""
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
    ap.add_argument('--angles', type=int, default=36)
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--starts', type=int, default=8)
    ap.add_argument('--share', type=float, default=0.2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--host-fields', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'trips_bench.json'))
    args = ap.parse_args()
    os.environ.setdefault('FCPP_THREADS', str(max(1, args.threads)))          # (read once, when the library first deals fields out)
    from field_coverage_path_planning_amd import _lib as L
    from field_coverage_path_planning_amd import engine as E
    from field_coverage_path_planning_amd import trips as TR
    from tools.bench_swaths import _timed, stars
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_trips needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, S, R = args.fields, args.starts, args.radius
    rec = {'tool': 'bench_trips', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': args.width, 'radius': R,
           'starts': S, 'variants_per_field': 2 * S, 'capacity_share': args.share, 'mode': 'dubins',
           'not_measured': ['the kernel\'s own time (the calls are timed, argument checks and synchronisation included)',
                            'the two sequential chains of a variant (P and base) within the kernel',
                            'the transit blocks and the ways to the service pose: built outside the timed calls']}
    polys = stars(np.random.default_rng(1), n, args.vertices)
    pf = E.polygon_fields(list(polys))
    angles = torch.as_tensor(np.linspace(0.0, np.pi, args.angles, endpoint=False), device=dev)
    best, _ = E.best_swath_angle(pf, angles, args.width)
    ss = E.polygon_swaths(pf, angles[best.clamp(min=0)].contiguous(), args.width)
    soff_h = np.ascontiguousarray(ss.offsets_host, dtype=np.int64)
    m = np.diff(soff_h)
    service = np.column_stack([polys[:, :, 0].min(axis=1), polys[:, :, 1].min(axis=1), np.zeros(n)])
    route = E.route_swaths(ss, R, entry=service, exit=service, starts=S)
    In = E._route_ends(ss, service, True, R, False, None)
    Out = E._route_ends(ss, service, False, R, False, None)
    work = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, E._owners(ss.offsets, int(soff_h[-1])), ss.length)
    Q = (work * args.share).clamp(min=1.0).contiguous()
    tours = route.tours.to(torch.int32)
    rec['swaths'] = {'total': int(soff_h[-1]), 'mean': float(m.mean()), 'max': int(m.max()), 'over_cap': int((m > L.ROUTE_MAX_SWATHS).sum())}
    tour, trip = (torch.empty(int(soff_h[-1]), dtype=torch.int32, device=dev) for _ in range(2))
    n_trips, overfull, winner, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    cost, base, extra = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
    costs = torch.empty((n, 2 * S), dtype=torch.float64, device=dev)
    nh = max(1, min(n, args.host_fields))
    times, host = [], None
    ctx.bind_stream()
    for lo, hi, ch, T in TR._transit_chunks(ctx, ss, R, False, None, 0.0, False):
        s0, mc = int(soff_h[lo]), ch.m
        part = lambda a: a[2 * s0:2 * (s0 + mc)]
        tr = tours[:, s0:s0 + mc].contiguous()

        def solve():
            L.check(lib.fcpp_trip_solve(ctx.handle, hi - lo, P(ch.soff), HP(ch.soff_h), mc, P(ch.toff), HP(ch.toff_h), int(ch.toff_h[-1]), P(T),
                                        P(ss.length[s0:s0 + mc]), P(part(In)), P(part(Out)), P(part(In)), P(part(Out)), S, P(tr), 1, P(Q[lo:hi]), None, 0.0,
                                        P(tour[s0:s0 + mc]), P(trip[s0:s0 + mc]), P(n_trips[lo:hi]), P(overfull[lo:hi]), P(winner[lo:hi]), P(status[lo:hi]),
                                        P(cost[lo:hi]), P(base[lo:hi]), P(extra[lo:hi]), P(costs[lo:hi])))
        times.append(_timed(torch, solve, args.reps, args.warmup))
        print('fields %d .. %d: solve %.2f ms' % (lo, hi, times[-1]['median_ms']), file=sys.stderr, flush=True)
        if lo == 0:          # the host twin's inputs: the first fields of the first chunk
            nh = min(nh, hi)
            s1, t1 = int(ch.soff_h[nh]), int(ch.toff_h[nh])
            cpu = lambda a: np.ascontiguousarray(a.cpu().numpy())
            host = dict(soff=np.ascontiguousarray(ch.soff_h[:nh + 1]), toff=np.ascontiguousarray(ch.toff_h[:nh + 1]), T=cpu(T[:t1]), length=cpu(ss.length[:s1]),
                        In=cpu(In[:2 * s1]), Out=cpu(Out[:2 * s1]), tours=cpu(tours[:, :s1]), Q=cpu(Q[:nh]), s1=s1, t1=t1)
    tt = {k: float(sum(t[k] for t in times)) for k in ('median_ms', 'min_ms', 'max_ms')}
    ok = (status == 0) & (base > 0) & torch.isfinite(base)
    rec.update(chunks=len(times), solve_time=tt, fields_per_s=n / (tt['median_ms'] * 1e-3), variants_per_s=2 * S * n / (tt['median_ms'] * 1e-3),
               status_nonzero=int((status != 0).sum().item()), mean_extra_over_base=float((extra[ok] / base[ok]).mean().item()),
               mean_trips_per_field=float(n_trips[status == 0].to(torch.float64).mean().item()), overfull_trips=int(overfull.sum().item()),
               winner_not_the_routers_share=float((winner[status == 0] != 2 * route.winner[status == 0]).to(torch.float64).mean().item()),
               winner_backwards_share=float(((winner[status == 0] & 1) == 1).to(torch.float64).mean().item()))
    # the host twin on the first nh fields, every value against the device's
    h = host
    s1 = h['s1']
    ho = dict(tour=np.zeros(s1, np.int32), trip=np.zeros(s1, np.int32), n_trips=np.zeros(nh, np.int32), overfull=np.zeros(nh, np.int32),
              winner=np.zeros(nh, np.int32), status=np.zeros(nh, np.int32), cost=np.zeros(nh), base=np.zeros(nh), extra=np.zeros(nh), costs=np.zeros(nh * 2 * S))
    p = lambda x: x.ctypes.data
    t0 = time.perf_counter()
    L.check(lib.fcpp_debug_trip_solve(nh, p(h['soff']), s1, p(h['toff']), h['t1'], p(h['T']), p(h['length']), p(h['In']), p(h['Out']), p(h['In']), p(h['Out']), S,
                                      p(h['tours']), 1, p(h['Q']), None, 0.0, *[p(v) for v in ho.values()]))
    dth = time.perf_counter() - t0
    got = dict(tour=tour[:s1], trip=trip[:s1], n_trips=n_trips[:nh], overfull=overfull[:nh], winner=winner[:nh], status=status[:nh], cost=cost[:nh],
               base=base[:nh], extra=extra[:nh], costs=costs[:nh].reshape(-1))
    same = all(ho[k].tobytes() == np.ascontiguousarray(got[k].cpu().numpy()).tobytes() for k in ho)
    rec['host_twin'] = {'threads': int(os.environ['FCPP_THREADS']), 'fields': nh, 'seconds': dth, 'fields_per_s': nh / dth, 'values_equal_device': bool(same)}
    rec['device_over_host_per_field'] = rec['fields_per_s'] / (nh / dth)
    out = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(out + '\n')
    print(out)


if __name__ == '__main__':
    main()
