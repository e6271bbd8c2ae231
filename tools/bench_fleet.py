"""Times the vehicle shares' entry (HIP events around each CALL of fcpp_fleet_solve, --reps repetitions after --warmup; median, minimum and
maximum), in the manner of tools/bench_trips.py:
  (a) the fields of tools/bench_route.py -- --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m), cut at W = --width,
      each at its best angle of --angles -- routed with route_swaths(starts=--starts) from and to the depot, which stands at the lower
      left corner of each field's bounding box, heading east; --vehicles vehicles per field, a metre of work weighing --work-weight metres
      of driving;
  (b) fcpp_fleet_solve on route_swaths' chunks of at most 1 GiB of transit blocks, every candidate in both directions: the chunks' medians
      summed, fields/s, variants/s, the shares used per field, the mean of makespan(K) / makespan(1) -- the latter from a second, untimed
      call --, the share of fields whose winner is not the router's own;
  (c) the same rule on the host, fcpp_debug_fleet_solve (the library deals the fields to its host threads, FCPP_THREADS = --threads) on the
      first --host-fields fields, every value checked equal to the device's.
The transit blocks and the ways to and from the depot are built outside the timed calls (tools/bench_route.py times them).  The timed calls
include the entry's own argument checks and its synchronisation; the kernel's own time is not separated from them, and what the winner's
second solve and the two sequential chains of a variant (P and S) cost within it is not measured.
Prints ONE JSON line and writes it to --out (default profiles/fleet_bench.json).  Needs a GPU; bench.py's metric is not touched by this."""
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
    ap.add_argument('--vehicles', type=int, default=4)
    ap.add_argument('--work-weight', type=float, default=1.0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--host-fields', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'fleet_bench.json'))
    args = ap.parse_args()
    os.environ.setdefault('FCPP_THREADS', str(max(1, args.threads)))          # (read once, when the library first deals fields out)
    from field_coverage_path_planning_amd import _lib as L
    from field_coverage_path_planning_amd import engine as E
    from field_coverage_path_planning_amd import trips as TR
    from tools.bench_swaths import _timed, stars
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_fleet needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, S, R, K, omega = args.fields, args.starts, args.radius, args.vehicles, args.work_weight
    rec = {'tool': 'bench_fleet', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': args.width, 'radius': R,
           'starts': S, 'variants_per_field': 2 * S, 'vehicles': K, 'work_weight': omega, 'mode': 'dubins',
           'not_measured': ['the kernel\'s own time (the calls are timed, argument checks and synchronisation included)',
                            'the winner\'s second solve and the two sequential chains of a variant (P and S) within the kernel',
                            'the transit blocks and the ways to the depot: built outside the timed calls']}
    polys = stars(np.random.default_rng(1), n, args.vertices)
    pf = E.polygon_fields(list(polys))
    angles = torch.as_tensor(np.linspace(0.0, np.pi, args.angles, endpoint=False), device=dev)
    best, _ = E.best_swath_angle(pf, angles, args.width)
    ss = E.polygon_swaths(pf, angles[best.clamp(min=0)].contiguous(), args.width)
    soff_h = np.ascontiguousarray(ss.offsets_host, dtype=np.int64)
    m = np.diff(soff_h)
    depot = np.column_stack([polys[:, :, 0].min(axis=1), polys[:, :, 1].min(axis=1), np.zeros(n)])
    route = E.route_swaths(ss, R, entry=depot, exit=depot, starts=S)
    In = E._route_ends(ss, depot, True, R, False, None)
    Out = E._route_ends(ss, depot, False, R, False, None)
    tours = route.tours.to(torch.int32)
    Kf = torch.full((n,), K, dtype=torch.int32, device=dev)
    K1 = torch.ones(n, dtype=torch.int32, device=dev)
    rec['swaths'] = {'total': int(soff_h[-1]), 'mean': float(m.mean()), 'max': int(m.max()), 'over_cap': int((m > L.ROUTE_MAX_SWATHS).sum())}
    tour, share = (torch.empty(int(soff_h[-1]), dtype=torch.int32, device=dev) for _ in range(2))
    n_used, winner, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    makespan, total, alone = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
    makespans, totals = (torch.empty((n, 2 * S), dtype=torch.float64, device=dev) for _ in range(2))
    share_first = torch.empty((n, K), dtype=torch.int32, device=dev)
    share_cost = torch.empty((n, K), dtype=torch.float64, device=dev)
    nh = max(1, min(n, args.host_fields))
    times, host = [], None
    ctx.bind_stream()
    for lo, hi, ch, T in TR._transit_chunks(ctx, ss, R, False, None, 0.0, False):
        s0, mc = int(soff_h[lo]), ch.m
        part = lambda a: a[2 * s0:2 * (s0 + mc)]
        tr = tours[:, s0:s0 + mc].contiguous()
        head = lambda: (ctx.handle, hi - lo, P(ch.soff), HP(ch.soff_h), mc, P(ch.toff), HP(ch.toff_h), int(ch.toff_h[-1]), P(T), P(ss.length[s0:s0 + mc]),
                        P(part(In)), P(part(Out)), S, P(tr), 1)

        def solve():
            L.check(lib.fcpp_fleet_solve(*head(), P(Kf[lo:hi]), K, omega, P(tour[s0:s0 + mc]), P(share[s0:s0 + mc]), P(n_used[lo:hi]), P(winner[lo:hi]),
                                         P(status[lo:hi]), P(makespan[lo:hi]), P(total[lo:hi]), P(makespans[lo:hi]), P(totals[lo:hi]), P(share_first[lo:hi]),
                                         P(share_cost[lo:hi])))
        times.append(_timed(torch, solve, args.reps, args.warmup))
        print('fields %d .. %d: solve %.2f ms' % (lo, hi, times[-1]['median_ms']), file=sys.stderr, flush=True)
        L.check(lib.fcpp_fleet_solve(*head(), P(K1[lo:hi]), K, omega, None, None, None, None, None, P(alone[lo:hi]), None, None, None, None, None))
        if lo == 0:          # the host twin's inputs: the first fields of the first chunk
            nh = min(nh, hi)
            s1, t1 = int(ch.soff_h[nh]), int(ch.toff_h[nh])
            cpu = lambda a: np.ascontiguousarray(a.cpu().numpy())
            host = dict(soff=np.ascontiguousarray(ch.soff_h[:nh + 1]), toff=np.ascontiguousarray(ch.toff_h[:nh + 1]), T=cpu(T[:t1]), length=cpu(ss.length[:s1]),
                        In=cpu(In[:2 * s1]), Out=cpu(Out[:2 * s1]), tours=cpu(tours[:, :s1]), K=cpu(Kf[:nh]), s1=s1, t1=t1)
    tt = {k: float(sum(t[k] for t in times)) for k in ('median_ms', 'min_ms', 'max_ms')}
    ok = (status == 0) & (alone > 0) & torch.isfinite(alone)
    rec.update(chunks=len(times), solve_time=tt, fields_per_s=n / (tt['median_ms'] * 1e-3), variants_per_s=2 * S * n / (tt['median_ms'] * 1e-3),
               status_nonzero=int((status != 0).sum().item()), mean_shares_per_field=float(n_used[status == 0].to(torch.float64).mean().item()),
               mean_makespan_over_one_vehicle=float((makespan[ok] / alone[ok]).mean().item()),
               winner_not_the_routers_share=float((winner[status == 0] != 2 * route.winner[status == 0]).to(torch.float64).mean().item()),
               winner_backwards_share=float(((winner[status == 0] & 1) == 1).to(torch.float64).mean().item()))
    # the host twin on the first nh fields, every value against the device's
    h = host
    s1 = h['s1']
    ho = dict(tour=np.zeros(s1, np.int32), share=np.zeros(s1, np.int32), n_used=np.zeros(nh, np.int32), winner=np.zeros(nh, np.int32),
              status=np.zeros(nh, np.int32), makespan=np.zeros(nh), total=np.zeros(nh), makespans=np.zeros(nh * 2 * S), totals=np.zeros(nh * 2 * S),
              share_first=np.zeros(nh * K, np.int32), share_cost=np.zeros(nh * K))
    p = lambda x: x.ctypes.data
    t0 = time.perf_counter()
    L.check(lib.fcpp_debug_fleet_solve(nh, p(h['soff']), s1, p(h['toff']), h['t1'], p(h['T']), p(h['length']), p(h['In']), p(h['Out']), S, p(h['tours']), 1,
                                       p(h['K']), K, omega, *[p(v) for v in ho.values()]))
    dth = time.perf_counter() - t0
    got = dict(tour=tour[:s1], share=share[:s1], n_used=n_used[:nh], winner=winner[:nh], status=status[:nh], makespan=makespan[:nh], total=total[:nh],
               makespans=makespans[:nh].reshape(-1), totals=totals[:nh].reshape(-1), share_first=share_first[:nh].reshape(-1),
               share_cost=share_cost[:nh].reshape(-1))
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
