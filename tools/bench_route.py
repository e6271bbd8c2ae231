"""Times the swath router (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum):
  (a) --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) cut at W = --width, each at its best angle of --angles;
  (b) fcpp_route_transit at R = --radius (Dubins; --reversing: Reeds-Shepp), in route_swaths' chunks of at most 1 GiB of blocks:
      entries/s (each canonical pair is solved once for two entries);
  (c) route_swaths, transit + fcpp_route_solve with --starts candidates per field: fields/s, the mean of cost / stored_cost over the
      fields with a stored cost above 0, the share of fields improved and the most moves a candidate applied;
  (d) the host twin (fcpp_debug_route_transit + fcpp_debug_route) on the library's host threads (FCPP_THREADS, at most 16) on the same
      batch, once, with the device results compared bit for bit.
  (e) --clear-of boundary --price-clear: the transit blocks against the fields' own boundaries, the penalty form (fcpp_route_transit +
      fcpp_route_transit_clear) and the priced form (fcpp_route_transit_priced) timed ALTERNATING within each repetition; the entries the
      priced form's first pass listed over the canonical pairs; and the mean connector length per field as driven with reshaping
      (clear_connectors on the legs) of the route on the penalty matrix and of the route on the priced one.
The timed calls include the entries' own argument checks and their synchronisation.  Prints ONE JSON line (and writes it to --out).
Needs a GPU; bench.py's metric is not touched by this."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=4096)
    ap.add_argument('--vertices', type=int, default=32)
    ap.add_argument('--angles', type=int, default=36)
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--starts', type=int, default=8)
    ap.add_argument('--reversing', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--clear-of', choices=['boundary'], default=None)
    ap.add_argument('--price-clear', action='store_true')
    ap.add_argument('--penalty', type=float, default=1.0e6)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.price_clear and args.clear_of is None:
        raise SystemExit('--price-clear needs --clear-of boundary')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_route needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, S, R, mode = args.fields, args.starts, args.radius, 1 if args.reversing else 0
    rec = {'tool': 'bench_route', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': args.width,
           'radius': R, 'starts': S, 'mode': 'reeds_shepp' if mode else 'dubins'}
    polys = stars(np.random.default_rng(1), n, args.vertices)
    pf = E.polygon_fields(list(polys))
    angles = torch.as_tensor(np.linspace(0.0, np.pi, args.angles, endpoint=False), device=dev)
    best, _ = E.best_swath_angle(pf, angles, args.width)
    ss = E.polygon_swaths(pf, angles[best.clamp(min=0)].contiguous(), args.width)
    soff_h = np.ascontiguousarray(ss.offsets_host, dtype=np.int64)
    m = np.diff(soff_h)
    toff_h = E._route_offsets(soff_h)
    nt, tt = int(soff_h[-1]), int(toff_h[-1])
    rec['swaths'] = {'total': nt, 'mean': float(m.mean()), 'max': int(m.max()), 'over_cap': int((m > L.ROUTE_MAX_SWATHS).sum()),
                     'transit_bytes': 8 * tt}
    chunks = E._route_chunks(soff_h, E.ROUTE_T_BUDGET)
    rec['chunks'] = len(chunks)
    ax, ay, bx, by = (t[:, k].contiguous() for t in (ss.a, ss.b) for k in (0, 1))
    max_sweeps = 8 * int(m[m <= L.ROUTE_MAX_SWATHS].max(initial=0)) + 8
    ctx.bind_stream()

    def transit():
        for lo, hi in chunks:
            E._route_transit(ctx, E._RouteChunk.of(ss, lo, hi), R, bool(mode))
    tr = _timed(torch, transit, args.reps, args.warmup)
    rec['transit'] = {'entries': tt, 'time': tr, 'entries_per_s': tt / (tr['median_ms'] * 1e-3)}
    box = {}

    def both():
        box['route'] = E.route_swaths(ss, R, reversing=bool(mode), starts=S, min_gain=1e-9, max_sweeps=max_sweeps)
    ts = _timed(torch, both, args.reps, args.warmup)
    route = box['route']
    c, s0, st = route.cost.cpu().numpy(), route.stored_cost.cpu().numpy(), route.status.cpu().numpy()
    ok = (st == 0) & (s0 > 0)
    rec['transit_plus_solve'] = {'time': ts, 'fields_per_s': n / (ts['median_ms'] * 1e-3), 'max_sweeps': max_sweeps,
                                 'most_moves': int(route.sweeps.max().item()), 'mean_cost_over_stored': float((c[ok] / s0[ok]).mean()),
                                 'improved_share': float((c[ok] < s0[ok] - 1e-9).mean()), 'status_nonzero': int((st != 0).sum())}
    rec['transit_plus_solve_ms'] = ts['median_ms']

    if args.clear_of is not None:
        import ctypes as C
        ro_h, vo_h = pf.ring_offsets.cpu().numpy(), pf.vert_offsets.cpu().numpy()
        parts = [E._fields_slice(pf, ro_h, vo_h, lo, hi) for lo, hi in chunks]
        listed = [0]

        def penalised():
            for (lo, hi), part in zip(chunks, parts):
                ch = E._RouteChunk.of(ss, lo, hi)
                E._route_transit_clear(ctx, ch, R, bool(mode), part, args.penalty, E._route_transit(ctx, ch, R, bool(mode)))

        def priced():
            listed[0] = 0
            for (lo, hi), part in zip(chunks, parts):
                E._route_transit_priced(ctx, E._RouteChunk.of(ss, lo, hi), R, bool(mode), part, args.penalty)
                got = C.c_int64(0)
                L.check(lib.fcpp_ctx_route_priced_passes(ctx.handle, C.byref(got), None))
                listed[0] += got.value

        def stamp(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        forms = (('penalty', penalised), ('priced', priced)) if args.price_clear else (('penalty', penalised),)
        ms = {k: [] for k, _ in forms}
        for k in range(args.warmup + args.reps):          # alternating: both forms see the same clocks and the same neighbours
            for name, fn in forms:
                t = stamp(fn)
                if k >= args.warmup:
                    ms[name].append(t)
        fit = m[m <= L.ROUTE_MAX_SWATHS]
        pairs = int((2 * fit * (fit - 1)).sum())          # canonical pairs of different swaths: (N^2 - 2 N) / 2, N = 2 m
        rec['clear_transit'] = {'penalty': args.penalty, 'canonical_pairs': pairs, 'penalty_form': _stat(ms['penalty'])}
        if args.price_clear:
            rec['clear_transit'].update(priced_form=_stat(ms['priced']), listed=listed[0], listed_share=listed[0] / max(pairs, 1))
            driven = {}
            for name, kw in (('penalty', {}), ('priced', {'price_clear': True})):
                r = E.route_swaths(ss, R, reversing=bool(mode), starts=S, min_gain=1e-9, max_sweeps=max_sweeps, clear_of=pf,
                                   blocked_penalty=args.penalty, **kw)
                frm, to, lf, _ = E._leg_pairs(ss, r.order, None, None)
                c = E.clear_connectors(frm, to, pf, lf, R, bool(mode))
                driven[name] = {'mean_driven_length_m': float(c.length.sum().item()) / n, 'blocked_legs': int((c.rank < 0).sum().item()),
                                'reshaped_legs': int((c.rank > 0).sum().item())}
            rec['clear_transit']['routes_driven_with_reshaping'] = driven

    if not args.no_host:
        hp = lambda a: a.ctypes.data
        hax, hay, hbx, hby, hang = (np.ascontiguousarray(t.cpu().numpy()) for t in (ax, ay, bx, by, ss.angle))
        hT = np.empty(tt)
        t0 = time.perf_counter()
        assert lib.fcpp_debug_route_transit(n, hp(soff_h), nt, hp(hax), hp(hay), hp(hbx), hp(hby), hp(hang), R, mode, hp(toff_h), tt, hp(hT)) == 0
        t1 = time.perf_counter()
        h_tours, h_costs = np.empty((S, nt), np.int32), np.empty((n, S))
        assert lib.fcpp_debug_route(n, hp(soff_h), nt, hp(toff_h), tt, hp(hT), None, None, S, 1e-9, max_sweeps, hp(h_tours), hp(h_costs), None, None, None,
                                    None, None, None) == 0
        t2 = time.perf_counter()
        same = bool(np.array_equal(h_tours, route.tours.cpu().numpy()) and np.array_equal(h_costs.view(np.int64), route.costs.cpu().numpy().view(np.int64)))
        rec['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'transit_ms': (t1 - t0) * 1e3,
                            'solve_ms': (t2 - t1) * 1e3, 'device_equals_host_bit_for_bit': same,
                            'speedup': ((t2 - t0) * 1e3) / rec['transit_plus_solve_ms']}

    out = json.dumps(rec)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(out + '\n')
    print(out)


if __name__ == '__main__':
    main()
