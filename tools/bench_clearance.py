"""Times the connector clearance over every field's transit block (HIP events around each call, --reps repetitions after --warmup; median,
minimum and maximum), on bench_route's batch with a hole in every field:
  (a) --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m), each with an octagonal hole of 15 m around its centre,
      cut at W = --width, each at its best angle of --angles;
  (b) fcpp_route_transit alone at R = --radius (Dubins; --reversing: Reeds-Shepp), in route_swaths' chunks;
  (c) fcpp_route_transit_clear on the blocks of (b) against the fields themselves: canonical pairs/s and (piece, edge) tests/s -- an upper
      count, 3 or 5 pieces per pair, before the chunk boxes skip any;
  (d) the host twin (fcpp_debug_route_transit_clear) on the library's host threads (FCPP_THREADS, at most 16) on the same batch, once, with
      the device's T and B compared bit for bit: what the device time is measured against.
The timed calls include the entries' own argument checks, the read-back of the offsets and their synchronisation.  No ratio is fixed in
advance.  Prints ONE JSON line and writes it to --out (default profiles/clearance_bench.json).  Needs a GPU; bench.py's metric is not
touched by this."""
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
from tools.bench_swaths import _timed                            # noqa: E402


def holed_stars(rng, n, m, hole_radius=15.0, hole_vertices=8):
    """bench_swaths.stars' polygons (the same draws) with a regular polygon cut out around every centre -> list of [outer, hole]"""
    a = np.sort(rng.uniform(0.0, 2.0 * np.pi, (n, m)), axis=1)
    r = rng.uniform(40.0, 120.0, (n, m))
    c = rng.uniform(0.0, 5000.0, (n, 1, 2))
    outer = np.stack([r * np.cos(a), r * np.sin(a)], axis=2) + c
    t = 2.0 * np.pi * np.arange(hole_vertices) / hole_vertices
    hole = hole_radius * np.stack([np.cos(t), np.sin(t)], axis=1)[None] + c
    return [[outer[i], hole[i]] for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=4096)
    ap.add_argument('--vertices', type=int, default=32)
    ap.add_argument('--angles', type=int, default=36)
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--penalty', type=float, default=1.0e6)
    ap.add_argument('--reversing', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'clearance_bench.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_clearance needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib = ctx.lib
    dev = torch.device('cuda', ctx.device)
    n, R, mode = args.fields, args.radius, 1 if args.reversing else 0
    rec = {'tool': 'bench_clearance', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': args.width,
           'radius': R, 'penalty': args.penalty, 'mode': 'reeds_shepp' if mode else 'dubins'}
    pf = E.polygon_fields(holed_stars(np.random.default_rng(1), n, args.vertices))
    angles = torch.as_tensor(np.linspace(0.0, np.pi, args.angles, endpoint=False), device=dev)
    best, _ = E.best_swath_angle(pf, angles, args.width)
    ss = E.polygon_swaths(pf, angles[best.clamp(min=0)].contiguous(), args.width)
    soff_h = np.ascontiguousarray(ss.offsets_host, dtype=np.int64)
    m = np.diff(soff_h)
    toff_h = E._route_offsets(soff_h)
    nt, tt = int(soff_h[-1]), int(toff_h[-1])
    ro_h, vo_h = pf.ring_offsets.cpu().numpy(), pf.vert_offsets.cpu().numpy()
    edges = vo_h[ro_h[1:]] - vo_h[ro_h[:-1]]
    fits = m <= L.ROUTE_MAX_SWATHS
    pairs = int((2 * m[fits] * (m[fits] - 1)).sum())                 # canonical pairs of different swaths: half of (2 m)^2 - 4 m
    tests = int((2 * m[fits] * (m[fits] - 1) * edges[fits]).sum()) * (5 if mode else 3)
    rec['batch'] = {'swaths': nt, 'mean_swaths': float(m.mean()), 'max_swaths': int(m.max()), 'over_cap': int((~fits).sum()),
                    'mean_edges': float(edges.mean()), 'transit_entries': tt, 'canonical_pairs': pairs, 'piece_edge_tests_at_most': tests}
    chunks = E._route_chunks(soff_h, E.ROUTE_T_BUDGET)
    rec['chunks'] = len(chunks)
    ctx.bind_stream()

    def transit():
        for lo, hi in chunks:
            E._route_transit(ctx, E._RouteChunk.of(ss, lo, hi), R, bool(mode))
    tr = _timed(torch, transit, args.reps, args.warmup)
    rec['transit'] = {'time': tr, 'entries_per_s': tt / (tr['median_ms'] * 1e-3)}

    # the clearance alone: the blocks are made outside the timed region, every repetition penalises a fresh copy
    recs = [E._RouteChunk.of(ss, lo, hi) for lo, hi in chunks]
    made = [E._route_transit(ctx, ch, R, bool(mode)) for ch in recs]
    parts = [E._fields_slice(pf, ro_h, vo_h, lo, hi) for lo, hi in chunks]
    box = {}

    def clear():
        box['T'] = [T.clone() for T in made]
        box['B'] = [E._route_transit_clear(ctx, ch, R, bool(mode), part, args.penalty, T) for ch, part, T in zip(recs, parts, box['T'])]
    tc = _timed(torch, clear, args.reps, args.warmup)
    B = torch.cat(box['B']).cpu().numpy()
    T = torch.cat(box['T']).cpu().numpy()
    rec['transit_clear'] = {'time': tc, 'includes': 'a device copy of the blocks per repetition', 'pairs_per_s': pairs / (tc['median_ms'] * 1e-3),
                            'piece_edge_tests_per_s_at_most': tests / (tc['median_ms'] * 1e-3), 'blocked_share': float(B.mean()) if B.size else 0.0,
                            'over_transit': tc['median_ms'] / tr['median_ms']}

    if not args.no_host:
        hp = lambda a: a.ctypes.data
        ax, ay, bx, by = (np.ascontiguousarray(t[:, k].cpu().numpy()) for t in (ss.a, ss.b) for k in (0, 1))
        hang, hx, hy = (np.ascontiguousarray(t.cpu().numpy()) for t in (ss.angle, pf.x, pf.y))
        hT, hB = np.empty(tt), np.empty(tt, np.uint8)
        assert lib.fcpp_debug_route_transit(n, hp(soff_h), nt, hp(ax), hp(ay), hp(bx), hp(by), hp(hang), R, mode, hp(toff_h), tt, hp(hT)) == 0
        t0 = time.perf_counter()
        assert lib.fcpp_debug_route_transit_clear(n, hp(soff_h), nt, hp(ax), hp(ay), hp(bx), hp(by), hp(hang), R, mode, hp(toff_h), tt, hp(ro_h),
                                                  len(vo_h) - 1, hp(vo_h), len(hx), hp(hx), hp(hy), args.penalty, hp(hT), hp(hB)) == 0
        t1 = time.perf_counter()
        same = bool(np.array_equal(hB, B) and np.array_equal(hT.view(np.int64), T.view(np.int64)))
        rec['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'transit_clear_ms': (t1 - t0) * 1e3,
                            'device_equals_host_bit_for_bit': same, 'host_over_device': ((t1 - t0) * 1e3) / tc['median_ms']}

    out = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(out + '\n')
    print(out)


if __name__ == '__main__':
    main()
