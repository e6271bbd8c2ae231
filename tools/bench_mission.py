"""Times the mission paths (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum) on the batch of
tools/bench_cover_regions.py: --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) planned by plan_polygon_fields at
W = --width with --passes headland passes driven, all outside the timed windows; then fcpp_mission_solve, fcpp_mission_counts and
fcpp_mission_fill over (headland loops outermost first, field path), Dubins and Reeds-Shepp, each call on its own into buffers allocated
before; and the host twin (fcpp_debug_mission_paths) on the library's host threads (FCPP_THREADS, at most 16) on the FIRST --host-fields
fields, whose records and samples must equal the device's (asserted).  Prints ONE JSON line (and writes it to --out).  Needs a GPU;
bench.py's metric is not touched by this."""
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
from tools.bench_cover_regions import _event_ms                  # noqa: E402
from tools.bench_swaths import _stat, stars                      # noqa: E402


def one_mode(args, torch, ctx, dev, polys, reversing):
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    n, mode = args.fields, 1 if reversing else 0
    plan = E.plan_polygon_fields(E.polygon_fields(list(polys)), args.width, args.radius, args.spacing,
                                 np.linspace(0.0, np.pi, args.angles, endpoint=False), passes=args.passes, reversing=reversing, headland_paths=True)
    t = E._mission_table([plan.headland_paths, plan.paths], dev, n_fields=n)
    del plan
    n_items, ps, total_in = len(t.ipath_h), t.paths, int(t.starts[-1])
    stride = max(1, -(-(t.longest - 1) // args.stations))
    R = E._chord_radius(args.radius, args.spacing)
    n_slots = 2 * n_items + n
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    status, transit, skipped = torch.empty(n, dtype=i32, device=dev), torch.empty(n, dtype=f64, device=dev), torch.empty(n, dtype=i32, device=dev)
    station, slot_item = torch.full((n_items,), -1, dtype=i64, device=dev), torch.full((n_slots,), -1, dtype=i64, device=dev)
    slot_word, slot_seg = torch.full((n_slots,), -1, dtype=i32, device=dev), torch.full((n_slots, 5), float('nan'), dtype=f64, device=dev)
    slot_total = torch.empty(n_slots, dtype=f64, device=dev)
    head = (mode, n, P(t.ioff), HP(t.ioff_h), n_items, P(t.ipath), HP(t.ipath_h), P(t.iclosed), int(t.first[-1]), P(ps.offsets),
            HP(ps.offsets_host), total_in)
    rec = (P(status), P(station), P(slot_item), P(slot_word), P(slot_seg))
    ctx.bind_stream()

    def solve():
        L.check(lib.fcpp_mission_solve(ctx.handle, *head, P(ps.x), P(ps.y), P(ps.heading), P(ps.part), P(ps.gear), *([None] * 6), R, stride, P(status),
                                       P(transit), P(skipped), P(station), P(slot_item), P(slot_word), P(slot_seg), P(slot_total)))
    solve()
    off, off_h, slot_off = torch.empty(n + 1, dtype=i64, device=dev), np.zeros(n + 1, np.int64), torch.empty(n_slots + 1, dtype=i64, device=dev)

    def counts():
        L.check(lib.fcpp_mission_counts(ctx.handle, *head, *rec, args.spacing, P(off), HP(off_h), P(slot_off)))
    counts()
    total = int(off_h[-1])
    cols = [torch.empty(total, dtype=dt, device=dev) for dt in (f64, f64, f64, f64, torch.int8, torch.int8, i32, i64)]

    def fill():
        L.check(lib.fcpp_mission_fill(ctx.handle, *head, P(ps.x), P(ps.y), P(ps.heading), P(ps.kappa), P(ps.part), P(ps.gear), None, None, None, R,
                                      args.spacing, *rec, P(slot_off), total, *[P(c) for c in cols]))
    ms = {'solve': [], 'counts': [], 'fill': []}
    for r in range(args.warmup + args.reps):
        for name, fn in (('solve', solve), ('counts', counts), ('fill', fill)):
            v = _event_ms(torch, fn)
            if r >= args.warmup:
                ms[name].append(v)
    closed = t.iclosed != 0
    lens = torch.as_tensor(np.diff(ps.offsets_host), device=dev)[t.ipath]
    nodes = torch.where(closed, torch.clamp((lens - 2) // stride + 1, min=0), torch.ones_like(lens))
    # (an upper bound: the candidates of every loop; the solves of a transition are the product of the two layers' nodes)
    ioff_h = t.ioff_h
    nd = nodes.cpu().numpy()
    solves = int(sum(int((nd[a:b - 1] * nd[a + 1:b]).sum()) for a, b in zip(ioff_h[:-1], ioff_h[1:]) if b - a > 1))
    out = {'stride': stride, 'items': n_items, 'loops': int(closed.sum().item()), 'samples_in': total_in, 'samples_out': total,
           'failed_fields': int((status != 0).sum().item()), 'skipped_items': int(skipped.sum().item()), 'candidate_solves_at_most': solves,
           'transit_length_m': float(transit[status == 0].sum().item())}
    for name in ('solve', 'counts', 'fill'):
        out[name + '_call'] = _stat(ms[name])
    out['solves_per_s_at_most'] = solves / (out['solve_call']['median_ms'] * 1e-3)
    kf = min(args.host_fields, n)
    if kf > 0:
        hi = int(ioff_h[kf])
        c = lambda a: np.ascontiguousarray(a.cpu().numpy())
        hx, hy, hh, hk, hpart, hgear, hclosed = (c(a) for a in (ps.x, ps.y, ps.heading, ps.kappa, ps.part, ps.gear, t.iclosed))
        hioff, hipath = np.ascontiguousarray(ioff_h[:kf + 1]), np.ascontiguousarray(t.ipath_h[:hi])
        hs = 2 * hi + kf
        o = dict(status=np.zeros(kf, np.int32), transit=np.zeros(kf), skipped=np.zeros(kf, np.int32), station=np.full(hi, -1, np.int64),
                 slot_item=np.full(hs, -1, np.int64), slot_word=np.full(hs, -1, np.int32), slot_seg=np.full((hs, 5), np.nan), slot_total=np.zeros(hs),
                 off=np.zeros(kf + 1, np.int64), slot_off=np.zeros(hs + 1, np.int64))
        hp = lambda a: None if a is None else a.ctypes.data
        hhead = (mode, kf, hp(hioff), hi, hp(hipath), hp(hclosed), int(t.first[-1]), hp(ps.offsets_host), total_in, hp(hx), hp(hy), hp(hh), hp(hk),
                 hp(hpart), hp(hgear), *([None] * 6), R, stride, args.spacing, *[hp(o[k]) for k in ('status', 'transit', 'skipped', 'station', 'slot_item',
                                                                                                   'slot_word', 'slot_seg', 'slot_total', 'off', 'slot_off')])
        assert lib.fcpp_debug_mission_paths(*hhead, 0, *([None] * 8)) == 0, lib.fcpp_last_error()
        ht = int(o['off'][-1])
        hcols = [np.zeros(ht, dt) for dt in (np.float64, np.float64, np.float64, np.float64, np.int8, np.int8, np.int32, np.int64)]
        t0 = time.perf_counter()
        assert lib.fcpp_debug_mission_paths(*hhead, ht, *[hp(a) for a in hcols]) == 0, lib.fcpp_last_error()
        t1 = time.perf_counter()
        assert np.array_equal(o['off'], off_h[:kf + 1]) and np.array_equal(o['status'], c(status[:kf])), 'offsets or status differ from the host twin'
        assert np.array_equal(o['station'], c(station[:hi])) and np.array_equal(o['transit'].view(np.int64), c(transit[:kf]).view(np.int64)), 'stations'
        for got, want in zip(cols, hcols):
            assert np.array_equal(c(got[:ht]).view(np.uint8), want.view(np.uint8)), 'samples differ from the host twin'
        dev_ms = sum(out[name + '_call']['median_ms'] for name in ('solve', 'counts', 'fill'))
        out['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'fields': kf, 'ms': (t1 - t0) * 1e3,
                            'ms_per_field': (t1 - t0) * 1e3 / kf, 'device_ms_per_field_three_calls': dev_ms / n,
                            'ratio_per_field': (t1 - t0) * 1e3 / kf / (dev_ms / n), 'equal': True,
                            'note': 'the twin ran on the first %d fields only; the ratio compares time per field, nothing is extrapolated' % kf}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=1024)
    ap.add_argument('--vertices', type=int, default=32)
    ap.add_argument('--angles', type=int, default=36)
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--spacing', type=float, default=0.5)
    ap.add_argument('--stations', type=int, default=128, help='the stride gives the longest loop at most this many stations')
    ap.add_argument('--host-fields', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mission needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    dev = torch.device('cuda', ctx.device)
    polys = stars(np.random.default_rng(1), args.fields, args.vertices)
    out = {'tool': 'bench_mission', 'reps': args.reps, 'warmup': args.warmup, 'fields': args.fields, 'vertices': args.vertices, 'width': args.width,
           'passes': args.passes, 'radius': args.radius, 'spacing': args.spacing, 'kernel_times': 'not measured (no trace in this run)'}
    for name, reversing in (('dubins', False), ('reeds_shepp', True)):
        out[name] = one_mode(args, torch, ctx, dev, polys, reversing)
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
