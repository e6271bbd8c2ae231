"""Times the field paths (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum):
  (a) --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) cut at W = --width, each at its best angle of --angles and
      routed with --starts candidates (route_swaths at the spacing driven), all outside the timed windows;
  (b) field_paths at R = --radius and --spacing (Dubins; --reversing: Reeds-Shepp) in the routed order: the whole call (counts + fill,
      allocations of the outputs included), and fcpp_field_path_counts and fcpp_field_path_fill each on its own into buffers allocated
      before.  The fill CALL recomputes the leg records, reads the two ends of the slot offsets back and synchronises: its samples/s and
      its share of the 8 TB/s write stream at 38 B per sample are the call's, not the fill kernel's alone;
  (c) the host twin (fcpp_debug_field_paths, sizing call + filling call) on the library's host threads (FCPP_THREADS, at most 16) on the
      same batch, once, with the device results compared bit for bit;
  (d) the parent's way: swath_route(order=route) in a Python loop over the FIRST --loop-fields fields, host clock around the loop with a
      synchronise at its end, reported per field; the ratio to (b) is per field against per field and covers those fields only.
--clear-of: instead of (b) - (d), the counts and fill CALLS of the plain entries and of the clear entries (fcpp_field_path_counts_clear /
_fill_clear; regions: the star fields' own boundaries) on the same batch and order, ALTERNATING plain and clear within every repetition;
with the slots the first pass listed and the blocked / reshaped sums.  No ratio is fixed in advance: the plain entries are the comparator.
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
from tools.bench_swaths import _timed, stars                     # noqa: E402

BYTES_PER_SAMPLE = 4 * 8 + 1 + 1 + 4          # x, y, heading, kappa; part; gear; leg
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=4096)
    ap.add_argument('--vertices', type=int, default=32)
    ap.add_argument('--angles', type=int, default=36)
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--spacing', type=float, default=0.5)
    ap.add_argument('--starts', type=int, default=8)
    ap.add_argument('--reversing', action='store_true')
    ap.add_argument('--loop-fields', type=int, default=64)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--clear-of', action='store_true', help='time the clear entries beside the plain ones (regions: the fields themselves)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_field_paths needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, R, sp, rev = args.fields, args.radius, args.spacing, bool(args.reversing)
    rec = {'tool': 'bench_field_paths', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': args.width,
           'radius': R, 'spacing': sp, 'starts': args.starts, 'mode': 'reeds_shepp' if rev else 'dubins', 'bytes_per_sample': BYTES_PER_SAMPLE}
    polys = stars(np.random.default_rng(1), n, args.vertices)
    pf = E.polygon_fields(list(polys))
    angles = torch.as_tensor(np.linspace(0.0, np.pi, args.angles, endpoint=False), device=dev)
    best, _ = E.best_swath_angle(pf, angles, args.width)
    ss = E.polygon_swaths(pf, angles[best.clamp(min=0)].contiguous(), args.width)
    route = E.route_swaths(ss, R, reversing=rev, starts=args.starts, spacing=sp)
    soff_h = np.ascontiguousarray(ss.offsets_host, dtype=np.int64)
    m = np.diff(soff_h)
    nt = int(soff_h[-1])
    rec['swaths'] = {'total': nt, 'mean': float(m.mean()), 'max': int(m.max()), 'leg_slots': 2 * nt + n}

    if args.clear_of:
        rec['tool'] = 'bench_field_paths --clear-of'
        rec.update(clear_bench(torch, ctx, ss, route, pf, n, nt, soff_h, R, sp, rev, args.reps, args.warmup))
        return emit(rec, args.out)

    box = {}

    def whole():
        box['fp'] = E.field_paths(ss, R, sp, reversing=rev, order=route)
    tw = _timed(torch, whole, args.reps, args.warmup)
    fp = box['fp']
    total = int(fp.offsets_host[-1])
    part = fp.part.cpu().numpy()
    rec['samples'] = {'total': total, 'per_field': total / max(n, 1), 'connector_share': float((part != 0).mean()) if total else 0.0,
                      'status_nonzero': int((fp.status != 0).sum().item())}
    rec['field_paths'] = {'time': tw, 'samples_per_s': total / (tw['median_ms'] * 1e-3), 'fields_per_s': n / (tw['median_ms'] * 1e-3)}
    rec['field_paths_ms'] = tw['median_ms']

    # the two entries on their own, into buffers allocated before
    ax, ay, bx, by = (t[:, k].contiguous() for t in (ss.a, ss.b) for k in (0, 1))
    order = route.order.to(torch.int32).contiguous()
    head = (ctx.handle, n, P(ss.offsets), HP(soff_h), nt, P(ax), P(ay), P(bx), P(by), P(ss.length), P(ss.angle), P(order), E._chord_radius(R, sp),
            1 if rev else 0, sp, *([None] * 6))
    off, leg_off = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(2 * nt + n + 1, dtype=torch.int64, device=dev)
    off_h = np.zeros(n + 1, dtype=np.int64)
    work, transit = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    x, y, h, kap = (torch.empty(total, dtype=torch.float64, device=dev) for _ in range(4))
    prt, gear = torch.empty(total, dtype=torch.int8, device=dev), torch.empty(total, dtype=torch.int8, device=dev)
    leg = torch.empty(total, dtype=torch.int32, device=dev)
    ctx.bind_stream()

    def counts():
        L.check(lib.fcpp_field_path_counts(*head, P(off), HP(off_h), P(leg_off), P(work), P(transit), P(status)))

    def fill():
        L.check(lib.fcpp_field_path_fill(*head, P(leg_off), total, P(x), P(y), P(h), P(kap), P(prt), P(gear), P(leg)))
    tc = _timed(torch, counts, args.reps, args.warmup)
    tf = _timed(torch, fill, args.reps, args.warmup)
    assert int(off_h[-1]) == total and torch.equal(x, fp.x) and torch.equal(leg, fp.leg)
    rate = total / (tf['median_ms'] * 1e-3)
    rec['counts_call'] = {'time': tc, 'slots_per_s': (2 * nt + n) / (tc['median_ms'] * 1e-3)}
    rec['fill_call'] = {'time': tf, 'samples_per_s': rate, 'bytes_per_s': rate * BYTES_PER_SAMPLE,
                        'share_of_8TBps_write_stream': rate * BYTES_PER_SAMPLE / HBM_PEAK}

    if not args.no_host:
        hp = lambda a: None if a is None else a.ctypes.data
        hax, hay, hbx, hby, hlen, hang, hord = (np.ascontiguousarray(t.cpu().numpy()) for t in (ax, ay, bx, by, ss.length, ss.angle, order))
        hoff, hleg = np.zeros(n + 1, np.int64), np.zeros(2 * nt + n + 1, np.int64)
        hhead = (n, hp(soff_h), nt, hp(hax), hp(hay), hp(hbx), hp(hby), hp(hlen), hp(hang), hp(hord), E._chord_radius(R, sp), 1 if rev else 0, sp,
                 *([None] * 6), hp(hoff), hp(hleg), None, None, None, None, None, None)
        t0 = time.perf_counter()
        assert lib.fcpp_debug_field_paths(*hhead, 0, *([None] * 7)) == 0
        ht = int(hoff[-1])
        outs = [np.empty(ht, dt) for dt in (np.float64, np.float64, np.float64, np.float64, np.int8, np.int8, np.int32)]
        assert lib.fcpp_debug_field_paths(*hhead, ht, *[hp(a) for a in outs]) == 0
        t1 = time.perf_counter()
        same = bool(ht == total and np.array_equal(hleg, fp.leg_offsets.cpu().numpy())
                    and all(np.array_equal(a.view(np.uint8), getattr(fp, k).cpu().numpy().view(np.uint8))
                            for a, k in zip(outs, ('x', 'y', 'heading', 'kappa', 'part', 'gear', 'leg'))))
        rec['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'ms': (t1 - t0) * 1e3,
                            'device_equals_host_bit_for_bit': same, 'speedup': ((t1 - t0) * 1e3) / rec['field_paths_ms']}

    # the parent's way, on the first fields only
    k = min(args.loop_fields, n)
    if k > 0:
        E.swath_route(ss, 0, R, sp, reversing=rev, order=route)          # (warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = 0
        for i in range(k):
            got += int(E.swath_route(ss, i, R, sp, reversing=rev, order=route)[0].numel())
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        per_field = (t1 - t0) * 1e3 / k
        assert got == int(fp.offsets_host[k])
        rec['swath_route_loop'] = {'fields': k, 'samples': got, 'ms': (t1 - t0) * 1e3, 'ms_per_field': per_field,
                                   'field_paths_ms_per_field': rec['field_paths_ms'] / n,
                                   'ratio_per_field': per_field / (rec['field_paths_ms'] / n),
                                   'note': 'the loop ran on the first %d fields only; the ratio compares time per field, nothing is extrapolated' % k}

    emit(rec, args.out)


def emit(rec, path):
    out = json.dumps(rec)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(out + '\n')
    print(out)


def clear_bench(torch, ctx, ss, route, pf, n, nt, soff_h, R, sp, rev, reps, warmup):
    """the four calls, plain and clear alternating within every repetition, each between two HIP events -> the record's entries"""
    import ctypes as C
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = ss.a.device
    n_slots = 2 * nt + n
    ax, ay, bx, by = (t[:, k].contiguous() for t in (ss.a, ss.b) for k in (0, 1))
    order = route.order.to(torch.int32).contiguous()
    head = (ctx.handle, n, P(ss.offsets), HP(soff_h), nt, P(ax), P(ay), P(bx), P(by), P(ss.length), P(ss.angle), P(order), E._chord_radius(R, sp),
            1 if rev else 0, sp, *([None] * 6))
    region = pf._head()[1:]
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    bufs = {}
    for kind in ('plain', 'clear'):
        bufs[kind] = dict(off=torch.empty(n + 1, dtype=torch.int64, device=dev), leg_off=torch.empty(n_slots + 1, dtype=torch.int64, device=dev),
                          off_h=np.zeros(n + 1, dtype=np.int64), work=torch.empty(n, dtype=torch.float64, device=dev),
                          transit=torch.empty(n, dtype=torch.float64, device=dev), status=i32(n))
    extra = [i32(n_slots), i32(n_slots), i32(n_slots), torch.empty((n_slots, 5), dtype=torch.float64, device=dev),
             torch.empty(n_slots, dtype=torch.float64, device=dev), i32(n), i32(n), i32(n)]
    ctx.bind_stream()

    def counts(kind):
        b = bufs[kind]
        tail = (P(b['off']), HP(b['off_h']), P(b['leg_off']), P(b['work']), P(b['transit']), P(b['status']))
        if kind == 'plain':
            L.check(lib.fcpp_field_path_counts(*head, *tail))
        else:
            L.check(lib.fcpp_field_path_counts_clear(*head, *region, *tail, *[P(t) for t in extra]))

    def fill(kind):
        b = bufs[kind]
        tail = (P(b['leg_off']), b['total'], *[P(t) for t in b['samples']])
        if kind == 'plain':
            L.check(lib.fcpp_field_path_fill(*head, *tail))
        else:
            L.check(lib.fcpp_field_path_fill_clear(*head, *region, *tail))

    for kind in ('plain', 'clear'):
        counts(kind)
        b = bufs[kind]
        b['total'] = int(b['off_h'][-1])
        b['samples'] = [torch.empty(b['total'], dtype=dt, device=dev)
                        for dt in (torch.float64, torch.float64, torch.float64, torch.float64, torch.int8, torch.int8, torch.int32)]
    listed, launches = C.c_int64(0), C.c_int64(0)
    L.check(lib.fcpp_ctx_field_path_clear_passes(ctx.handle, C.byref(listed), C.byref(launches)))
    times = {(call, kind): [] for call in ('counts', 'fill') for kind in ('plain', 'clear')}
    for rep in range(warmup + reps):
        for call, fn in (('counts', counts), ('fill', fill)):
            for kind in ('plain', 'clear'):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(kind)
                e1.record()
                e1.synchronize()
                if rep >= warmup:
                    times[call, kind].append(e0.elapsed_time(e1))
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v)), 'max_ms': float(np.max(v))}
    out = {'%s_call_%s' % (call, kind): stat(v) for (call, kind), v in times.items()}
    out['samples'] = {kind: bufs[kind]['total'] for kind in bufs}
    out['clear'] = {'connector_slots': nt + n, 'listed': int(listed.value), 'blocked': int(extra[5].sum().item()), 'reshaped': int(extra[6].sum().item()),
                    'region_status_nonzero': int((extra[7] != 0).sum().item()), 'status_nonzero': int((bufs['clear']['status'] != 0).sum().item())}
    return out


if __name__ == '__main__':
    main()
