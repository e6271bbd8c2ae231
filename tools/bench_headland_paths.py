"""Times the headland paths (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum):
  (a) tools/bench_inset.py's configuration: --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m), three headland
      passes at W = --width (the insets at W/2, 3W/2, 5W/2, arc_step --arc-step), cut outside the timed windows;
  (b) headland_paths at R = --radius and --spacing (Dubins; --reversing: Reeds-Shepp) over all rings: the whole call (counts + fill,
      allocations of the outputs included), and fcpp_headland_path_counts and fcpp_headland_path_fill each on its own into buffers
      allocated before -- the split between the two calls.  The fill CALL recomputes the leg records, reads the two ends of the slot
      offsets back and synchronises: its samples/s and its share of the 8 TB/s write stream at 38 B per sample are the call's, not the fill
      kernel's alone.  The kernels' own times and the scan's share of the counts call are NOT measured here;
  (c) the host twin (fcpp_debug_headland_paths, sizing call + filling call) on the library's host threads (FCPP_THREADS, at most 16) on
      the same rings, once, with the device results compared bit for bit.
Prints ONE JSON line and writes it to --out (default profiles/headland_paths_bench.json).  Needs a GPU; bench.py's metric is not touched
by this."""
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
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--arc-step', type=float, default=0.1)
    ap.add_argument('--radius', type=float, default=6.0)
    ap.add_argument('--spacing', type=float, default=0.5)
    ap.add_argument('--reversing', action='store_true')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'headland_paths_bench.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_headland_paths needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, Wd, R, sp, rev = args.fields, args.width, args.radius, args.spacing, bool(args.reversing)
    rec = {'tool': 'bench_headland_paths', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': Wd, 'passes': 3,
           'arc_step': args.arc_step, 'radius': R, 'spacing': sp, 'mode': 'reeds_shepp' if rev else 'dubins', 'bytes_per_sample': BYTES_PER_SAMPLE}
    polys = stars(np.random.default_rng(1), n, args.vertices)
    lines, _ = E.headland(list(polys), Wd, 3, arc_step=args.arc_step)
    nr, nv = int(lines.ring_offsets.numel()) - 1, int(lines.x.numel())
    rec['rings'] = {'total': nr, 'vertices': nv, 'leg_slots': 2 * nv, 'bad_pairs': int((lines.status != 0).sum().item())}

    box = {}

    def whole():
        box['hp'] = E.headland_paths(lines, R, sp, reversing=rev)
    tw = _timed(torch, whole, args.reps, args.warmup)
    hp = box['hp']
    total = int(hp.offsets_host[-1])
    part, kinds = hp.part.cpu().numpy(), np.diff(hp.leg_offsets.cpu().numpy())
    rec['samples'] = {'total': total, 'per_ring': total / max(nr, 1), 'connector_share': float((part == 1).mean()) if total else 0.0,
                      'arc_share': float((part == 4).mean()) if total else 0.0, 'legs': int((kinds > 0).sum()),
                      'status_nonzero': int((hp.status != 0).sum().item()), 'skipped_m': float(hp.skipped_length.nan_to_num().sum().item()),
                      'work_m': float(hp.work_length.nan_to_num().sum().item()), 'transit_m': float(hp.transit_length.nan_to_num().sum().item())}
    rec['headland_paths'] = {'time': tw, 'samples_per_s': total / (tw['median_ms'] * 1e-3), 'rings_per_s': nr / (tw['median_ms'] * 1e-3)}
    rec['headland_paths_ms'] = tw['median_ms']

    # the two entries on their own, into buffers allocated before
    roff_h = np.ascontiguousarray(lines.ring_offsets.cpu().numpy(), dtype=np.int64)
    rdist = lines.distances[hp.ring_pair[:, 1]].contiguous()
    head = (ctx.handle, nr, P(lines.ring_offsets), HP(roff_h), nv, P(lines.x), P(lines.y), P(lines.src), P(rdist), E._chord_radius(R, sp), 1 if rev else 0,
            sp, 1, 1e-6)
    off, leg_off = torch.empty(nr + 1, dtype=torch.int64, device=dev), torch.empty(2 * nv + 1, dtype=torch.int64, device=dev)
    off_h = np.zeros(nr + 1, dtype=np.int64)
    work, transit, skipped = (torch.empty(nr, dtype=torch.float64, device=dev) for _ in range(3))
    status = torch.empty(nr, dtype=torch.int32, device=dev)
    x, y, h, kap = (torch.empty(total, dtype=torch.float64, device=dev) for _ in range(4))
    prt, gear = torch.empty(total, dtype=torch.int8, device=dev), torch.empty(total, dtype=torch.int8, device=dev)
    leg = torch.empty(total, dtype=torch.int32, device=dev)
    ctx.bind_stream()

    def counts():
        L.check(lib.fcpp_headland_path_counts(*head, P(off), HP(off_h), P(leg_off), P(work), P(transit), P(skipped), P(status)))

    def fill():
        L.check(lib.fcpp_headland_path_fill(*head, P(leg_off), total, P(x), P(y), P(h), P(kap), P(prt), P(gear), P(leg)))
    tc = _timed(torch, counts, args.reps, args.warmup)
    tf = _timed(torch, fill, args.reps, args.warmup)
    assert int(off_h[-1]) == total and torch.equal(x, hp.x) and torch.equal(leg, hp.leg)
    rate = total / (tf['median_ms'] * 1e-3)
    rec['counts_call'] = {'time': tc, 'slots_per_s': 2 * nv / (tc['median_ms'] * 1e-3)}
    rec['fill_call'] = {'time': tf, 'samples_per_s': rate, 'bytes_per_s': rate * BYTES_PER_SAMPLE,
                        'share_of_8TBps_write_stream': rate * BYTES_PER_SAMPLE / HBM_PEAK}
    rec['split'] = {'counts_ms': tc['median_ms'], 'fill_ms': tf['median_ms'], 'counts_share': tc['median_ms'] / (tc['median_ms'] + tf['median_ms'])}
    rec['not_measured'] = 'the kernels\' own times and the scan\'s share of the counts call'

    if not args.no_host:
        p = lambda a: None if a is None else a.ctypes.data
        hx, hy, hsrc, hdist = (np.ascontiguousarray(t.cpu().numpy()) for t in (lines.x, lines.y, lines.src, rdist))
        hoff, hleg = np.zeros(nr + 1, np.int64), np.zeros(2 * nv + 1, np.int64)
        hhead = (nr, p(roff_h), nv, p(hx), p(hy), p(hsrc), p(hdist), E._chord_radius(R, sp), 1 if rev else 0, sp, 1, 1e-6, p(hoff), p(hleg),
                 *([None] * 8))
        t0 = time.perf_counter()
        assert lib.fcpp_debug_headland_paths(*hhead, 0, *([None] * 7)) == 0
        ht = int(hoff[-1])
        outs = [np.empty(ht, dt) for dt in (np.float64, np.float64, np.float64, np.float64, np.int8, np.int8, np.int32)]
        assert lib.fcpp_debug_headland_paths(*hhead, ht, *[p(a) for a in outs]) == 0
        t1 = time.perf_counter()
        same = bool(ht == total and np.array_equal(hleg, hp.leg_offsets.cpu().numpy())
                    and all(np.array_equal(a.view(np.uint8), getattr(hp, k).cpu().numpy().view(np.uint8))
                            for a, k in zip(outs, ('x', 'y', 'heading', 'kappa', 'part', 'gear', 'leg'))))
        rec['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'ms': (t1 - t0) * 1e3,
                            'device_equals_host_bit_for_bit': same, 'speedup_over_counts_plus_fill': ((t1 - t0) * 1e3) / (tc['median_ms'] + tf['median_ms'])}

    out = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(out + '\n')
    print(out)


if __name__ == '__main__':
    main()
