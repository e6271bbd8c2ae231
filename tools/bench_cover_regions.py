"""Times the coverage regions (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum) on
tools/bench_polygon_cover.py's batch: --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) planned by
plan_polygon_fields at W = --width with the headland loops driven, their coverage grids at --res kept (polygon_coverage(want_grid=True)),
all outside the timed windows; then, for kind 'missed' under connectivity 4 and 8, fcpp_cover_regions_counts and fcpp_cover_regions_fill,
each on its own into buffers allocated before (a repetition is one counts call and one fill call: the fill consumes the counts' labels);
and the host twin (fcpp_debug_cover_regions) on the library's host threads (FCPP_THREADS, at most 16) on the FIRST --host-fields fields,
once per connectivity, whose offsets, records and labels must equal the device's (asserted).  The floor per cell is one grid byte read and the
4-byte label written and read again a few times; bytes_per_cell_at_floor states the count the figures are set against.
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
from tools.bench_swaths import _stat, stars                      # noqa: E402

# counts: the grid byte, the label written by the tile pass, read and written by the flatten pass; fill: the label read by the count,
# the first and the fill pass and written once
FLOOR_BYTES = {'counts': 1 + 4 + 4 + 4, 'fill': 4 + 4 + 4 + 4}


def _event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=1024)
    ap.add_argument('--vertices', type=int, default=32)
    ap.add_argument('--angles', type=int, default=36)
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--res', type=float, default=0.25)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--spacing', type=float, default=0.5)
    ap.add_argument('--kind', default='missed')
    ap.add_argument('--host-fields', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_cover_regions needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, Wd, res = args.fields, args.width, args.res
    mask, value = E.REGION_KINDS[args.kind]
    polys = stars(np.random.default_rng(1), n, args.vertices)
    pf = E.polygon_fields(list(polys))
    plan = E.plan_polygon_fields(pf, Wd, args.radius, args.spacing, np.linspace(0.0, np.pi, args.angles, endpoint=False), headland_paths=True)
    cov = E.polygon_coverage(pf, Wd, res, paths=(plan.paths, plan.headland_paths), want_grid=True)
    del plan
    dims, coff, coff_h = cov.dims.contiguous(), cov.cell_offsets.contiguous(), np.ascontiguousarray(cov.cell_offsets_host, dtype=np.int64)
    cells = int(coff_h[-1])
    c = cov.counts.cpu().numpy()
    nxny = dims[:, 2:].cpu().numpy()
    rec = {'tool': 'bench_cover_regions', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': Wd, 'res': res,
           'radius': args.radius, 'spacing': args.spacing, 'kind': args.kind, 'mask': mask, 'value': value,
           'batch': {'cells': cells, 'tiles': int((((nxny[:, 0] + 63) // 64) * ((nxny[:, 1] + 63) // 64)).sum()), 'inside': int(c[:, 0].sum()),
                     'covered': int(c[:, 1].sum()), 'missed_cells': int((c[:, 0] - c[:, 1]).sum()), 'label_bytes': 4 * cells},
           'bytes_per_cell_at_floor': FLOOR_BYTES, 'kernel_times': 'not measured (no trace in this run)'}
    labels = torch.empty(cells, dtype=torch.int32, device=dev)
    roff, roff_h = torch.empty(n + 1, dtype=torch.int64, device=dev), np.zeros(n + 1, dtype=np.int64)
    ctx.bind_stream()
    k = min(args.host_fields, n)
    host_in = None
    if k > 0:
        hc = int(coff_h[k])
        host_in = (np.ascontiguousarray(dims[:k].cpu().numpy()), np.ascontiguousarray(coff_h[:k + 1]), np.ascontiguousarray(cov.cells[:hc].cpu().numpy()))

    for connectivity in (4, 8):
        def counts():
            L.check(lib.fcpp_cover_regions_counts(ctx.handle, n, P(dims), P(coff), HP(coff_h), P(cov.cells), mask, value, connectivity, P(labels), P(roff),
                                                  HP(roff_h)))
        counts()
        regions = int(roff_h[-1])
        records = torch.empty((regions, 6), dtype=torch.int64, device=dev)

        def fill():
            L.check(lib.fcpp_cover_regions_fill(ctx.handle, n, P(dims), P(coff), HP(coff_h), P(labels), P(roff), HP(roff_h), regions, P(records)))
        tc, tf = [], []
        for r in range(args.warmup + args.reps):
            a = _event_ms(torch, counts)
            keys_head = labels[:int(coff_h[k])].cpu().numpy() if (k > 0 and r == 0) else None
            b = _event_ms(torch, fill)
            if r == 0:
                keys0 = keys_head
            if r >= args.warmup:
                tc.append(a)
                tf.append(b)
        sc, sf = _stat(tc), _stat(tf)
        rcells = records[:, 1]
        out = {'regions': regions, 'largest_region_cells': int(rcells.max().item()) if regions else 0,
               'regions_of_one_cell': int((rcells == 1).sum().item()), 'regions_under_1_m2': int((rcells.to(torch.float64) * res * res < 1.0).sum().item()),
               'counts_call': {'time': sc, 'cells_per_s': cells / (sc['median_ms'] * 1e-3),
                               'GBps_at_floor_bytes': FLOOR_BYTES['counts'] * cells / (sc['median_ms'] * 1e-3) / 1e9},
               'fill_call': {'time': sf, 'cells_per_s': cells / (sf['median_ms'] * 1e-3),
                             'GBps_at_floor_bytes': FLOOR_BYTES['fill'] * cells / (sf['median_ms'] * 1e-3) / 1e9}}
        if k > 0:
            hd, ho, hg = host_in
            hro = np.zeros(k + 1, np.int64)
            hp = lambda a: a.ctypes.data
            rc = lib.fcpp_debug_cover_regions(k, hp(hd), hp(ho), hp(hg), mask, value, connectivity, hp(hro), 0, None, None, None)      # the sizes
            assert rc == 0, lib.fcpp_last_error()
            hrec = np.zeros((int(hro[-1]), 6), np.int64)
            hkeys, hidx = np.zeros(len(hg), np.int32), np.zeros(len(hg), np.int32)
            t0 = time.perf_counter()
            rc = lib.fcpp_debug_cover_regions(k, hp(hd), hp(ho), hp(hg), mask, value, connectivity, hp(hro), len(hrec), hp(hrec), hp(hkeys), hp(hidx))
            t1 = time.perf_counter()
            assert rc == 0, lib.fcpp_last_error()
            assert np.array_equal(hro, roff_h[:k + 1]), 'region offsets differ from the host twin'
            assert np.array_equal(hrec, records[:int(hro[-1])].cpu().numpy()), 'records differ from the host twin'
            assert np.array_equal(hkeys, keys0), 'labels after counts differ from the host twin'
            assert np.array_equal(hidx, labels[:len(hg)].cpu().numpy()), 'labels after fill differ from the host twin'
            per_cell = (t1 - t0) / max(len(hg), 1)
            dev_per_cell = (sc['median_ms'] + sf['median_ms']) * 1e-3 / cells
            out['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'fields': k, 'cells': int(len(hg)),
                                'ms': (t1 - t0) * 1e3, 'ns_per_cell': per_cell * 1e9,
                                'device_ns_per_cell_counts_plus_fill': dev_per_cell * 1e9, 'ratio_per_cell': per_cell / dev_per_cell,
                                'equal': {'offsets': True, 'records': True, 'labels_after_counts': True, 'labels_after_fill': True},
                                'note': 'the twin ran on the first %d fields only; the ratio compares time per cell, nothing is extrapolated' % k}
        rec['connectivity_%d' % connectivity] = out

    text = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
