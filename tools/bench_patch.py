"""Times the patch passes (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum) on
tools/bench_cover_regions.py's batch: --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) planned by
plan_polygon_fields at W = --width with the headland loops driven, their coverage grids at --res kept and the missed regions of at least
--min-area m^2 labelled (coverage_regions(want_labels=True)), all outside the timed windows; then fcpp_patch_sizes, fcpp_patch_counts and
fcpp_patch_fill at each field's chosen angle, each on its own into buffers allocated before; and the host twin (fcpp_debug_patch_swaths)
on the library's host threads (FCPP_THREADS, at most 16) on the FIRST --host-fields fields, whose frame, records, offsets and swaths must
equal the device's (asserted).  The sizes and the counts call each read every 4-byte label once; bytes_per_cell_at_floor states that.
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
from tools.bench_cover_regions import _event_ms                  # noqa: E402
from tools.bench_swaths import _stat, stars                      # noqa: E402

FLOOR_BYTES = {'sizes': 4, 'counts': 4, 'fill': 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=1024)
    ap.add_argument('--vertices', type=int, default=32)
    ap.add_argument('--angles', type=int, default=36)
    ap.add_argument('--width', type=float, default=3.2)
    ap.add_argument('--res', type=float, default=0.25)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--spacing', type=float, default=0.5)
    ap.add_argument('--min-area', type=float, default=1.0)
    ap.add_argument('--host-fields', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_patch needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    n, Wd, res = args.fields, args.width, args.res
    polys = stars(np.random.default_rng(1), n, args.vertices)
    pf = E.polygon_fields(list(polys))
    plan = E.plan_polygon_fields(pf, Wd, args.radius, args.spacing, np.linspace(0.0, np.pi, args.angles, endpoint=False), headland_paths=True)
    cov = E.polygon_coverage(pf, Wd, res, paths=(plan.paths, plan.headland_paths), want_grid=True)
    ang = plan.angle.contiguous()
    del plan
    reg = E.coverage_regions(cov, 'missed', min_area=args.min_area, want_labels=True)
    dims, coff, coff_h = cov.dims.contiguous(), cov.cell_offsets.contiguous(), np.ascontiguousarray(cov.cell_offsets_host, dtype=np.int64)
    labels, roff, roff_h = reg.labels.contiguous(), reg.offsets.contiguous(), np.ascontiguousarray(reg.offsets_host, dtype=np.int64)
    cells, k = int(coff_h[-1]), int(roff_h[-1])
    margin, join = res / 2, Wd
    rule = (float(Wd), margin, join)
    i64, f64 = torch.int64, torch.float64
    frame, rec, totals = torch.empty((n, 2), dtype=f64, device=dev), torch.empty((k, 8), dtype=i64, device=dev), np.zeros(2, np.int64)
    ctx.bind_stream()

    def sizes():
        L.check(lib.fcpp_patch_sizes(ctx.handle, n, P(dims), P(coff), HP(coff_h), res, P(labels), P(roff), HP(roff_h), k, P(ang), *rule, P(frame), P(rec),
                                     HP(totals)))
    sizes()
    nl, nw = int(totals[0]), int(totals[1])
    bitmap, cnt = torch.empty(nw, dtype=i64, device=dev), torch.empty(nl, dtype=i64, device=dev)
    loff, soff, soff_h = torch.empty(nl + 1, dtype=i64, device=dev), torch.empty(n + 1, dtype=i64, device=dev), np.zeros(n + 1, np.int64)

    def counts():
        L.check(lib.fcpp_patch_counts(ctx.handle, n, P(dims), P(coff), HP(coff_h), res, P(labels), P(roff), HP(roff_h), k, P(frame), *rule, P(rec), nl, nw,
                                      P(bitmap), P(cnt), P(loff), P(soff), HP(soff_h)))
    counts()
    ms = int(soff_h[-1])
    a, b = torch.empty((2, ms), dtype=f64, device=dev), torch.empty((2, ms), dtype=f64, device=dev)
    line, length, region = torch.empty(ms, dtype=torch.int32, device=dev), torch.empty(ms, dtype=f64, device=dev), torch.empty(ms, dtype=i64, device=dev)

    def fill():
        L.check(lib.fcpp_patch_fill(ctx.handle, n, P(dims), res, P(roff), HP(roff_h), k, P(frame), *rule, P(rec), nl, nw, P(bitmap), P(loff), ms, P(a[0]),
                                    P(a[1]), P(b[0]), P(b[1]), P(line), P(length), P(region)))
    t = {'sizes': [], 'counts': [], 'fill': []}
    for r in range(args.warmup + args.reps):
        for name, fn in (('sizes', sizes), ('counts', counts), ('fill', fill)):
            v = _event_ms(torch, fn)
            if r >= args.warmup:
                t[name].append(v)
    out = {'tool': 'bench_patch', 'reps': args.reps, 'warmup': args.warmup, 'fields': n, 'vertices': args.vertices, 'width': Wd, 'res': res,
           'radius': args.radius, 'spacing': args.spacing, 'min_area': args.min_area, 'margin': margin, 'join': join,
           'batch': {'cells': cells, 'member_cells': int((labels >= 0).sum().item()), 'regions': k, 'lines': nl, 'bitmap_words': nw, 'swaths': ms,
                     'swath_length_m': float(length.sum().item()), 'unsupported_regions': int((rec[:, 6] != 0).sum().item())},
           'bytes_per_cell_at_floor': FLOOR_BYTES, 'kernel_times': 'not measured (no trace in this run)'}
    for name in ('sizes', 'counts', 'fill'):
        s = _stat(t[name])
        out[name + '_call'] = {'time': s, 'cells_per_s': cells / (s['median_ms'] * 1e-3),
                               'GBps_at_floor_bytes': FLOOR_BYTES[name] * cells / (s['median_ms'] * 1e-3) / 1e9}
    kf = min(args.host_fields, n)
    if kf > 0:
        hc, hk = int(coff_h[kf]), int(roff_h[kf])
        hd, ho = np.ascontiguousarray(dims[:kf].cpu().numpy()), np.ascontiguousarray(coff_h[:kf + 1])
        hl, hr, ha = np.ascontiguousarray(labels[:hc].cpu().numpy()), np.ascontiguousarray(roff_h[:kf + 1]), np.ascontiguousarray(ang[:kf].cpu().numpy())
        hp = lambda x: None if x is None else x.ctypes.data
        head = (kf, hp(hd), hp(ho), res, hp(hl), hp(hr), hk, hp(ha), *rule)
        tot = np.zeros(3, np.int64)
        rc = lib.fcpp_debug_patch_swaths(*head, None, None, hp(tot), 0, None, 0, None, None, None, 0, *([None] * 7))          # the sizes
        assert rc == 0, lib.fcpp_last_error()
        hn = int(tot[2])
        hframe, hrec, hsoff = np.zeros(2 * kf), np.zeros((hk, 8), np.int64), np.zeros(kf + 1, np.int64)
        f8 = lambda: np.zeros(hn)
        hax, hay, hbx, hby, hlen, hline, hreg = f8(), f8(), f8(), f8(), f8(), np.zeros(hn, np.int32), np.zeros(hn, np.int64)
        t0 = time.perf_counter()
        rc = lib.fcpp_debug_patch_swaths(*head, hp(hframe), hp(hrec), hp(tot), 0, None, 0, None, None, hp(hsoff), hn, hp(hax), hp(hay), hp(hbx), hp(hby),
                                         hp(hline), hp(hlen), hp(hreg))
        t1 = time.perf_counter()
        assert rc == 0, lib.fcpp_last_error()
        c = lambda x: x.cpu().numpy()
        assert np.array_equal(hsoff, soff_h[:kf + 1]), 'swath offsets differ from the host twin'
        assert np.array_equal(hframe, c(frame[:kf]).reshape(-1)) and np.array_equal(hrec, c(rec[:hk])), 'frame or records differ from the host twin'
        for got, want, what in ((a[0], hax, 'ax'), (a[1], hay, 'ay'), (b[0], hbx, 'bx'), (b[1], hby, 'by'), (line, hline, 'line'), (length, hlen, 'length'),
                                (region, hreg, 'region')):
            assert np.array_equal(c(got[:hn]), want), what + ' differs from the host twin'
        per_cell = (t1 - t0) / max(hc, 1)
        dev_per_cell = sum(out[name + '_call']['time']['median_ms'] for name in ('sizes', 'counts', 'fill')) * 1e-3 / cells
        out['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'fields': kf, 'cells': hc, 'swaths': hn,
                            'ms': (t1 - t0) * 1e3, 'ns_per_cell': per_cell * 1e9, 'device_ns_per_cell_three_calls': dev_per_cell * 1e9,
                            'ratio_per_cell': per_cell / dev_per_cell, 'equal': {'frame': True, 'records': True, 'offsets': True, 'swaths': True},
                            'note': 'the twin ran on the first %d fields only; the ratio compares time per cell, nothing is extrapolated' % kf}
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
