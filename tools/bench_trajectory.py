"""Times the trajectory entries against the existing operator that reads the same arrays (fcpp_verify), in one process:
  (a) the headline batch's points (4096 fields of 500 x 200 m) as 8192 paths, main work and headland of every field;
  (b) one path of 3.2e7 points (a spiral with duplicates and a jump): the scan's spine over 62 500 tiles;
  and fcpp_trajectory_counts + fcpp_trajectory_sample at dt = 0.1 s on (a).
HIP events around each call (every call ends in its own stream synchronisation), the two operators alternating, --reps repetitions after
--warmup; median, minimum and maximum per operator.  Bytes are the algorithm's: 24 B read and 24 B written per point for the trajectory.
Prints ONE JSON line.  Needs a GPU; bench.py's metric is not touched by this."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from field_coverage_path_planning_amd import _lib as L          # noqa: E402
from field_coverage_path_planning_amd import engine as E        # noqa: E402
from field_coverage_path_planning_amd import workloads as W     # noqa: E402


def _stat(ms):
    a = np.sort(np.asarray(ms))
    return {'median_ms': float(np.median(a)), 'min_ms': float(a[0]), 'max_ms': float(a[-1]), 'n': int(len(a))}


def time_pair(torch, ctx, x, y, v, off_h, reps, warmup):
    """-> (verify stats, trajectory stats) on the same paths; all three trajectory outputs, no flags"""
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = x.device
    off = torch.as_tensor(off_h, device=dev)
    n, m = x.numel(), len(off_h) - 1
    veh = E.make_vehicle()
    stats = torch.zeros((m, L.STATS_WORDS), dtype=torch.int64, device=dev)
    s, t, h = (torch.empty_like(x) for _ in range(3))
    totals = torch.zeros((m, 2), dtype=torch.float64, device=dev)
    ctx.bind_stream()

    def verify():
        L.check(lib.fcpp_verify(ctx.handle, C.byref(veh), m, P(off), n, P(x), P(y), P(v), P(stats), HP(off_h)))

    def traj():
        L.check(lib.fcpp_trajectory(ctx.handle, m, P(off), n, P(x), P(y), P(v), None, P(s), P(t), P(h), P(totals), HP(off_h)))

    out = {'verify': [], 'trajectory': []}
    for k in range(warmup + reps):
        for name, fn in (('verify', verify), ('trajectory', traj)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                out[name].append(e0.elapsed_time(e1))
    return _stat(out['verify']), _stat(out['trajectory']), (s, t, h, totals, off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=4096)
    ap.add_argument('--long-points', type=int, default=32_000_000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dt', type=float, default=0.1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_trajectory needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    rec = {'tool': 'bench_trajectory', 'reps': args.reps, 'warmup': args.warmup}

    # (a) the headline batch as 2 x fields paths
    batch, res = E.Batch.plan(E.FieldTable.from_rectangles(W.cfg1_batch(args.fields)), E.make_vehicle(), E.make_options())
    torch.cuda.synchronize()
    off_h = res.path_offsets()
    x, y, v = res.x.clone(), res.y.clone(), res.v.clone()
    ver, trj, (s, t, h, totals, off) = time_pair(torch, ctx, x, y, v, off_h, args.reps, args.warmup)
    n = x.numel()
    rec['a'] = {'points': n, 'paths': len(off_h) - 1, 'verify': ver, 'trajectory': trj, 'ratio_median': trj['median_ms'] / ver['median_ms'],
                'trajectory_bytes_per_s': 48.0 * n / (trj['median_ms'] * 1e-3)}
    # the samples of (a) at dt
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    m = len(off_h) - 1
    oo = torch.empty(m + 1, dtype=torch.int64, device=x.device)
    oo_h = np.zeros(m + 1, dtype=np.int64)
    L.check(lib.fcpp_trajectory_counts(ctx.handle, m, P(totals), args.dt, 1, P(oo), HP(oo_h)))
    k = int(oo_h[-1])
    outs = [torch.empty(k, dtype=torch.float64, device=x.device) for _ in range(5)]
    fss = torch.empty(k, dtype=torch.int32, device=x.device)
    src = torch.empty(k, dtype=torch.int64, device=x.device)
    fs = res.flagseg.clone()
    cnt_ms, smp_ms = [], []
    for r in range(args.warmup + args.reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        L.check(lib.fcpp_trajectory_counts(ctx.handle, m, P(totals), args.dt, 1, P(oo), HP(oo_h)))
        e[1].record()
        L.check(lib.fcpp_trajectory_sample(ctx.handle, m, P(off), n, P(x), P(y), P(v), P(s), P(t), P(h), P(fs), args.dt, 1, P(oo), k,
                                           *[P(o) for o in outs], P(fss), P(src), HP(off_h), HP(oo_h)))
        e[2].record()
        e[2].synchronize()
        if r >= args.warmup:
            cnt_ms.append(e[0].elapsed_time(e[1]))
            smp_ms.append(e[1].elapsed_time(e[2]))
    st = _stat(smp_ms)
    rec['sample'] = {'dt': args.dt, 'samples': k, 'counts': _stat(cnt_ms), 'sample': st, 'samples_per_s': k / (st['median_ms'] * 1e-3),
                     'output_bytes_per_s': 52.0 * k / (st['median_ms'] * 1e-3)}
    del outs, fss, src, s, t, h, x, y, v, res
    batch.close()

    # (b) one long path
    n = args.long_points
    i = torch.arange(n, dtype=torch.float64, device='cuda')
    r, th = 50.0 + 1e-5 * i, 2e-4 * i
    x, y = r * torch.cos(th), r * torch.sin(th)
    del r, th, i
    dup = torch.arange(1_000_003, n, 1_000_003, device='cuda')
    x[dup], y[dup] = x[dup - 1], y[dup - 1]
    x[n // 2:] += 25.0
    v = torch.as_tensor(np.random.default_rng(3).choice([2.5, 4.0, 9.0, 14.0, 15.0], size=n), device='cuda')
    ver, trj, _ = time_pair(torch, ctx, x, y, v, np.array([0, n], dtype=np.int64), args.reps, args.warmup)
    rec['b'] = {'points': n, 'paths': 1, 'verify': ver, 'trajectory': trj, 'ratio_median': trj['median_ms'] / ver['median_ms'],
                'trajectory_bytes_per_s': 48.0 * n / (trj['median_ms'] * 1e-3),
                'share_of_8_TB_per_s': 48.0 * n / (trj['median_ms'] * 1e-3) / 8e12}
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
