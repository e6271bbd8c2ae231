"""Times the path speeds (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum) on the mission
paths of the batch of tools/bench_mission.py: --fields star-shaped polygons of --vertices vertices (radii U[40, 120) m) planned by
plan_polygon_fields(mission='headland_first') at W = --width with --passes headland passes, Dubins and Reeds-Shepp, all outside the timed
windows.  In the same run, ALTERNATING with it, fcpp_speed_plan on the same samples at a constant target speed: the operator the library
had for this before, with the same three-pass shape, 24 B read per pass and 8 B written per sample against 26 B and 16 B here.  And the
host twin (fcpp_debug_path_speeds) on the library's host threads (FCPP_THREADS, at most 16) on the FIRST --host-fields fields, which the
device must meet to the rule's bound (asserted).  Prints ONE JSON line (and writes it to --out).  Needs a GPU; bench.py's metric is not
touched by this."""
import argparse
import ctypes as C
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

HBM_BYTES_PER_S = 8.0e12          # the figure DESIGN.md section 5 relates its streams to
BYTES_HERE = 2 * 26 + 16          # both passes read x, y, kappa, part, gear; the apply pass writes v and cap
BYTES_SPEED_PLAN = 24 + 8 + 24 + 24 + 8          # clamp: x, y, v -> v; tiles: x, y, v; apply: x, y, v -> v


def one_mode(args, torch, ctx, dev, polys, reversing):
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    veh = E.make_vehicle()
    plan = E.plan_polygon_fields(E.polygon_fields(list(polys)), args.width, args.radius, args.spacing,
                                 np.linspace(0.0, np.pi, args.angles, endpoint=False), passes=args.passes, reversing=reversing, headland_paths=True,
                                 mission='headland_first')
    m = plan.mission
    del plan
    n, total, off_h = int(m.offsets.numel()) - 1, int(m.x.numel()), m.offsets_host
    prm = E.speed_params(veh)
    f64 = torch.float64
    v, cap, status = torch.empty(total, dtype=f64, device=dev), torch.empty(total, dtype=f64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    v_in, v_old, nadj = torch.full((total,), veh.max_work_speed_kmh, dtype=f64, device=dev), torch.empty(total, dtype=f64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    ctx.bind_stream()

    def speeds():
        L.check(lib.fcpp_path_speeds(ctx.handle, C.byref(prm), n, P(m.offsets), total, P(m.x), P(m.y), P(m.kappa), P(m.part), P(m.gear), P(v), P(cap),
                                     P(status), HP(off_h)))

    def speed_plan():
        L.check(lib.fcpp_speed_plan(ctx.handle, C.byref(veh), 1, n, P(m.offsets), total, P(m.x), P(m.y), P(v_in), P(v_old), None, P(nadj), HP(off_h)))
    ms = {'path_speeds': [], 'speed_plan': []}
    for r in range(args.warmup + args.reps):
        for name, fn in (('path_speeds', speeds), ('speed_plan', speed_plan)):
            t = _event_ms(torch, fn)
            if r >= args.warmup:
                ms[name].append(t)
    out = {'paths': n, 'samples': total, 'tiles': int(sum(-(-int(k) // 512) for k in np.diff(off_h))), 'failed_paths': int((status != 0).sum().item()),
           'cusp_samples': int((m.gear[1:] != m.gear[:-1]).sum().item()) * 2, 'zero_speed_samples': int((v == 0).sum().item())}
    for name in ms:
        out[name + '_call'] = _stat(ms[name])
    t_new, t_old = out['path_speeds_call']['median_ms'] * 1e-3, out['speed_plan_call']['median_ms'] * 1e-3
    out['ratio_to_speed_plan'] = t_new / t_old
    out['byte_ratio_to_speed_plan'] = BYTES_HERE / BYTES_SPEED_PLAN
    out['bytes_per_sample'] = BYTES_HERE
    out['tb_per_s'] = total * BYTES_HERE / t_new / 1e12
    out['share_of_hbm_stream'] = total * BYTES_HERE / t_new / HBM_BYTES_PER_S
    out['speed_plan_tb_per_s'] = total * BYTES_SPEED_PLAN / t_old / 1e12
    kf = min(args.host_fields, n)
    if kf > 0:
        hi = int(off_h[kf])
        c = lambda a: np.ascontiguousarray(a[:hi].cpu().numpy())
        hx, hy, hk, hp_, hg = c(m.x), c(m.y), c(m.kappa), c(m.part), c(m.gear)
        hoff = np.ascontiguousarray(off_h[:kf + 1])
        hv, hcap, hst = np.zeros(hi), np.zeros(hi), np.zeros(kf, np.int32)
        hp = lambda a: a.ctypes.data
        call = lambda: lib.fcpp_debug_path_speeds(C.byref(prm), kf, hp(hoff), hi, hp(hx), hp(hy), hp(hk), hp(hp_), hp(hg), hp(hv), hp(hcap), hp(hst))
        assert call() == 0, lib.fcpp_last_error()
        t0 = time.perf_counter()
        assert call() == 0, lib.fcpp_last_error()
        t1 = time.perf_counter()
        dv, dcap = c(v), c(cap)
        assert np.array_equal(hst, status[:kf].cpu().numpy()) and np.array_equal(dcap.view(np.int64), hcap.view(np.int64)), 'status or cap differ from the host twin'
        longest = int(np.diff(hoff).max())
        assert (np.abs(dv - hv) <= (longest + 4) * 2.0 ** -52 * hv).all(), 'v misses the bound against the host twin'
        out['host_twin'] = {'threads': min(os.cpu_count() or 1, int(os.environ.get('FCPP_THREADS', 16))), 'fields': kf, 'samples': hi, 'ms': (t1 - t0) * 1e3,
                            'ns_per_sample': (t1 - t0) * 1e9 / hi, 'device_ns_per_sample': t_new * 1e9 / total,
                            'ratio_per_sample': ((t1 - t0) / hi) / (t_new / total), 'within_bound': True,
                            'max_rel_diff_ulps': float(np.nanmax(np.abs(dv - hv) / np.where(hv > 0, hv, np.inf)) / 2.0 ** -52),
                            'note': 'the twin ran on the first %d fields only; the ratio compares time per sample, nothing is extrapolated' % kf}
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
    ap.add_argument('--host-fields', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_path_speeds needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    dev = torch.device('cuda', ctx.device)
    polys = stars(np.random.default_rng(1), args.fields, args.vertices)
    out = {'tool': 'bench_path_speeds', 'reps': args.reps, 'warmup': args.warmup, 'fields': args.fields, 'vertices': args.vertices, 'width': args.width,
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
