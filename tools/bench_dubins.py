"""Times the Dubins entries (HIP events around each call, --reps repetitions after --warmup; median, minimum and maximum):
  (a) fcpp_dubins_matrix at 4096 x 4096 and 16384 x 16384 poses drawn as in the tests (positions U[0, 5000)^2, headings U(-pi, pi], R = 8):
      pairs/s -- beside the number of vector instructions per pair counted in the compiled kernel's ISA (the pair loop of k_conn_matrix<0>:
      every v_* instruction, and those on float64) and the issue-rate bound that follows from it.  On gfx950 a SIMD issues a vector
      instruction for 16 lanes per clock, float64 at the same rate as 32-bit ones: 256 CUs x 4 SIMDs x 16 lanes x clock lane-instructions
      per second.  The count is static (all five argument classes of each atan2 are counted though a lane takes one), so the bound is on
      the low side; the achieved fraction is reported, not gated.
  (b) fcpp_dubins_sample on 65 536 paths at 0.1 m (goals within 1 km of the starts): samples/s and bytes/s written (32 B per sample),
      beside fcpp_trajectory_sample (k_traj_sample, 52 B per sample) on the headline batch measured in the same process.
  (c) for scale only: the numpy restatement of tests/test_dubins_host.py on one core of the same box.
Prints ONE JSON line (and writes it to --out).  Needs a GPU; bench.py's metric is not touched by this."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from field_coverage_path_planning_amd import _lib as L          # noqa: E402
from field_coverage_path_planning_amd import engine as E        # noqa: E402
from field_coverage_path_planning_amd import workloads as W     # noqa: E402


def _stat(ms):
    a = np.sort(np.asarray(ms))
    return {'median_ms': float(np.median(a)), 'min_ms': float(a[0]), 'max_ms': float(a[-1]), 'n': int(len(a))}


def _timed(torch, fn, reps, warmup):
    ms = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    return _stat(ms)


def isa_counts():
    """vector instructions in the pair loop of k_conn_matrix<0>, from the device assembly of csrc/fcpp_conn.hip (the Makefile's flags)
    -> dict, or a note why it could not be counted"""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        return {'note': 'not counted: no hipcc'}
    src = os.path.join(REPO, 'field_coverage_path_planning_amd', 'csrc', 'fcpp_conn.hip')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'dubins.s')
        cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fno-fast-math', '--cuda-device-only', '-S', '-o', out,
               '-x', 'hip', src]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {'note': 'not counted: ' + r.stderr[-300:]}
        lines = open(out).read().split('\n')
    start = next(i for i, l in enumerate(lines) if re.match(r'^_ZN4fcpp13k_conn_matrixILi0EE\w*:', l))
    end = next(i for i in range(start, len(lines)) if 's_endpgm' in lines[i])
    body = lines[start:end]
    head = next(i for i, l in enumerate(body) if 'Loop Header' in l)
    # (the blocks of the loop are marked `in Loop: Header=` in the listing: from the header to the end of the last such block)
    last = max(i for i, l in enumerate(body) if 'in Loop: Header=' in l)
    nxt = next((i for i in range(last + 1, len(body)) if re.match(r'^\.LBB', body[i])), len(body))
    loop = body[head:nxt]
    valu = [l for l in loop if re.match(r'^\s+v_', l)]
    f64 = [l for l in valu if 'f64' in l.split()[0]]
    return {'valu_per_pair': len(valu), 'fp64_valu_per_pair': len(f64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[4096, 16384])
    ap.add_argument('--paths', type=int, default=65536)
    ap.add_argument('--spacing', type=float, default=0.1)
    ap.add_argument('--fields', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--clock-ghz', type=float, default=2.4, help='peak engine clock of the issue-rate bound')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_dubins needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    R = 8.0
    rec = {'tool': 'bench_dubins', 'reps': args.reps, 'warmup': args.warmup, 'radius': R}
    isa = isa_counts()
    rec['isa'] = isa
    lane_rate = 256 * 4 * 16 * args.clock_ghz * 1e9
    rng = np.random.default_rng(1)

    # (a) the transit matrix
    rec['matrix'] = []
    for n in args.sizes:
        poses = np.column_stack((rng.uniform(0, 5000, (n, 2)), -rng.uniform(-np.pi, np.pi, n)))
        f = E._poses(poses, dev)
        D = torch.empty((n, n), dtype=torch.float64, device=dev)
        ctx.bind_stream()

        def run():
            L.check(lib.fcpp_dubins_matrix(ctx.handle, n, P(f[0]), P(f[1]), P(f[2]), n, P(f[0]), P(f[1]), P(f[2]), R, P(D), None))
        st = _timed(torch, run, args.reps, args.warmup)
        row = {'n': n, 'pairs': n * n, 'time': st, 'pairs_per_s': n * n / (st['median_ms'] * 1e-3), 'bytes_written_per_s': 8.0 * n * n / (st['median_ms'] * 1e-3)}
        if 'valu_per_pair' in isa:
            row['bound_pairs_per_s'] = lane_rate / isa['valu_per_pair']
            row['achieved_fraction_of_bound'] = row['pairs_per_s'] / row['bound_pairs_per_s']
        rec['matrix'].append(row)
        del D

    # (b) the sampler, beside k_traj_sample in the same process
    n = args.paths
    frm = np.column_stack((rng.uniform(0, 5000, (n, 2)), -rng.uniform(-np.pi, np.pi, n)))
    to = np.column_stack((frm[:, :2] + rng.uniform(-1000, 1000, (n, 2)), -rng.uniform(-np.pi, np.pi, n)))
    f, t = E._poses(frm, dev), E._poses(to, dev)
    word, seg, length = E._conn_solve(ctx, f, t, R, False)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    off_h = np.zeros(n + 1, dtype=np.int64)
    L.check(lib.fcpp_dubins_counts(ctx.handle, n, P(length), args.spacing, P(off), HP(off_h)))
    m = int(off_h[-1])
    outs = [torch.empty(m, dtype=torch.float64, device=dev) for _ in range(4)]

    def sample():
        L.check(lib.fcpp_dubins_sample(ctx.handle, n, P(f[0]), P(f[1]), P(f[2]), R, P(word), P(seg), args.spacing, P(off), m, *[P(o) for o in outs],
                                       HP(off_h)))
    st = _timed(torch, sample, args.reps, args.warmup)
    rec['sample'] = {'paths': n, 'spacing': args.spacing, 'samples': m, 'time': st, 'samples_per_s': m / (st['median_ms'] * 1e-3),
                     'bytes_written_per_s': 32.0 * m / (st['median_ms'] * 1e-3)}
    st = _timed(torch, lambda: L.check(lib.fcpp_dubins_solve(ctx.handle, n, P(f[0]), P(f[1]), P(f[2]), P(t[0]), P(t[1]), P(t[2]), R, P(word), P(seg),
                                                             P(length))) or torch.cuda.current_stream().synchronize(), args.reps, args.warmup)
    rec['solve'] = {'pairs': n, 'time': st, 'pairs_per_s': n / (st['median_ms'] * 1e-3)}
    del outs

    batch, res = E.Batch.plan(E.FieldTable.from_rectangles(W.cfg1_batch(args.fields)), E.make_vehicle(), E.make_options())
    torch.cuda.synchronize()
    poff_h = res.path_offsets()
    s, tt, h, totals = res.trajectory()
    npts, mp = res.x.numel(), len(poff_h) - 1
    poff = torch.as_tensor(poff_h, device=dev)
    oo = torch.empty(mp + 1, dtype=torch.int64, device=dev)
    oo_h = np.zeros(mp + 1, dtype=np.int64)
    dt = 0.1
    L.check(lib.fcpp_trajectory_counts(ctx.handle, mp, P(totals), dt, 1, P(oo), HP(oo_h)))
    k = int(oo_h[-1])
    touts = [torch.empty(k, dtype=torch.float64, device=dev) for _ in range(5)]
    fss = torch.empty(k, dtype=torch.int32, device=dev)
    src = torch.empty(k, dtype=torch.int64, device=dev)

    def traj_sample():
        L.check(lib.fcpp_trajectory_sample(ctx.handle, mp, P(poff), npts, P(res.x), P(res.y), P(res.v), P(s), P(tt), P(h), P(res.flagseg), dt, 1, P(oo), k,
                                           *[P(o) for o in touts], P(fss), P(src), HP(poff_h), HP(oo_h)))
    st = _timed(torch, traj_sample, args.reps, args.warmup)
    rec['trajectory_sample_same_process'] = {'dt': dt, 'samples': k, 'time': st, 'samples_per_s': k / (st['median_ms'] * 1e-3),
                                             'bytes_written_per_s': 52.0 * k / (st['median_ms'] * 1e-3)}
    del touts, fss, src
    batch.close()

    # (c) the numpy restatement on one core
    from tests.test_dubins_host import random_pairs, restated_totals
    a, b = random_pairs(np.random.default_rng(1), 200_000, R, False)
    t0 = time.perf_counter()
    restated_totals(a, b, R)
    dtm = time.perf_counter() - t0
    rec['numpy_restatement_one_core'] = {'pairs': len(a), 'seconds': dtm, 'pairs_per_s': len(a) / dtm}

    line = json.dumps(rec)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
