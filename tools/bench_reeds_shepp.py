"""Times the Reeds-Shepp entries beside the Dubins ones IN THE SAME PROCESS (HIP events around each call, --reps repetitions after --warmup;
median, minimum and maximum):
  (a) fcpp_rs_matrix and fcpp_dubins_matrix at 4096 x 4096 and 16384 x 16384 poses drawn as in the tests (positions U[0, 5000)^2, headings
      U(-pi, pi], R = 8): pairs/s, their ratio, and for each kernel the number of vector instructions per pair counted in the compiled pair
      loop (the method of tools/bench_dubins.py: every v_* instruction of the loop's blocks, and those on float64) with the issue-rate
      bound that follows -- 256 CUs x 4 SIMDs x 16 lanes x clock lane-instructions per second -- and the achieved fraction of it.  The
      count is static (every argument class of each atan2 is counted though a lane takes one), so the bound is on the low side.
  (b) fcpp_rs_sample (33 B per sample) and fcpp_dubins_sample (32 B) on 65 536 paths at 0.1 m (goals within 1 km of the starts):
      samples/s and bytes/s written.
--isa-only counts the instructions and prints them (no GPU needed: hipcc cross-compiles); --isa FILE takes such a record instead of
compiling.  Prints ONE JSON line; it is written to a file only when --out names one (as tools/bench_dubins.py: the committed record is
profiles/reeds_shepp_bench.json, made with --out profiles/reeds_shepp_bench.json).  bench.py's metric is not touched by this."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from field_coverage_path_planning_amd import _lib as L          # noqa: E402
from field_coverage_path_planning_amd import engine as E        # noqa: E402


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


def isa_counts(source, kernel):
    """vector instructions in the pair loop of a matrix kernel, from the device assembly of csrc/<source> (the Makefile's flags), and the
    kernel's registers, LDS and scratch from the assembly's metadata -> dict, or a note why it could not be counted"""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        return {'note': 'not counted: no hipcc'}
    src = os.path.join(REPO, 'field_coverage_path_planning_amd', 'csrc', source)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'k.s')
        cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fno-fast-math', '--cuda-device-only', '-S', '-o', out,
               '-x', 'hip', src]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        if r.returncode != 0:
            return {'note': 'not counted: ' + r.stderr[-300:]}
        lines = open(out).read().split('\n')
    start = next(i for i, l in enumerate(lines) if re.match(r'^_ZN4fcpp\d+' + kernel + r'\w*:', l))
    end = next(i for i in range(start, len(lines)) if 's_endpgm' in lines[i])
    body = lines[start:end]
    head = next(i for i, l in enumerate(body) if 'Loop Header' in l)
    last = max(i for i, l in enumerate(body) if 'in Loop: Header=' in l)
    nxt = next((i for i in range(last + 1, len(body)) if re.match(r'^\.LBB', body[i])), len(body))
    loop = body[head:nxt]
    valu = [l for l in loop if re.match(r'^\s+v_', l)]
    f64 = [l for l in valu if 'f64' in l.split()[0]]
    rec = {'valu_per_pair': len(valu), 'fp64_valu_per_pair': len(f64)}
    tail = lines[end:end + 400]
    for key, pat in (('vgprs', r'; NumVgprs: (\d+)'), ('agprs', r'; NumAgprs: (\d+)'), ('sgprs', r'; NumSgprs: (\d+)'), ('scratch_bytes', r'; ScratchSize: (\d+)'),
                     ('lds_bytes', r'; LDSByteSize: (\d+)'), ('occupancy_waves_per_simd', r'; Occupancy: (\d+)')):
        m = next((re.search(pat, l) for l in tail if re.search(pat, l)), None)
        if m:
            rec[key] = int(m.group(1))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[4096, 16384])
    ap.add_argument('--paths', type=int, default=65536)
    ap.add_argument('--spacing', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--clock-ghz', type=float, default=2.4, help='peak engine clock of the issue-rate bound')
    ap.add_argument('--isa-only', action='store_true')
    ap.add_argument('--isa', default=None, help='a record written by --isa-only')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.isa:
        isa = json.load(open(args.isa))
    else:
        isa = {'rs': isa_counts('fcpp_conn.hip', 'k_conn_matrixILi1EE'), 'dubins': isa_counts('fcpp_conn.hip', 'k_conn_matrixILi0EE')}
    if args.isa_only:
        line = json.dumps(isa)
        if args.out:
            open(args.out, 'w').write(line + '\n')
        print(line)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_reeds_shepp needs a GPU: there is no CPU path to time')
    ctx = E.get_context()
    lib, P, HP = ctx.lib, E._ptr, E._host_ptr
    dev = torch.device('cuda', ctx.device)
    R = 8.0
    rec = {'tool': 'bench_reeds_shepp', 'reps': args.reps, 'warmup': args.warmup, 'radius': R, 'isa': isa}
    lane_rate = 256 * 4 * 16 * args.clock_ghz * 1e9
    rng = np.random.default_rng(1)

    # (a) the two transit matrices
    rec['matrix'] = []
    for n in args.sizes:
        poses = np.column_stack((rng.uniform(0, 5000, (n, 2)), -rng.uniform(-np.pi, np.pi, n)))
        f = E._poses(poses, dev)
        D = torch.empty((n, n), dtype=torch.float64, device=dev)
        ctx.bind_stream()
        row = {'n': n, 'pairs': n * n}
        for name, entry in (('rs', lib.fcpp_rs_matrix), ('dubins', lib.fcpp_dubins_matrix)):
            def run():
                L.check(entry(ctx.handle, n, P(f[0]), P(f[1]), P(f[2]), n, P(f[0]), P(f[1]), P(f[2]), R, P(D), None))
            st = _timed(torch, run, args.reps, args.warmup)
            r = {'time': st, 'pairs_per_s': n * n / (st['median_ms'] * 1e-3)}
            if 'valu_per_pair' in isa.get(name, {}):
                r['bound_pairs_per_s'] = lane_rate / isa[name]['valu_per_pair']
                r['achieved_fraction_of_bound'] = r['pairs_per_s'] / r['bound_pairs_per_s']
            row[name] = r
        row['rs_over_dubins_time'] = row['rs']['time']['median_ms'] / row['dubins']['time']['median_ms']
        rec['matrix'].append(row)
        del D

    # (b) the two samplers on the same pairs
    n = args.paths
    frm = np.column_stack((rng.uniform(0, 5000, (n, 2)), -rng.uniform(-np.pi, np.pi, n)))
    to = np.column_stack((frm[:, :2] + rng.uniform(-1000, 1000, (n, 2)), -rng.uniform(-np.pi, np.pi, n)))
    f, t = E._poses(frm, dev), E._poses(to, dev)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    off_h = np.zeros(n + 1, dtype=np.int64)
    rec['sample'] = {'paths': n, 'spacing': args.spacing}
    word, seg, length = E._conn_solve(ctx, f, t, R, True)
    L.check(lib.fcpp_rs_counts(ctx.handle, n, P(word), P(seg), args.spacing, P(off), HP(off_h)))
    m = int(off_h[-1])
    outs = [torch.empty(m, dtype=torch.float64, device=dev) for _ in range(4)]
    gear = torch.empty(m, dtype=torch.int8, device=dev)
    st = _timed(torch, lambda: L.check(lib.fcpp_rs_sample(ctx.handle, n, P(f[0]), P(f[1]), P(f[2]), R, P(word), P(seg), args.spacing, P(off), m,
                                                          *[P(o) for o in outs], P(gear), HP(off_h))), args.reps, args.warmup)
    rec['sample']['rs'] = {'samples': m, 'time': st, 'samples_per_s': m / (st['median_ms'] * 1e-3), 'bytes_written_per_s': 33.0 * m / (st['median_ms'] * 1e-3)}
    del outs, gear
    word, seg, length = E._conn_solve(ctx, f, t, R, False)
    L.check(lib.fcpp_dubins_counts(ctx.handle, n, P(length), args.spacing, P(off), HP(off_h)))
    m = int(off_h[-1])
    outs = [torch.empty(m, dtype=torch.float64, device=dev) for _ in range(4)]
    st = _timed(torch, lambda: L.check(lib.fcpp_dubins_sample(ctx.handle, n, P(f[0]), P(f[1]), P(f[2]), R, P(word), P(seg), args.spacing, P(off), m,
                                                              *[P(o) for o in outs], HP(off_h))), args.reps, args.warmup)
    rec['sample']['dubins'] = {'samples': m, 'time': st, 'samples_per_s': m / (st['median_ms'] * 1e-3), 'bytes_written_per_s': 32.0 * m / (st['median_ms'] * 1e-3)}

    line = json.dumps(rec)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
