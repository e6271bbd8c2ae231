// fcpp_traj.hip -- gfx950 (MI355X) kernels of the trajectory output: per point of every path its arc length s, its time stamp t and the
// heading of the vehicle (fcpp_trajectory), and the same trajectory sampled at a fixed time step (fcpp_trajectory_sample).
//
// s and t are the running values of _calculate_path_length / _calculate_work_time (MLP:1290-1311): segmented inclusive scans of
//     d_i = sqrt((x_i - x_(i-1))^2 + (y_i - y_(i-1))^2),     tau_i = d_i / max(((v_(i-1) + v_i) / 2) / 3.6, 0.1)
// -- the expressions of k_validate, term for term.  The heading is the chord direction of the step that leaves the point; a zero step
// takes the direction of the nearest earlier non-zero step: the running MAXIMUM of "index at which a non-zero step starts", an integer
// scan that runs beside the two sums; atan2 is evaluated once per point, on the step the scan names.
//
// Shape: tiles -> blocks -> paths -> apply, like the speed planner's min-plus scan (fcpp_kernels.hip), with two differences.
//   * A sum does not reset itself at a path's first point, so the spine is segmented, and it is ANCHORED AT THE PATH: a block is up to
//     TRAJ_BLOCK_TILES consecutive tiles of one path counted from the path's first tile.  The order of the additions then depends on
//     the path alone: the same path gives the same bits alone or as path 4711 of a batch.
//   * Every level adds "what entered the group" to "the value inside the group", and what enters a group is the VALUE AT THE END of
//     the group before it (chains across waves, tiles and blocks; inside a wave the scan that adds the first half's last value to the
//     second half, level by level).  Rounding is monotone and all terms are >= 0, so s and t never decrease along a path -- a scan
//     whose elements are summed in unrelated orders (Hillis-Steele, a carry taken from another tree) can step back by an ulp at a
//     duplicate point.  A point's value is   cin[block] + (pre[tile] + (wave base + value inside the wave)).
//
// Traffic per point: pass 1 reads x, y, v (24 B), the apply pass reads them again (+ 4 B flag word) and writes s, t, heading (24 B);
// the spine moves 64 B per TILE.  No atomics; float64; -ffp-contract=off like every other translation unit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_samplefn.h"
#include "fcpp_traj.h"

namespace fcpp {

static constexpr int TBLOCK = 256, TNWAVE = TBLOCK / 64;
static_assert(TILE_POINTS == 2 * TBLOCK, "two consecutive points per thread");
static constexpr double TRAJ_PI = 3.14159265358979323846;

// one thread's two consecutive points j0 = 2 * tid, j0 + 1 of a tile, after the tile-local scan
struct TrajLane {
    double s0, s1, t0, t1;      // running sums at the two points, relative to the tile's first point
    double dx0, dy0, dx1, dy1;  // the steps that leave the two points (valid where ok0 / ok1)
    int l0, l1;                 // tile-local index of the last non-zero step that starts at or before the point; -1: none in the tile so far
    bool ok0, ok1;              // the point has a non-zero outgoing step
    bool in0, in1;              // the point belongs to the tile
};
struct TrajShared { double s[TNWAVE], t[TNWAVE]; int l[TNWAVE], f[TNWAVE]; };

// The tile-local scan.  tot = the values at the tile's last point: (sum of d, sum of tau, last / first non-zero step as tile-local
// indices, -1 / TILE_POINTS: none).  Neighbouring points come from the neighbouring lanes; only a wavefront's first and last lane
// (and the tile's last point) load their halo themselves.
__device__ __forceinline__ void traj_tile_scan(TrajShared &S, const DevTile &t, const DevPath &p, const double *__restrict__ x,
                                               const double *__restrict__ y, const double *__restrict__ v, TrajLane &r, double &tot_s,
                                               double &tot_t, int &tot_l, int &tot_f)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j0 = 2 * tid;
    const int64_t i0 = t.start + j0, g0 = p.off + i0;
    r.in0 = j0 < t.count; r.in1 = j0 + 1 < t.count;
    const bool have1 = r.in0 && i0 + 1 < p.n;                   // the point after j0 exists (in this tile or as its halo)
    double x0 = 0, y0 = 0, v0 = 0, x1 = 0, y1 = 0, v1 = 0;
    if (r.in0) { x0 = x[g0]; y0 = y[g0]; v0 = v[g0]; }
    if (have1) { x1 = x[g0 + 1]; y1 = y[g0 + 1]; v1 = v[g0 + 1]; }
    // the point before j0: the neighbouring lane's second point
    double xp = __shfl_up(x1, 1), yp = __shfl_up(y1, 1), vp = __shfl_up(v1, 1);
    const bool havep = r.in0 && i0 > 0;
    if (lane == 0 && havep) { xp = x[g0 - 1]; yp = y[g0 - 1]; vp = v[g0 - 1]; }
    // the point after j0 + 1: the neighbouring lane's first point
    double xn = __shfl_down(x0, 1), yn = __shfl_down(y0, 1);
    const bool have2 = r.in1 && i0 + 2 < p.n;
    if (have2 && (lane == 63 || j0 + 2 >= t.count)) { xn = x[g0 + 2]; yn = y[g0 + 2]; }
    // the two incoming steps (MLP:1294-1296, 1303-1310)
    double d0 = 0, tau0 = 0, d1 = 0, tau1 = 0;
    if (havep) {
        const double dx = x0 - xp, dy = y0 - yp;
        d0 = sqrt(dx * dx + dy * dy);
        const double ms = ((vp + v0) / 2) / 3.6;
        tau0 = d0 / fmax(ms, 0.1);
    }
    r.dx0 = x1 - x0; r.dy0 = y1 - y0;
    if (r.in1) {
        d1 = sqrt(r.dx0 * r.dx0 + r.dy0 * r.dy0);
        const double ms = ((v0 + v1) / 2) / 3.6;
        tau1 = d1 / fmax(ms, 0.1);
    }
    r.dx1 = xn - x1; r.dy1 = yn - y1;
    r.ok0 = have1 && (r.dx0 != 0.0 || r.dy0 != 0.0);
    r.ok1 = have2 && (r.dx1 != 0.0 || r.dy1 != 0.0);
    // inside the thread, then across the wavefront: level k adds the last value of the first half of every group of 2 << k lanes to its second half
    r.s0 = d0; r.s1 = d0 + d1; r.t0 = tau0; r.t1 = tau0 + tau1;
    r.l0 = r.ok0 ? j0 : -1; r.l1 = r.ok1 ? j0 + 1 : r.l0;
    int f = r.ok0 ? j0 : (r.ok1 ? j0 + 1 : TILE_POINTS);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int src = (lane & ~((2 << k) - 1)) | ((1 << k) - 1);
        const double bs = __shfl(r.s1, src), bt = __shfl(r.t1, src);
        const int bl = __shfl(r.l1, src);
        if (lane & (1 << k)) {
            r.s0 = bs + r.s0; r.s1 = bs + r.s1; r.t0 = bt + r.t0; r.t1 = bt + r.t1;
            r.l0 = max(bl, r.l0); r.l1 = max(bl, r.l1);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f = min(f, __shfl_xor(f, o));
    if (lane == 63) { S.s[wave] = r.s1; S.t[wave] = r.t1; S.l[wave] = r.l1; }
    if (lane == 0) S.f[wave] = f;
    __syncthreads();
    // across the wavefronts: a chain -- what enters wave w + 1 is the value at the end of wave w
    double bs = 0, bt = 0;
    int bl = -1;
    tot_s = 0; tot_t = 0; tot_l = -1; tot_f = TILE_POINTS;
#pragma unroll
    for (int w = 0; w < TNWAVE; ++w) {
        if (w == wave) { bs = tot_s; bt = tot_t; bl = tot_l; }
        tot_s = tot_s + S.s[w]; tot_t = tot_t + S.t[w];
        tot_l = max(tot_l, S.l[w]); tot_f = min(tot_f, S.f[w]);
    }
    r.s0 = bs + r.s0; r.s1 = bs + r.s1; r.t0 = bt + r.t0; r.t1 = bt + r.t1;
    r.l0 = max(bl, r.l0); r.l1 = max(bl, r.l1);
}

__global__ __launch_bounds__(TBLOCK) void k_traj_tiles(const DevTile *__restrict__ tiles, const DevPath *__restrict__ paths,
                                                       const double *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ v, TrajAgg *__restrict__ agg)
{
    __shared__ TrajShared S;
    const DevTile t = tiles[blockIdx.x];
    const DevPath p = paths[t.field];
    TrajLane r;
    double ts, tt;
    int tl, tf;
    traj_tile_scan(S, t, p, x, y, v, r, ts, tt, tl, tf);
    if (threadIdx.x == 0) {
        const int64_t g = p.off + t.start;
        TrajAgg a;
        a.s = ts; a.t = tt; a.last = tl >= 0 ? g + tl : -1; a.first = tf < TILE_POINTS ? g + tf : INT64_MAX;
        agg[blockIdx.x] = a;
    }
}

// One wavefront per block: the tiles' sums are loaded side by side, lane 0 walks the chain (what enters tile k + 1 is the value at the
// end of tile k -- TRAJ_BLOCK_TILES dependent additions, a few microseconds, beside 1.5 KiB of HBM traffic per tile in the two other
// passes), and the entering values are written side by side again.
__global__ __launch_bounds__(64) void k_traj_blocks(const TrajBlock *__restrict__ blocks, const TrajAgg *__restrict__ agg,
                                                    TrajAgg *__restrict__ pre, TrajAgg *__restrict__ blk)
{
    __shared__ TrajAgg sh[TRAJ_BLOCK_TILES];
    const TrajBlock b = blocks[blockIdx.x];
    const int lane = threadIdx.x;
    for (int k = lane; k < b.count; k += 64) sh[k] = agg[b.tile0 + k];
    __syncthreads();
    if (lane == 0) {
        TrajAgg run = { 0.0, 0.0, -1, INT64_MAX };
        for (int k = 0; k < b.count; ++k) {
            const TrajAgg a = sh[k];
            sh[k] = run;
            run.s = run.s + a.s; run.t = run.t + a.t;
            run.last = a.last > run.last ? a.last : run.last;
            run.first = a.first < run.first ? a.first : run.first;
        }
        blk[blockIdx.x] = run;
    }
    __syncthreads();
    for (int k = lane; k < b.count; k += 64) pre[b.tile0 + k] = sh[k];
}

// One wavefront per path: the chain across the path's blocks, 64 blocks loaded at a time.
__global__ __launch_bounds__(64) void k_traj_paths(int64_t n_paths, const int64_t *__restrict__ block_first, const TrajAgg *__restrict__ blk,
                                                   TrajAgg *__restrict__ cin, int64_t *__restrict__ path_first, double *__restrict__ totals)
{
    __shared__ TrajAgg sh[64];
    __shared__ TrajAgg run_sh;
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t b0 = block_first[p], nb = block_first[p + 1] - b0;
    if (lane == 0) run_sh = { 0.0, 0.0, -1, INT64_MAX };
    for (int64_t base = 0; base < nb; base += 64) {
        const int cnt = (int)(nb - base < 64 ? nb - base : 64);
        if (lane < cnt) sh[lane] = blk[b0 + base + lane];
        __syncthreads();
        if (lane == 0) {
            TrajAgg run = run_sh;
            for (int k = 0; k < cnt; ++k) {
                const TrajAgg a = sh[k];
                sh[k] = run;
                run.s = run.s + a.s; run.t = run.t + a.t;
                run.last = a.last > run.last ? a.last : run.last;
                run.first = a.first < run.first ? a.first : run.first;
            }
            run_sh = run;
        }
        __syncthreads();
        if (lane < cnt) cin[b0 + base + lane] = sh[lane];
        __syncthreads();
    }
    __syncthreads();
    if (lane == 0) {
        const TrajAgg run = run_sh;
        path_first[p] = run.first;
        if (totals) { totals[2 * p] = run.s; totals[2 * p + 1] = run.t; }
    }
}

// heading of a point: the chord direction, turned by pi and wrapped into (-pi, pi] where the point is driven backwards
__device__ __forceinline__ double traj_heading(double dx, double dy, bool reverse)
{
    double h = atan2(dy, dx);
    if (reverse) h = h > 0.0 ? h - TRAJ_PI : h + TRAJ_PI;
    return h;
}

__global__ __launch_bounds__(TBLOCK) void k_traj_apply(const DevTile *__restrict__ tiles, const DevPath *__restrict__ paths,
                                                       const int64_t *__restrict__ tile_first, const int64_t *__restrict__ block_first,
                                                       const double *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ v, const uint32_t *__restrict__ fs,
                                                       const TrajAgg *__restrict__ pre, const TrajAgg *__restrict__ cin,
                                                       const int64_t *__restrict__ path_first, double *__restrict__ s_out,
                                                       double *__restrict__ t_out, double *__restrict__ h_out)
{
    __shared__ TrajShared S;
    const DevTile t = tiles[blockIdx.x];
    const DevPath p = paths[t.field];
    TrajLane r;
    double ts, tt;
    int tl, tf;
    traj_tile_scan(S, t, p, x, y, v, r, ts, tt, tl, tf);
    const TrajAgg e = pre[blockIdx.x];
    const TrajAgg c = cin[block_first[t.field] + ((int64_t)blockIdx.x - tile_first[t.field]) / TRAJ_BLOCK_TILES];
    const int64_t g_tile = p.off + t.start, g0 = g_tile + 2 * threadIdx.x;
    if (s_out) {
        if (r.in0) s_out[g0] = c.s + (e.s + r.s0);
        if (r.in1) s_out[g0 + 1] = c.s + (e.s + r.s1);
    }
    if (t_out) {
        if (r.in0) t_out[g0] = c.t + (e.t + r.t0);
        if (r.in1) t_out[g0 + 1] = c.t + (e.t + r.t1);
    }
    if (h_out) {
        // the step whose direction the point takes: the last non-zero one at or before it -- in this tile, in the tiles before it, or
        // (leading zero steps) the path's first non-zero step; none at all: heading 0
        const int64_t before = c.last > e.last ? c.last : e.last, lead = path_first[t.field];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!(k ? r.in1 : r.in0)) continue;
            const int64_t g = g0 + k;
            const int l = k ? r.l1 : r.l0;
            int64_t at = l >= 0 ? g_tile + l : before;
            if (at < 0) at = lead;
            double dx = k ? r.dx1 : r.dx0, dy = k ? r.dy1 : r.dy0, h = 0.0;
            if (at != INT64_MAX) {
                if (at != g) { dx = x[at + 1] - x[at]; dy = y[at + 1] - y[at]; }
                h = traj_heading(dx, dy, fs && (fs[g] & FCPP_KIND_MASK) == (uint32_t)FCPP_KIND_REVERSE);
            }
            h_out[g] = h;
        }
    }
}

// ---- fixed-rate sampling ----------------------------------------------------------------------------------------------------------
// The sample counts and offsets: k_sample_counts (fcpp_samplefn.h) over the paths' total times, one more sample AT T_p with include_end.
struct TrajTime { const double *totals; __device__ double operator()(int64_t p) const { return totals[2 * p + 1]; } };   // (length, time) per path

// A lane per output sample: its path by bisection of out_offsets, its step by bisection of the path's t (non-decreasing by
// construction): the LAST i with t_i <= T.  Neighbouring lanes land in the same or adjacent steps, so the last levels of the search
// hit the cache; the kernel is bounded by its 44-52 B per sample of output.
// x, y and s are interpolated linearly with lambda = (T - t_i) / (t_(i+1) - t_i), and so is v: LINEAR IN TIME, the constant
// acceleration over a step that the speed planner's sweeps assume (v^2 linear in distance).  Heading and flag word are those of
// point i.  T >= T_p -- and, with include_end, the last sample of a path -- is the path's last point, bit for bit.
__global__ __launch_bounds__(TBLOCK) void k_traj_sample(int64_t n_paths, const int64_t *__restrict__ offsets,
                                                        const int64_t *__restrict__ out_offsets, int64_t total_samples,
                                                        const double *__restrict__ x, const double *__restrict__ y,
                                                        const double *__restrict__ v, const double *__restrict__ s,
                                                        const double *__restrict__ t, const double *__restrict__ heading,
                                                        const uint32_t *__restrict__ fs, double dt, int include_end,
                                                        double *__restrict__ xs, double *__restrict__ ys, double *__restrict__ vs,
                                                        double *__restrict__ ss, double *__restrict__ hs, uint32_t *__restrict__ fss,
                                                        int64_t *__restrict__ src)
{
    const int64_t q = (int64_t)blockIdx.x * TBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t p, k, K;
    sample_path(out_offsets, n_paths, q, p, k, K);
    const int64_t a = offsets[p], n = offsets[p + 1] - a;
    if (n <= 0) {                                       // a path without points has no trajectory: its sample says so
        const double nan = __builtin_nan("");
        if (xs) xs[q] = nan;
        if (ys) ys[q] = nan;
        if (vs) vs[q] = nan;
        if (ss) ss[q] = nan;
        if (hs) hs[q] = nan;
        if (fss) fss[q] = 0u;
        if (src) src[q] = -1;
        return;
    }
    const double T = (double)k * dt;
    int64_t i = n - 1;
    if (!(include_end && k == K - 1)) {
        int64_t l = 0, h = n;                           // t[a] = 0 <= T
        while (h - l > 1) {
            const int64_t mid = l + (h - l) / 2;
            if (t[a + mid] <= T) l = mid; else h = mid;
        }
        i = l;
    }
    const int64_t g = a + i;
    double lam = 0.0;
    const bool inner = i < n - 1;
    if (inner) lam = (T - t[g]) / (t[g + 1] - t[g]);
    if (xs) xs[q] = inner ? x[g] + lam * (x[g + 1] - x[g]) : x[g];
    if (ys) ys[q] = inner ? y[g] + lam * (y[g + 1] - y[g]) : y[g];
    if (vs) vs[q] = inner ? v[g] + lam * (v[g + 1] - v[g]) : v[g];
    if (ss) ss[q] = inner ? fmin(s[g] + lam * (s[g + 1] - s[g]), s[g + 1]) : s[g];
    if (hs) hs[q] = heading[g];
    if (fss) fss[q] = fs ? fs[g] : 0u;
    if (src) src[q] = g;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_traj_tiles(hipStream_t st, int64_t n_tiles, const DevTile *tiles, const DevPath *paths, const double *x, const double *y,
                      const double *v, TrajAgg *agg)
{
    if (n_tiles <= 0) return 0;
    return launch(st, k_traj_tiles, (unsigned)n_tiles, TBLOCK, tiles, paths, x, y, v, agg);
}

int launch_traj_blocks(hipStream_t st, int64_t n_blocks, const TrajBlock *blocks, const TrajAgg *agg, TrajAgg *pre, TrajAgg *blk)
{
    if (n_blocks <= 0) return 0;
    return launch(st, k_traj_blocks, (unsigned)n_blocks, 64, blocks, agg, pre, blk);
}

int launch_traj_paths(hipStream_t st, int64_t n_paths, const int64_t *block_first, const TrajAgg *blk, TrajAgg *cin, int64_t *path_first,
                      double *totals)
{
    if (n_paths <= 0) return 0;
    return launch(st, k_traj_paths, (unsigned)n_paths, 64, n_paths, block_first, blk, cin, path_first, totals);
}

int launch_traj_apply(hipStream_t st, int64_t n_tiles, const DevTile *tiles, const DevPath *paths, const int64_t *tile_first,
                      const int64_t *block_first, const double *x, const double *y, const double *v, const uint32_t *fs, const TrajAgg *pre,
                      const TrajAgg *cin, const int64_t *path_first, double *s, double *t, double *heading)
{
    if (n_tiles <= 0) return 0;
    return launch(st, k_traj_apply, (unsigned)n_tiles, TBLOCK, tiles, paths, tile_first, block_first, x, y, v, fs, pre, cin, path_first, s, t,
                  heading);
}

int launch_traj_counts(hipStream_t st, int64_t n_paths, const double *totals, double dt, int include_end, int64_t *out_offsets, int64_t *err)
{
    return launch_sample_counts<TBLOCK>(st, n_paths, TrajTime{ totals }, dt, include_end, 0, out_offsets, err);
}

int launch_traj_sample(hipStream_t st, int64_t n_paths, const int64_t *offsets, const int64_t *out_offsets, int64_t total_samples, const double *x,
                       const double *y, const double *v, const double *s, const double *t, const double *heading, const uint32_t *fs, double dt,
                       int include_end, double *xs, double *ys, double *vs, double *ss, double *hs, uint32_t *fss, int64_t *src)
{
    if (total_samples <= 0 || n_paths <= 0) return 0;
    return launch(st, k_traj_sample, blocks_for(total_samples, TBLOCK), TBLOCK, n_paths, offsets, out_offsets, total_samples, x, y, v, s, t, heading, fs,
                  dt, include_end, xs, ys, vs, ss, hs, fss, src);
}

}  // namespace fcpp
