// fcpp_rs.hip -- gfx950 (MI355X) kernels of the Reeds-Shepp connectors: fcpp_rs_solve (a lane per pair), fcpp_rs_matrix (all pairs of two
// pose lists: the transit matrix of a vehicle that reverses) and fcpp_rs_counts / fcpp_rs_sample (solved paths at a fixed spacing, run by
// run of one gear).  The mathematics is ONE host+device function, fcpp_rsfn.h; float64, -ffp-contract=off like every other translation
// unit, so the kernels give the bits fcpp_debug_rs gives on the host.
//
// k_rs_matrix is the hot one and has k_dubins_matrix's shape: 8 B (+ 1 B of word) written per pair against 22 atan2, 26 square roots and
// some 90 angle reductions -- 48 words from eight polar forms -- so it is bound by fp64 vector issue.  A workgroup takes RS_ROWS "from" poses
// x RS_COLS "to" poses.  What depends on one pose only is the sine and cosine of the FROM heading (the rotation into the start frame),
// computed once per pose and tile into LDS, where every lane reads the same pose at a time (a broadcast); of its "to" pose a lane keeps x, y
// and h in registers for the whole tile (rs_prep's sine and cosine of it are unused there and eliminated).  sin and cos of phi = h_1 - h_0
// are taken of the difference itself, per pair (35 of the pair's 4600 instructions), so that equal headings give exactly 0 and 1.
// Lanes run along the row of D, so a wavefront writes 512 consecutive bytes.  All words are evaluated and the shortest selected: no
// divergence by word; the five segment lengths the matrix does not store are dead code there.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_rs.h"
#include "fcpp_rsfn.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int RBLOCK = 256;
static_assert(RS_COLS == RBLOCK && RS_ROWS <= RBLOCK, "a lane per column; the first RS_ROWS lanes prepare the rows");

#define RS_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

__global__ __launch_bounds__(RBLOCK) void k_rs_solve(int64_t n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                     const double *__restrict__ fh, const double *__restrict__ tx,
                                                     const double *__restrict__ ty, const double *__restrict__ th, double R,
                                                     int32_t *__restrict__ word, double *__restrict__ seg, double *__restrict__ len)
{
    const int64_t i = (int64_t)blockIdx.x * RBLOCK + threadIdx.x;
    if (i >= n) return;
    int w;
    double s[5], tot;
    rs_solve(fx[i], fy[i], fh[i], tx[i], ty[i], th[i], R, w, s, tot);
    if (word) word[i] = w;
    if (seg) { seg[5 * i] = s[0]; seg[5 * i + 1] = s[1]; seg[5 * i + 2] = s[2]; seg[5 * i + 3] = s[3]; seg[5 * i + 4] = s[4]; }
    if (len) len[i] = tot;
}

__global__ __launch_bounds__(RBLOCK) void k_rs_matrix(int64_t n_from, const double *__restrict__ fx, const double *__restrict__ fy,
                                                      const double *__restrict__ fh, int64_t n_to, const double *__restrict__ tx,
                                                      const double *__restrict__ ty, const double *__restrict__ th, double R,
                                                      double *__restrict__ D, int8_t *__restrict__ word)
{
    __shared__ RsPose rows[RS_ROWS];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * RS_ROWS, j = (int64_t)blockIdx.x * RS_COLS + tid;
    if (tid < RS_ROWS && i0 + tid < n_from) rows[tid] = rs_prep(fx[i0 + tid], fy[i0 + tid], fh[i0 + tid]);
    RsPose to = { 0.0, 0.0, 0.0, 0.0, 1.0 };
    if (j < n_to) to = rs_prep(tx[j], ty[j], th[j]);
    __syncthreads();
    if (j >= n_to) return;
    const int n_rows = (int)(n_from - i0 < RS_ROWS ? n_from - i0 : RS_ROWS);
#pragma unroll 1
    for (int r = 0; r < n_rows; ++r) {
        const RsPose f = rows[r];
        int w;
        double s[5], tot;
        rs_solve_prepped(f, to, R, w, s, tot);
        const int64_t at = (i0 + r) * n_to + j;
        if (D) D[at] = tot;
        if (word) word[at] = (int8_t)w;
    }
}

// The count of a path: its gear runs (rs_runs), each by the count rule with its end; a NaN path (word -1) has one sample.
struct RsCount {
    const int32_t *word;
    const double *seg;
    double spacing;
    __device__ int64_t operator()(int64_t p, int64_t &bad) const
    {
        double s[5];
        for (int k = 0; k < 5; ++k) s[k] = seg[5 * p + k];
        const int w = word[p];
        if (w < 0 || w >= RS_WORDS || s[0] != s[0] || s[1] != s[1] || s[2] != s[2] || s[3] != s[3] || s[4] != s[4]) return 1;
        const RsRuns runs = rs_runs(w, s);
        return sample_count_runs(runs.len, runs.n, spacing, bad);
    }
};

// A lane per output sample: its path by bisection of out_offsets, its run by the runs' counts, then the pose from the start of the segment
// that holds e = k * spacing within the run (one multiplication, never accumulated); the last sample of a run lies AT its end, which is
// the first sample of the next run: a cusp is two samples with one pose and opposite gears.  33 B written per sample.
__global__ __launch_bounds__(RBLOCK) void k_rs_sample(int64_t n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                      const double *__restrict__ fh, double R, const int32_t *__restrict__ word,
                                                      const double *__restrict__ seg, double spacing, const int64_t *__restrict__ out_offsets,
                                                      int64_t total_samples, double *__restrict__ xs, double *__restrict__ ys,
                                                      double *__restrict__ hs, double *__restrict__ kappas, int8_t *__restrict__ gears)
{
    const int64_t q = (int64_t)blockIdx.x * RBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t p, k, K;
    sample_path(out_offsets, n, q, p, k, K);
    double s[5];
    for (int j = 0; j < 5; ++j) s[j] = seg[5 * p + j];
    const int w = word[p];
    double x, y, h, kap;
    int gear = 0;
    x = y = h = kap = __builtin_nan("");
    if (w >= 0 && w < RS_WORDS && s[0] == s[0] && s[1] == s[1] && s[2] == s[2] && s[3] == s[3] && s[4] == s[4]) {
        const RsRuns runs = rs_runs(w, s);
        int r = 0;
        int64_t Kr = 0, bad = 0;
        for (; r < runs.n; ++r) {
            Kr = sample_count(runs.len[r], spacing, true, false, bad);
            if (k < Kr || r == runs.n - 1) break;
            k -= Kr;
        }
        double e = (double)k * spacing;
        if (k >= Kr - 1 || e > runs.len[r]) e = runs.len[r];        // (Kr - 1) * spacing <= the run's length: its last sample is its end
        rs_pose_in_run(fx[p], fy[p], fh[p], R, w, s, runs, r, e, x, y, h, kap, gear);
    }
    if (xs) xs[q] = x;
    if (ys) ys[q] = y;
    if (hs) hs[q] = h;
    if (kappas) kappas[q] = kap;
    if (gears) gears[q] = (int8_t)gear;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_rs_solve(hipStream_t st, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
                    const double *th, double R, int32_t *word, double *seg, double *len)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_rs_solve, dim3((unsigned)((n + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, st, n, fx, fy, fh, tx, ty, th, R, word, seg, len);
    RS_LAUNCH_CHECK();
    return 0;
}

int launch_rs_matrix(hipStream_t st, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to, const double *tx,
                     const double *ty, const double *th, double R, double *D, int8_t *word)
{
    if (n_from <= 0 || n_to <= 0) return 0;
    const dim3 grid((unsigned)((n_to + RS_COLS - 1) / RS_COLS), (unsigned)((n_from + RS_ROWS - 1) / RS_ROWS));
    hipLaunchKernelGGL(k_rs_matrix, grid, dim3(RBLOCK), 0, st, n_from, fx, fy, fh, n_to, tx, ty, th, R, D, word);
    RS_LAUNCH_CHECK();
    return 0;
}

int launch_rs_counts(hipStream_t st, int64_t n, const int32_t *word, const double *seg, double spacing, int64_t *out_offsets, int64_t *err)
{
    hipLaunchKernelGGL((k_path_counts<RBLOCK, RsCount>), dim3(1), dim3(RBLOCK), 0, st, n, RsCount{ word, seg, spacing }, out_offsets, err);
    RS_LAUNCH_CHECK();
    return 0;
}

int launch_rs_sample(hipStream_t st, int64_t n, const double *fx, const double *fy, const double *fh, double R, const int32_t *word,
                     const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                     double *kappas, int8_t *gears)
{
    if (total_samples <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(k_rs_sample, dim3((unsigned)((total_samples + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, st, n, fx, fy, fh, R, word, seg,
                       spacing, out_offsets, total_samples, xs, ys, hs, kappas, gears);
    RS_LAUNCH_CHECK();
    return 0;
}

}  // namespace fcpp
