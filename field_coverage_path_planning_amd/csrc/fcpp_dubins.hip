// fcpp_dubins.hip -- gfx950 (MI355X) kernels of the Dubins connectors: fcpp_dubins_solve (a lane per pair), fcpp_dubins_matrix (all pairs
// of two pose lists: the transit matrix the GA takes) and fcpp_dubins_counts / fcpp_dubins_sample (solved paths at a fixed spacing).
// The mathematics is ONE host+device function, fcpp_dubinsfn.h; float64, -ffp-contract=off like every other translation unit, so the
// kernels give the bits fcpp_debug_dubins gives on the host.
//
// k_dubins_matrix is the hot one: 8 B (+ 1 B of word) written per pair against several hundred fp64 operations -- six closed forms with an
// atan2 (one division, a degree-11 polynomial) each, six square roots, twelve angle reductions -- so it is bound by fp64 vector issue, not by
// memory.  A workgroup takes DUB_ROWS "from" poses x DUB_COLS "to" poses.  What depends on one pose only (sine and cosine of its heading,
// times R) is computed once per pose and tile: a lane keeps its "to" pose in registers for the whole tile, the tile's "from" poses lie
// in LDS and every lane of the workgroup reads the same one at a time (one address: a broadcast, no bank conflict).  Lanes run along the
// row of D, so a wavefront writes 512 consecutive bytes.  All six words are evaluated and the shortest selected: no divergence by word.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_dubins.h"
#include "fcpp_dubinsfn.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int DBLOCK = 256;
static_assert(DUB_COLS == DBLOCK && DUB_ROWS <= DBLOCK, "a lane per column; the first DUB_ROWS lanes prepare the rows");

#define DUB_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

__global__ __launch_bounds__(DBLOCK) void k_dubins_solve(int64_t n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                         const double *__restrict__ fh, const double *__restrict__ tx,
                                                         const double *__restrict__ ty, const double *__restrict__ th, double R,
                                                         int32_t *__restrict__ word, double *__restrict__ seg, double *__restrict__ len)
{
    const int64_t i = (int64_t)blockIdx.x * DBLOCK + threadIdx.x;
    if (i >= n) return;
    int w;
    double s0, s1, s2, tot;
    dubins_solve(fx[i], fy[i], fh[i], tx[i], ty[i], th[i], R, w, s0, s1, s2, tot);
    if (word) word[i] = w;
    if (seg) { seg[3 * i] = s0; seg[3 * i + 1] = s1; seg[3 * i + 2] = s2; }
    if (len) len[i] = tot;
}

__global__ __launch_bounds__(DBLOCK) void k_dubins_matrix(int64_t n_from, const double *__restrict__ fx, const double *__restrict__ fy,
                                                          const double *__restrict__ fh, int64_t n_to, const double *__restrict__ tx,
                                                          const double *__restrict__ ty, const double *__restrict__ th, double R,
                                                          double *__restrict__ D, int8_t *__restrict__ word)
{
    __shared__ DubinsPose rows[DUB_ROWS];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * DUB_ROWS, j = (int64_t)blockIdx.x * DUB_COLS + tid;
    if (tid < DUB_ROWS && i0 + tid < n_from) rows[tid] = dubins_prep(fx[i0 + tid], fy[i0 + tid], fh[i0 + tid], R);
    DubinsPose to = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (j < n_to) to = dubins_prep(tx[j], ty[j], th[j], R);
    __syncthreads();
    if (j >= n_to) return;
    const int n_rows = (int)(n_from - i0 < DUB_ROWS ? n_from - i0 : DUB_ROWS);
#pragma unroll 1
    for (int r = 0; r < n_rows; ++r) {
        const DubinsPose f = rows[r];
        int w;
        double s0, s1, s2, tot;
        dubins_solve_prepped(f, to, R, w, s0, s1, s2, tot);
        const int64_t at = (i0 + r) * n_to + j;
        if (D) D[at] = tot;
        if (word) word[at] = (int8_t)w;
    }
}

// The sample counts and offsets: k_sample_counts (fcpp_samplefn.h) over the paths' lengths; the last sample lies AT the path's end, a
// NaN path has one sample.
struct DubinsLength { const double *len; __device__ double operator()(int64_t p) const { return len[p]; } };

// A lane per output sample: its path by bisection of out_offsets, then dubins_pose_at from the start of the segment that holds
// s = k * spacing (one multiplication, never accumulated); the last sample of a path lies AT its total.  32 B written per sample.
__global__ __launch_bounds__(DBLOCK) void k_dubins_sample(int64_t n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                          const double *__restrict__ fh, double R, const int32_t *__restrict__ word,
                                                          const double *__restrict__ seg, double spacing,
                                                          const int64_t *__restrict__ out_offsets, int64_t total_samples,
                                                          double *__restrict__ xs, double *__restrict__ ys, double *__restrict__ hs,
                                                          double *__restrict__ kappas)
{
    const int64_t q = (int64_t)blockIdx.x * DBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t p, k, K;
    sample_path(out_offsets, n, q, p, k, K);
    const double s0 = seg[3 * p], s1 = seg[3 * p + 1], s2 = seg[3 * p + 2], total = (s0 + s1) + s2;
    double s = (double)k * spacing;
    if (k == K - 1 || s > total) s = total;             // (K - 1) * spacing <= total: the last sample is the path's end either way
    double x, y, h, kap;
    dubins_pose_at(fx[p], fy[p], fh[p], R, word[p], s0, s1, s2, s, x, y, h, kap);
    if (xs) xs[q] = x;
    if (ys) ys[q] = y;
    if (hs) hs[q] = h;
    if (kappas) kappas[q] = kap;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_dubins_solve(hipStream_t st, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
                        const double *th, double R, int32_t *word, double *seg, double *len)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_dubins_solve, dim3((unsigned)((n + DBLOCK - 1) / DBLOCK)), dim3(DBLOCK), 0, st, n, fx, fy, fh, tx, ty, th, R, word, seg, len);
    DUB_LAUNCH_CHECK();
    return 0;
}

int launch_dubins_matrix(hipStream_t st, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to, const double *tx,
                         const double *ty, const double *th, double R, double *D, int8_t *word)
{
    if (n_from <= 0 || n_to <= 0) return 0;
    const dim3 grid((unsigned)((n_to + DUB_COLS - 1) / DUB_COLS), (unsigned)((n_from + DUB_ROWS - 1) / DUB_ROWS));
    hipLaunchKernelGGL(k_dubins_matrix, grid, dim3(DBLOCK), 0, st, n_from, fx, fy, fh, n_to, tx, ty, th, R, D, word);
    DUB_LAUNCH_CHECK();
    return 0;
}

int launch_dubins_counts(hipStream_t st, int64_t n, const double *len, double spacing, int64_t *out_offsets, int64_t *err)
{
    hipLaunchKernelGGL((k_sample_counts<DBLOCK, DubinsLength>), dim3(1), dim3(DBLOCK), 0, st, n, DubinsLength{ len }, spacing, 1, 1, out_offsets, err);
    DUB_LAUNCH_CHECK();
    return 0;
}

int launch_dubins_sample(hipStream_t st, int64_t n, const double *fx, const double *fy, const double *fh, double R, const int32_t *word,
                         const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                         double *kappas)
{
    if (total_samples <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(k_dubins_sample, dim3((unsigned)((total_samples + DBLOCK - 1) / DBLOCK)), dim3(DBLOCK), 0, st, n, fx, fy, fh, R, word, seg,
                       spacing, out_offsets, total_samples, xs, ys, hs, kappas);
    DUB_LAUNCH_CHECK();
    return 0;
}

}  // namespace fcpp
