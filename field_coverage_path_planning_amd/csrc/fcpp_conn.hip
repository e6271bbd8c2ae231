// fcpp_conn.hip -- gfx950 (MI355X) kernels of the connectors, Dubins (MODE 0) and Reeds-Shepp (MODE 1) from one set of templates over
// Conn<MODE> (fcpp_connfn.h): fcpp_*_solve (a lane per pair), fcpp_*_matrix (all pairs of two pose lists: the transit matrix the GA takes)
// and fcpp_*_counts / fcpp_*_sample (solved paths at a fixed spacing; Reeds-Shepp run by run of one gear).  The mathematics is ONE
// host+device function per family, fcpp_dubinsfn.h / fcpp_rsfn.h; float64, -ffp-contract=off like every other translation unit, so the
// kernels give the bits fcpp_debug_dubins / fcpp_debug_rs give on the host.
//
// k_conn_matrix is the hot one: 8 B (+ 1 B of word) written per pair against several hundred fp64 operations (Dubins: six closed forms with
// an atan2 -- one division, a degree-11 polynomial -- each, six square roots, twelve angle reductions), so it is bound by fp64 vector issue,
// not by memory.  A workgroup takes CONN_ROWS "from" poses x CONN_COLS "to" poses.  What depends on one pose only (Dubins: sine and cosine
// of its heading, times R) is computed once per pose and tile: a lane keeps its "to" pose in registers for the whole tile, the tile's
// "from" poses lie in LDS and every lane of the workgroup reads the same one at a time (one address: a broadcast, no bank conflict).
// Lanes run along the row of D, so a wavefront writes 512 consecutive bytes.  All words are evaluated and the shortest selected: no
// divergence by word.
// Reeds-Shepp: 22 atan2, 26 square roots and some 90 angle reductions per pair -- 48 words from eight polar forms.  What depends on one
// pose only is the sine and cosine of the FROM heading (the rotation into the start frame); of its "to" pose a lane keeps x, y and h
// (rs_prep's sine and cosine of it are unused there and eliminated).  sin and cos of phi = h_1 - h_0 are taken of the difference itself,
// per pair (35 of the pair's 4600 instructions), so that equal headings give exactly 0 and 1.  The five segment lengths the matrix does
// not store are dead code there.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_conn.h"
#include "fcpp_connfn.h"
#include "fcpp_launch.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int CBLOCK = 256;
static_assert(CONN_COLS == CBLOCK && CONN_ROWS <= CBLOCK, "a lane per column; the first CONN_ROWS lanes prepare the rows");

template <int MODE>
__global__ __launch_bounds__(CBLOCK) void k_conn_solve(int64_t n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                       const double *__restrict__ fh, const double *__restrict__ tx,
                                                       const double *__restrict__ ty, const double *__restrict__ th, double R,
                                                       int32_t *__restrict__ word, double *__restrict__ seg, double *__restrict__ len)
{
    using C = Conn<MODE>;
    const int64_t i = (int64_t)blockIdx.x * CBLOCK + threadIdx.x;
    if (i >= n) return;
    int w;
    double s[C::NSEG], tot;
    C::solve(fx[i], fy[i], fh[i], tx[i], ty[i], th[i], R, w, s, tot);
    if (word) word[i] = w;
    if (seg) for (int k = 0; k < C::NSEG; ++k) seg[C::NSEG * i + k] = s[k];
    if (len) len[i] = tot;
}

template <int MODE>
__global__ __launch_bounds__(CBLOCK) void k_conn_matrix(int64_t n_from, const double *__restrict__ fx, const double *__restrict__ fy,
                                                        const double *__restrict__ fh, int64_t n_to, const double *__restrict__ tx,
                                                        const double *__restrict__ ty, const double *__restrict__ th, double R,
                                                        double *__restrict__ D, int8_t *__restrict__ word)
{
    using C = Conn<MODE>;
    __shared__ typename C::Pose rows[CONN_ROWS];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * CONN_ROWS, j = (int64_t)blockIdx.x * CONN_COLS + tid;
    if (tid < CONN_ROWS && i0 + tid < n_from) rows[tid] = C::prep(fx[i0 + tid], fy[i0 + tid], fh[i0 + tid], R);
    typename C::Pose to = C::idle();
    if (j < n_to) to = C::prep(tx[j], ty[j], th[j], R);
    __syncthreads();
    if (j >= n_to) return;
    const int n_rows = (int)(n_from - i0 < CONN_ROWS ? n_from - i0 : CONN_ROWS);
#pragma unroll 1
    for (int r = 0; r < n_rows; ++r) {
        const typename C::Pose f = rows[r];
        int w;
        double s[C::NSEG], tot;
        C::solve_prepped(f, to, R, w, s, tot);
        const int64_t at = (i0 + r) * n_to + j;
        if (D) D[at] = tot;
        if (word) word[at] = (int8_t)w;
    }
}

// The Dubins sample counts and offsets: k_sample_counts (fcpp_samplefn.h) over the paths' lengths; a NaN path has one sample.
struct DubinsLength { const double *len; __device__ double operator()(int64_t p) const { return len[p]; } };

// The Reeds-Shepp ones: k_path_counts over Conn<1>::count of the paths' words and segments; a NaN path (word -1) has one sample.
struct RsCount {
    const int32_t *word;
    const double *seg;
    double spacing;
    __device__ int64_t operator()(int64_t p, int64_t &bad) const
    {
        double s[5];
        for (int k = 0; k < 5; ++k) s[k] = seg[5 * p + k];
        return Conn<1>::count(word[p], s, spacing, bad);
    }
};

// A lane per output sample: its path by bisection of out_offsets, then Conn<MODE>::eval.  32 B written per sample, 33 B with the gear.
template <int MODE>
__global__ __launch_bounds__(CBLOCK) void k_conn_sample(int64_t n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                        const double *__restrict__ fh, double R, const int32_t *__restrict__ word,
                                                        const double *__restrict__ seg, double spacing,
                                                        const int64_t *__restrict__ out_offsets, int64_t total_samples,
                                                        double *__restrict__ xs, double *__restrict__ ys, double *__restrict__ hs,
                                                        double *__restrict__ kappas, int8_t *__restrict__ gears)
{
    using C = Conn<MODE>;
    const int64_t q = (int64_t)blockIdx.x * CBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t p, k, K;
    sample_path(out_offsets, n, q, p, k, K);
    double s[C::NSEG];
    for (int j = 0; j < C::NSEG; ++j) s[j] = seg[C::NSEG * p + j];
    double x, y, h, kap;
    int gear;
    C::eval(fx[p], fy[p], fh[p], R, word[p], s, spacing, k, K, x, y, h, kap, gear);
    if (xs) xs[q] = x;
    if (ys) ys[q] = y;
    if (hs) hs[q] = h;
    if (kappas) kappas[q] = kap;
    if (gears) gears[q] = (int8_t)gear;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_conn_solve(hipStream_t st, int mode, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx,
                      const double *ty, const double *th, double R, int32_t *word, double *seg, double *len)
{
    if (n <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_conn_solve<M()>, blocks_for(n, CBLOCK), CBLOCK, n, fx, fy, fh, tx, ty, th, R, word, seg, len);
    });
}

int launch_conn_matrix(hipStream_t st, int mode, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to,
                       const double *tx, const double *ty, const double *th, double R, double *D, int8_t *word)
{
    if (n_from <= 0 || n_to <= 0) return 0;
    const dim3 grid(blocks_for(n_to, CONN_COLS), blocks_for(n_from, CONN_ROWS));
    return by_mode(mode, [&](auto M) {
        return launch(st, k_conn_matrix<M()>, grid, CBLOCK, n_from, fx, fy, fh, n_to, tx, ty, th, R, D, word);
    });
}

int launch_dubins_counts(hipStream_t st, int64_t n, const double *len, double spacing, int64_t *out_offsets, int64_t *err)
{
    return launch_sample_counts<CBLOCK>(st, n, DubinsLength{ len }, spacing, 1, 1, out_offsets, err);
}

int launch_rs_counts(hipStream_t st, int64_t n, const int32_t *word, const double *seg, double spacing, int64_t *out_offsets, int64_t *err)
{
    return launch_path_counts<CBLOCK>(st, n, RsCount{ word, seg, spacing }, out_offsets, err);
}

int launch_conn_sample(hipStream_t st, int mode, int64_t n, const double *fx, const double *fy, const double *fh, double R, const int32_t *word,
                       const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                       double *kappas, int8_t *gears)
{
    if (total_samples <= 0 || n <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_conn_sample<M()>, blocks_for(total_samples, CBLOCK), CBLOCK, n, fx, fy, fh, R, word, seg, spacing, out_offsets,
                      total_samples, xs, ys, hs, kappas, gears);
    });
}

}  // namespace fcpp
