// fcpp_route.hip -- gfx950 (MI355X) kernels of the swath router: k_route_transit (every field's block of oriented-swath transits),
// k_route_solve (a candidate tour of a field: construction, improvement sweeps, cost) and k_route_pick (the winner of a field's candidates).
// The rule is ONE set of host+device expressions, fcpp_routefn.h; float64, -ffp-contract=off like every other translation unit, so the
// kernels give the bits fcpp_debug_route_transit / fcpp_debug_route give on the host.
//
// k_route_transit: a thread per entry of every field's block; its field by bisection of the block offsets.  Only the thread of the
// CANONICAL pair of an entry evaluates the connector (dubins_solve / rs_solve of fcpp_dubinsfn.h / fcpp_rsfn.h, nothing restated here) and
// writes both entries that share the value; the other thread leaves.  Which pair is canonical follows the row -- nearly all of a low row,
// nearly none of a high one -- so wavefronts are all in or all out and the connector is evaluated once per two entries.  Bound by fp64
// vector issue like k_conn_matrix; the mirrored entry is a strided 8 B write beside several hundred (Dubins) to several
// thousand (Reeds-Shepp) instructions.
//
// k_route_solve: one workgroup of 256 threads per (field, candidate).  The tour lives in LDS as int16 (m <= 512), twice: a move is applied
// by every thread writing its positions of the NEW tour from the old one (route_moved), then the two swap.  T, E and X are read from
// global memory: a field's block is (2 m)^2 x 8 B -- 128 KiB at m = 64 -- and is re-read by every sweep of every candidate of the field, so
// it stays in L2.  A sweep: the threads stride over the move codes, each keeps its least (delta, code); a shuffle butterfly across the 64
// lanes and an LDS step across the four waves give the workgroup's.  The minimum over (delta, code) pairs does not depend on that order
// and every delta is one fixed expression, so host and device agree bit for bit.  Nearest neighbour is m such arg-min steps over a row of
// T.  No float atomics, no per-thread arrays (no scratch), every loop bounded (max_sweeps <= 2^20 is checked on the host).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_route.h"
#include "fcpp_routefn.h"

namespace fcpp {

static constexpr int RBLOCK = 256;            // k_route_transit, k_route_solve
static constexpr int RWAVES = RBLOCK / 64;
static constexpr int PBLOCK = 64;             // k_route_pick

template <int MODE>
__global__ __launch_bounds__(RBLOCK) void k_route_transit(int64_t n, const int64_t *__restrict__ soff, const double *__restrict__ ax,
                                                          const double *__restrict__ ay, const double *__restrict__ bx,
                                                          const double *__restrict__ by, const double *__restrict__ angle, double R,
                                                          const int64_t *__restrict__ toff, double *__restrict__ T)
{
    const int64_t g = (int64_t)blockIdx.x * RBLOCK + threadIdx.x;
    if (g >= toff[n]) return;
    int64_t lo = 0, hi = n;                    // the last field whose block starts at or before g: the one that holds it
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (toff[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t i = lo, s0 = soff[i], m = soff[i + 1] - s0, e = g - toff[i];
    if (m <= 0 || m > ROUTE_MAX_SWATHS || toff[i + 1] - toff[i] != route_block(m)) return;      // (the host has checked the offsets)
    const int N = (int)(2 * m), p = (int)(e / N), q = (int)(e - (int64_t)p * N);
    if (!route_canonical(p, q, N)) return;
    const double v = route_transit<MODE>(ax + s0, ay + s0, bx + s0, by + s0, angle[i], R, p, q);
    double *blk = T + toff[i];
    blk[p * N + q] = v;
    blk[(q ^ 1) * N + (p ^ 1)] = v;
}

// the workgroup's least (v, code) under route_better, in every thread.  v is never NaN here.
__device__ __forceinline__ void route_wg_min(double &v, int &code, double *sh_v, int *sh_c)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oc = __shfl_xor(code, o);
        if (route_better(ov, oc, v, code)) { v = ov; code = oc; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                           // (the slots' readers of the step before are through)
    if (lane == 0) { sh_v[wave] = v; sh_c[wave] = code; }
    __syncthreads();
    v = sh_v[0]; code = sh_c[0];
#pragma unroll
    for (int w = 1; w < RWAVES; ++w)
        if (route_better(sh_v[w], sh_c[w], v, code)) { v = sh_v[w]; code = sh_c[w]; }
}

__global__ __launch_bounds__(RBLOCK) void k_route_solve(int S, const int64_t *__restrict__ soff, int64_t n_total,
                                                        const int64_t *__restrict__ toff, const double *__restrict__ T,
                                                        const double *__restrict__ E, const double *__restrict__ X, double min_gain,
                                                        int max_sweeps, int32_t *__restrict__ tours, double *__restrict__ costs,
                                                        int32_t *__restrict__ applied_out, double *__restrict__ stored)
{
    __shared__ int16_t tour[2][ROUTE_MAX_SWATHS];
    __shared__ uint8_t seen[ROUTE_MAX_SWATHS];
    __shared__ double sh_v[RWAVES];
    __shared__ int sh_c[RWAVES];
    __shared__ double sh_stored;
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x / S, s0 = soff[i], m64 = soff[i + 1] - s0;
    const int c = (int)(blockIdx.x - i * S);
    int32_t *out = tours + (int64_t)c * n_total + s0;
    if (m64 > ROUTE_MAX_SWATHS) {              // no block, nothing in LDS: the stored order
        for (int64_t k = tid; k < m64; k += RBLOCK) out[k] = (int32_t)(2 * k + (k & 1));
        if (tid == 0) {
            costs[i * S + c] = __builtin_nan("");
            applied_out[i * S + c] = 0;
            if (c == 0) stored[i] = __builtin_nan("");
        }
        return;
    }
    const int m = (int)m64;
    const RouteCosts rc = { T + toff[i], E ? E + 2 * s0 : nullptr, X ? X + 2 * s0 : nullptr, 2 * m };
    int16_t *t = tour[0], *nt = tour[1];
    // candidate 0 as constructed and its cost: the field's status, the same in every workgroup of the field
    for (int k = tid; k < m; k += RBLOCK) t[k] = (int16_t)route_stored(0, k);
    __syncthreads();
    if (tid == 0) sh_stored = route_cost(rc, t, m);
    __syncthreads();
    const bool improve = route_finite(sh_stored);
    if (c == 1) for (int k = tid; k < m; k += RBLOCK) t[k] = (int16_t)route_stored(1, k);
    if (c >= 2 && m > 0) {
        for (int k = tid; k < m; k += RBLOCK) seen[k] = 0;
        int cur = route_nn_start(c, S, rc.N);
        __syncthreads();
        if (tid == 0) { t[0] = (int16_t)cur; seen[cur >> 1] = 1; }
        __syncthreads();
        for (int k = 1; k < m; ++k) {
            double bv = INFINITY;
            int bq = INT32_MAX;
            for (int q = tid; q < rc.N; q += RBLOCK) {
                if (seen[q >> 1]) continue;
                const double v = route_nn_key(rc.T[cur * rc.N + q]);
                if (route_better(v, q, bv, bq)) { bv = v; bq = q; }
            }
            route_wg_min(bv, bq, sh_v, sh_c);          // (an unvisited swath exists: bq names one)
            cur = bq;
            if (tid == 0) { t[k] = (int16_t)cur; seen[cur >> 1] = 1; }
            __syncthreads();
        }
    }
    __syncthreads();
    int applied = 0;
    if (improve) {
        const int n_codes = route_n_codes(m);
        while (applied < max_sweeps) {
            double bd = INFINITY;
            int bc = INT32_MAX;
            RouteMove mv;
            for (int code = tid; code < n_codes; code += RBLOCK) {
                if (!route_decode(m, code, mv)) continue;
                const double d = route_delta(rc, t, m, mv);
                if (route_better(d, code, bd, bc)) { bd = d; bc = code; }
            }
            route_wg_min(bd, bc, sh_v, sh_c);
            if (!(bd < -min_gain)) break;              // (uniform: every thread holds the same pair)
            (void)route_decode(m, bc, mv);
            for (int p = tid; p < m; p += RBLOCK) nt[p] = (int16_t)route_moved(t, mv, p);
            __syncthreads();
            int16_t *sw = t; t = nt; nt = sw;
            ++applied;
        }
    }
    for (int k = tid; k < m; k += RBLOCK) out[k] = t[k];
    if (tid == 0) {
        costs[i * S + c] = route_cost(rc, t, m);
        applied_out[i * S + c] = applied;
        if (c == 0) stored[i] = sh_stored;
    }
}

// per field: status, the winner over its S candidates and the winner's tour
__global__ __launch_bounds__(PBLOCK) void k_route_pick(int S, const int64_t *__restrict__ soff, int64_t n_total,
                                                       const int32_t *__restrict__ tours, const double *__restrict__ costs,
                                                       const int32_t *__restrict__ applied, const double *__restrict__ stored,
                                                       int32_t *__restrict__ route, double *__restrict__ cost, int32_t *__restrict__ winner,
                                                       int32_t *__restrict__ sweeps, int32_t *__restrict__ status)
{
    const int64_t i = blockIdx.x, s0 = soff[i], m = soff[i + 1] - s0;
    const int st = m > ROUTE_MAX_SWATHS ? ROUTE_EUNSUPPORTED : (route_finite(stored[i]) ? ROUTE_OK : ROUTE_EINVAL);
    double best = costs[i * S];
    int w = 0, sw = applied[i * S];
    for (int c = 1; c < S; ++c) {              // (uniform: every lane walks the same S values)
        const double v = costs[i * S + c];
        if (st == ROUTE_OK && v < best) { best = v; w = c; }
        if (applied[i * S + c] > sw) sw = applied[i * S + c];
    }
    if (route) {
        const int32_t *src = tours + (int64_t)w * n_total + s0;
        for (int64_t k = threadIdx.x; k < m; k += PBLOCK) route[s0 + k] = src[k];
    }
    if (threadIdx.x != 0) return;
    if (cost) cost[i] = best;
    if (winner) winner[i] = w;
    if (sweeps) sweeps[i] = sw;
    if (status) status[i] = st;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_route_transit(hipStream_t st, int64_t n, const int64_t *soff, const double *ax, const double *ay, const double *bx, const double *by,
                         const double *angle, double R, int mode, const int64_t *toff, int64_t t_total, double *T)
{
    if (n <= 0 || t_total <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_route_transit<M()>, blocks_for(t_total, RBLOCK), RBLOCK, n, soff, ax, ay, bx, by, angle, R, toff, T);
    });
}

int launch_route_solve(hipStream_t st, int64_t n, int S, const int64_t *soff, int64_t n_total, const int64_t *toff, const double *T,
                       const double *E, const double *X, double min_gain, int max_sweeps, int32_t *tours, double *costs, int32_t *applied,
                       double *stored)
{
    if (n <= 0) return 0;
    return launch(st, k_route_solve, (unsigned)(n * S), RBLOCK, S, soff, n_total, toff, T, E, X, min_gain, max_sweeps, tours, costs, applied, stored);
}

int launch_route_pick(hipStream_t st, int64_t n, int S, const int64_t *soff, int64_t n_total, const int32_t *tours, const double *costs,
                      const int32_t *applied, const double *stored, int32_t *route, double *cost, int32_t *winner, int32_t *sweeps,
                      int32_t *status)
{
    if (n <= 0) return 0;
    return launch(st, k_route_pick, (unsigned)n, PBLOCK, S, soff, n_total, tours, costs, applied, stored, route, cost, winner, sweeps, status);
}

}  // namespace fcpp
