// fcpp_tour.hip -- gfx950 (MI355X) kernels of the cell tour: k_tour_transit (every field's block of node-to-node joints), k_tour_solve (a
// candidate order of a field's cells: construction, improvement sweeps, cost) and k_tour_pick (the winner of a field's candidates, its
// nodes by one more walk of the layers with predecessors, the backtrack).  The rule is ONE set of host+device expressions,
// fcpp_tourfn.h; float64, -ffp-contract=off like every other translation unit, so the kernels give the bits fcpp_debug_cell_tour gives.
//
// k_tour_transit: a thread per entry of every field's block; its field by bisection of the block offsets, the cells of its two nodes
// by bisection of the field's node offsets.  An entry within one cell is +inf without a solve, every other one Conn<MODE>::solve on the
// two poses (fcpp_dubinsfn.h / fcpp_rsfn.h, nothing restated here).  Bound by fp64 vector issue like k_route_transit.
//
// k_tour_solve: one workgroup of 256 threads per (field, candidate).  The order lives in LDS as bytes (k <= 32), twice, like the
// router's tour.  D, E, X and w are read from global memory: a block is at most 8 MiB and is re-read by every sweep of every candidate
// of the field, so it stays in L2.  The hot loop is the move evaluation: a WAVEFRONT per move code, a LANE per target node b of the
// current layer (that is why a cell has at most 64 nodes).  The layer before lives in the lanes' registers; its a-th value comes by a
// shuffle, a ascending, with a strict "less than" -- the host loop's order, so the bits agree without a reduction tree; for a fixed a the
// lanes read 64 consecutive entries of row a of D.  Only the minimum over the last layer and the minimum over (cost, code) across moves
// are reductions; both are lexicographic and total (no value is NaN: tour_plus), so they do not depend on their order.  No float
// atomics, no per-thread arrays (no scratch), every loop bounded (max_sweeps <= 2^20 is checked on the host).
//
// k_tour_pick: a wavefront per field.  The predecessors of the winner's walk are 2 B per node in LDS (N_f <= 1024), not a global
// temporary: the walk and the backtrack share the workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_tour.h"
#include "fcpp_tourfn.h"

namespace fcpp {

static constexpr int TBLOCK = 256;            // k_tour_transit, k_tour_solve
static constexpr int TWAVES = TBLOCK / 64;
static constexpr int TPBLOCK = 64;            // k_tour_pick

template <int MODE>
__global__ __launch_bounds__(TBLOCK) void k_tour_transit(int64_t n, const int64_t *__restrict__ coff, const int64_t *__restrict__ voff,
                                                         const double *__restrict__ ix, const double *__restrict__ iy,
                                                         const double *__restrict__ ih, const double *__restrict__ ox,
                                                         const double *__restrict__ oy, const double *__restrict__ oh, double R,
                                                         const int64_t *__restrict__ doff, double *__restrict__ D)
{
    const int64_t g = (int64_t)blockIdx.x * TBLOCK + threadIdx.x;
    if (g >= doff[n]) return;
    int64_t lo = 0, hi = n;                    // the last field whose block starts at or before g: the one that holds it
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (doff[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t f = lo, c0 = coff[f], c1 = coff[f + 1], v0 = voff[c0], Nf = 2 * (voff[c1] - v0), e = g - doff[f];
    if (Nf <= 0 || c1 - c0 > TOUR_MAX_CELLS || doff[f + 1] - doff[f] != Nf * Nf) return;      // (the host has checked the offsets)
    const int64_t a = e / Nf, b = e - a * Nf;
    if (tour_cell_of(voff, c0, c1, a) == tour_cell_of(voff, c0, c1, b)) { D[g] = INFINITY; return; }
    D[g] = tour_transit<MODE>(ix, iy, ih, ox, oy, oh, R, v0 + (a >> 1), (int)(a & 1), v0 + (b >> 1), (int)(b & 1));
}

// the wavefront's least (v, idx) under tour_better, in every lane.  v is never NaN.
__device__ __forceinline__ void tour_wave_min(double &v, int &idx)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(idx, o);
        if (tour_better(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
}

// tour_eval_host by ONE wavefront, every lane of which calls it with the same arguments: lane b holds node b of the current layer.
// pred (LDS, N_f, or NULL) and last as there.  The result is the same in every lane.
__device__ __forceinline__ double tour_eval_wave(const TourField &F, const uint8_t *t, int k, const TourMove &mv, int16_t *pred, int *last)
{
    const int lane = threadIdx.x & 63;
    if (last) *last = -1;
    if (k <= 0) return 0.0;
    double g = INFINITY;
    int nprev = 0, n0prev = 0;
    for (int j = 0; j < k; ++j) {
        const int cell = tour_moved(t, mv, j), n0 = F.noff[cell], nc = F.noff[cell + 1] - n0;
        const bool mine = lane < nc;
        double ng = INFINITY;
        if (j == 0) {
            if (mine) ng = tour_first(F, n0 + lane);
        } else {
            double best = INFINITY;
            int arg = 0;
            // (uniform: every lane walks the layer before.)  Four rows of D are loaded before the first of them is used, so that their
            // latencies overlap; the sums and the comparisons stay in the order a = 0, 1, 2, .. of the host loop.
            const double *col = F.D + n0prev * F.Nf + n0 + lane;
            int a = 0;
            for (; a + 4 <= nprev; a += 4) {
                double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
                if (mine) { d0 = col[a * F.Nf]; d1 = col[(a + 1) * F.Nf]; d2 = col[(a + 2) * F.Nf]; d3 = col[(a + 3) * F.Nf]; }
                const double g0 = __shfl(g, a), g1 = __shfl(g, a + 1), g2 = __shfl(g, a + 2), g3 = __shfl(g, a + 3);
                if (mine) {
                    double v = tour_plus(g0, d0);
                    if (a == 0 || v < best) { best = v; arg = a; }
                    v = tour_plus(g1, d1);
                    if (v < best) { best = v; arg = a + 1; }
                    v = tour_plus(g2, d2);
                    if (v < best) { best = v; arg = a + 2; }
                    v = tour_plus(g3, d3);
                    if (v < best) { best = v; arg = a + 3; }
                }
            }
            for (; a < nprev; ++a) {
                const double ga = __shfl(g, a);
                if (mine) {
                    const double v = tour_step(F, ga, n0prev + a, n0 + lane);
                    if (a == 0 || v < best) { best = v; arg = a; }
                }
            }
            if (mine) {
                ng = tour_close(F, best, n0 + lane);
                if (pred) pred[n0 + lane] = (int16_t)arg;
            }
        }
        g = ng; nprev = nc; n0prev = n0;
    }
    double v = lane < nprev ? tour_last(F, g, n0prev + lane) : INFINITY;
    int b = lane < nprev ? lane : INT32_MAX;
    tour_wave_min(v, b);                       // (lane 0 holds a node: b names one)
    if (last) *last = n0prev + b;
    return v;
}

// what k_tour_solve and k_tour_pick set up alike in LDS: the cells' node offsets, the kept and the skipped cells -> k.  m <= TOUR_MAX_CELLS.
__device__ __forceinline__ int tour_field_lds(const int64_t *voff, int64_t c0, int m, int *noff, uint8_t *kept, uint8_t *rest, int *sh_k)
{
    for (int j = threadIdx.x; j <= m; j += blockDim.x) noff[j] = (int)(2 * (voff[c0 + j] - voff[c0]));
    __syncthreads();
    if (threadIdx.x == 0) {
        int k = 0, n_rest = 0;
        for (int j = 0; j < m; ++j)
            if (noff[j + 1] > noff[j]) kept[k++] = (uint8_t)j; else rest[n_rest++] = (uint8_t)j;
        *sh_k = k;
    }
    __syncthreads();
    return *sh_k;
}

__global__ __launch_bounds__(TBLOCK) void k_tour_solve(int S, const int64_t *__restrict__ coff, int64_t n_cells, const int64_t *__restrict__ voff,
                                                       const double *__restrict__ w, const int32_t *__restrict__ stored_node,
                                                       const int64_t *__restrict__ doff, const double *__restrict__ D,
                                                       const double *__restrict__ E, const double *__restrict__ X, double min_gain,
                                                       int max_sweeps, int32_t *__restrict__ tours, double *__restrict__ costs,
                                                       int32_t *__restrict__ applied_out, double *__restrict__ stored)
{
    __shared__ uint8_t ord[2][TOUR_MAX_CELLS];
    __shared__ uint8_t kept[TOUR_MAX_CELLS], rest[TOUR_MAX_CELLS];
    __shared__ int noff[TOUR_MAX_CELLS + 1];
    __shared__ double C[TOUR_MAX_CELLS * TOUR_MAX_CELLS];
    __shared__ double sh_v[TWAVES];
    __shared__ int sh_c[TWAVES];
    __shared__ double sh_stored;
    __shared__ int sh_k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.x / S, c0 = coff[f], c1 = coff[f + 1], m64 = c1 - c0;
    const int c = (int)(blockIdx.x - f * S);
    int32_t *out = tours + (int64_t)c * n_cells + c0;
    if (!tour_supported(voff, c0, c1)) {       // no block, nothing in LDS: the stored order of every cell
        for (int64_t q = tid; q < m64; q += TBLOCK) out[q] = (int32_t)q;
        if (tid == 0) {
            costs[f * S + c] = __builtin_nan("");
            applied_out[f * S + c] = 0;
            if (c == 0) stored[f] = __builtin_nan("");
        }
        return;
    }
    const int m = (int)m64;
    const int k = tour_field_lds(voff, c0, m, noff, kept, rest, &sh_k);
    const int64_t n0 = 2 * voff[c0];
    const TourField F = { D + doff[f], E ? E + n0 : nullptr, X ? X + n0 : nullptr, w + voff[c0], noff, noff[m] };
    // the stored cost: the field's status, the same in every workgroup of the field
    if (tid == 0) sh_stored = tour_stored(F, kept, k, stored_node ? stored_node + c0 : nullptr);
    // C, for a nearest-neighbour candidate: a wavefront per pair of cells, a lane per node of the second
    if (c >= 2 && k > 0) {
        for (int pair = wave; pair < m * m; pair += TWAVES) {
            const int i = pair / m, j = pair - i * m, nj = noff[j + 1] - noff[j];
            double mn = INFINITY;
            if (i != j && lane < nj)
                for (int a = noff[i]; a < noff[i + 1]; ++a) {
                    const double v = tour_key(F.D[a * F.Nf + noff[j] + lane]);
                    if (v < mn) mn = v;
                }
            int any = 0;
            tour_wave_min(mn, any);
            if (lane == 0) C[i * TOUR_MAX_CELLS + j] = mn;
        }
    }
    __syncthreads();
    const bool improve = tour_finite(sh_stored);
    uint8_t *t = ord[0], *nt = ord[1];
    if (tid == 0 && k > 0) tour_construct(C, kept, k, c, S, t);
    __syncthreads();
    const TourMove none = { -1, 0, 0, 0, 0, 0 };
    double cur = tour_eval_wave(F, t, k, none, nullptr, nullptr);          // (every wavefront for itself: the same bits)
    int applied = 0;
    if (improve) {
        const int n_codes = tour_n_codes(k);
        while (applied < max_sweeps) {
            double bd = INFINITY;
            int bc = INT32_MAX;
            TourMove mv;
            for (int code = wave; code < n_codes; code += TWAVES) {          // (uniform within a wavefront)
                if (!tour_decode(k, code, mv)) continue;
                const double d = tour_eval_wave(F, t, k, mv, nullptr, nullptr);
                if (tour_better(d, code, bd, bc)) { bd = d; bc = code; }
            }
            __syncthreads();                   // (the slots' readers of the sweep before are through)
            if (lane == 0) { sh_v[wave] = bd; sh_c[wave] = bc; }
            __syncthreads();
            bd = sh_v[0]; bc = sh_c[0];
#pragma unroll
            for (int x = 1; x < TWAVES; ++x)
                if (tour_better(sh_v[x], sh_c[x], bd, bc)) { bd = sh_v[x]; bc = sh_c[x]; }
            if (!(bd < cur - min_gain)) break;         // (uniform: every thread holds the same pair)
            (void)tour_decode(k, bc, mv);
            if (tid < k) nt[tid] = (uint8_t)tour_moved(t, mv, tid);
            __syncthreads();
            uint8_t *sw = t; t = nt; nt = sw;
            cur = bd;
            ++applied;
        }
    }
    if (tid < m) out[tid] = tid < k ? t[tid] : rest[tid - k];
    if (tid == 0) {
        costs[f * S + c] = cur;
        applied_out[f * S + c] = applied;
        if (c == 0) stored[f] = sh_stored;
    }
}

// per field: status, the winner over its S candidates, its nodes and joints
__global__ __launch_bounds__(TPBLOCK) void k_tour_pick(int S, const int64_t *__restrict__ coff, int64_t n_cells, const int64_t *__restrict__ voff,
                                                       const double *__restrict__ w, const int32_t *__restrict__ stored_node,
                                                       const int64_t *__restrict__ doff, const double *__restrict__ D,
                                                       const double *__restrict__ E, const double *__restrict__ X,
                                                       const int32_t *__restrict__ tours, const double *__restrict__ costs,
                                                       const int32_t *__restrict__ applied, const double *__restrict__ stored_in,
                                                       int32_t *__restrict__ order, int32_t *__restrict__ node, double *__restrict__ cost,
                                                       double *__restrict__ stored, double *__restrict__ joint, int32_t *__restrict__ winner,
                                                       int32_t *__restrict__ sweeps, int32_t *__restrict__ skipped, int32_t *__restrict__ status)
{
    __shared__ uint8_t t[TOUR_MAX_CELLS], kept[TOUR_MAX_CELLS], rest[TOUR_MAX_CELLS];
    __shared__ int noff[TOUR_MAX_CELLS + 1];
    __shared__ int32_t nd[TOUR_MAX_CELLS];
    __shared__ int16_t pred[TOUR_MAX_NODES];
    __shared__ int sh_k;
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x, c0 = coff[f], c1 = coff[f + 1], m64 = c1 - c0;
    const double nan = __builtin_nan("");
    if (!tour_supported(voff, c0, c1)) {
        int empty = 0;
        for (int64_t q = tid; q < m64; q += TPBLOCK) {
            if (order) order[c0 + q] = (int32_t)q;
            if (node) node[c0 + q] = -1;
            empty += voff[c0 + q + 1] == voff[c0 + q];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) empty += __shfl_xor(empty, o);
        if (tid != 0) return;
        if (cost) cost[f] = nan;
        if (stored) stored[f] = nan;
        if (joint) joint[f] = nan;
        if (winner) winner[f] = 0;
        if (sweeps) sweeps[f] = 0;
        if (skipped) skipped[f] = empty;
        if (status) status[f] = TOUR_EUNSUPPORTED;
        return;
    }
    const int m = (int)m64;
    const int k = tour_field_lds(voff, c0, m, noff, kept, rest, &sh_k);
    const int64_t n0 = 2 * voff[c0];
    const TourField F = { D + doff[f], E ? E + n0 : nullptr, X ? X + n0 : nullptr, w + voff[c0], noff, noff[m] };
    const double st = stored_in[f];
    const bool improve = tour_finite(st);
    double best = costs[f * S];
    int win = 0, sw = applied[f * S];
    for (int c = 1; c < S; ++c) {              // (uniform: every lane walks the same S values)
        const double v = costs[f * S + c];
        if (improve && v < best) { best = v; win = c; }
        if (applied[f * S + c] > sw) sw = applied[f * S + c];
    }
    const int32_t *src = tours + (int64_t)win * n_cells + c0;
    if (tid < m) { t[tid] = (uint8_t)src[tid]; nd[tid] = -1; }
    __syncthreads();
    double jl = nan;
    if (improve) {
        const TourMove none = { -1, 0, 0, 0, 0, 0 };
        int b = -1;
        best = tour_eval_wave(F, t, k, none, pred, &b);
        __syncthreads();                       // (the predecessors are written)
        if (tid == 0) {
            for (int q = k - 1; q >= 0; --q) {
                const int cell = t[q];
                nd[cell] = b - noff[cell];
                if (q > 0) b = noff[t[q - 1]] + pred[b];
            }
            jl = tour_joints(F, t, k, nd);
        }
    } else {
        best = st;
        const int32_t *sn = stored_node ? stored_node + c0 : nullptr;
        if (tid < k) {
            const int cell = kept[tid], u = sn ? sn[cell] : 0;
            nd[cell] = (u < 0 || u >= noff[cell + 1] - noff[cell]) ? 0 : u;
        }
    }
    __syncthreads();
    if (tid < m) {
        if (order) order[c0 + tid] = t[tid];
        if (node) node[c0 + tid] = nd[tid];
    }
    if (tid != 0) return;
    if (cost) cost[f] = best;
    if (stored) stored[f] = st;
    if (joint) joint[f] = jl;
    if (winner) winner[f] = win;
    if (sweeps) sweeps[f] = sw;
    if (skipped) skipped[f] = m - k;
    if (status) status[f] = improve ? TOUR_OK : TOUR_EINVAL;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_tour_transit(hipStream_t st, int64_t n, const int64_t *coff, const int64_t *voff, const double *ix, const double *iy, const double *ih,
                        const double *ox, const double *oy, const double *oh, double R, int mode, const int64_t *doff, int64_t d_total, double *D)
{
    if (n <= 0 || d_total <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_tour_transit<M()>, blocks_for(d_total, TBLOCK), TBLOCK, n, coff, voff, ix, iy, ih, ox, oy, oh, R, doff, D);
    });
}

int launch_tour_solve(hipStream_t st, int64_t n, int S, const int64_t *coff, int64_t n_cells, const int64_t *voff, const double *w,
                      const int32_t *stored_node, const int64_t *doff, const double *D, const double *E, const double *X, double min_gain,
                      int max_sweeps, int32_t *tours, double *costs, int32_t *applied, double *stored)
{
    if (n <= 0) return 0;
    return launch(st, k_tour_solve, (unsigned)(n * S), TBLOCK, S, coff, n_cells, voff, w, stored_node, doff, D, E, X, min_gain, max_sweeps, tours, costs,
                  applied, stored);
}

int launch_tour_pick(hipStream_t st, int64_t n, int S, const int64_t *coff, int64_t n_cells, const int64_t *voff, const double *w,
                     const int32_t *stored_node, const int64_t *doff, const double *D, const double *E, const double *X, const int32_t *tours,
                     const double *costs, const int32_t *applied, const double *stored_in, int32_t *order, int32_t *node, double *cost,
                     double *stored, double *joint, int32_t *winner, int32_t *sweeps, int32_t *skipped, int32_t *status)
{
    if (n <= 0) return 0;
    return launch(st, k_tour_pick, (unsigned)n, TPBLOCK, S, coff, n_cells, voff, w, stored_node, doff, D, E, X, tours, costs, applied, stored_in, order,
                  node, cost, stored, joint, winner, sweeps, skipped, status);
}

}  // namespace fcpp
