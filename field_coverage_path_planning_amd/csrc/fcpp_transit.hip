// fcpp_transit.hip -- gfx950 (MI355X) kernels of the loop transits: per pair of poses the cheapest "clear connector to a station of a
// headland loop, ride along the loop, clear connector from a second station" (the rule: fcpp_transitfn.h over fcpp_solveclearfn.h).
// float64, -ffp-contract=off like every other translation unit, so the kernels give the bits fcpp_debug_loop_transits gives on the host.
// Plain C++: no inline assembly, no atomics on doubles, every loop bounded.
//
// k_transit_stations, a wavefront per field: the field's loops one after the other, 64 samples at a time; a ballot of the lanes whose
// sample is a station gives every one its place (the count so far + the set bits below the lane), so the list is in sample order
// whatever the hardware does.  Lane 0 writes the count and whether every loop of the field has a finite first and last s.
//
// THE STATIONS PASS is the two passes of k_solve_clear_pairs / _words on the items (pair, side, station slot): side 0 the connector
// P -> station, side 1 station -> Q.  k_transit_sides, a lane per item of a grid of `per` slots per side (per: the batch's largest station
// count rounded up to the workgroup, read back by the call): solve_clear_first -- the solve, the shortest word's test, the field's edges
// read from GLOBAL memory through the CSR as k_solve_clear_pairs reads them (all lanes of a wavefront belong to one pair, hence one
// field: they read the same vertex, one cache line served by the vector L1; staging the edges through LDS in CLEAR_EDGE_CHUNK chunks as
// k_clear_transit does would save those L1 hits and is not done: static reasoning, not measured).  Every lane of a pair of status 0
// with a station writes val = the len, or +inf unless rank 0, and lists its item when the other words have to be looked at
// (solve_clear_append).  k_transit_words, a group of lanes per listed item, is solve_clear_group as it is; a clear winner overwrites
// val with its total.  Skipped by the call when nothing is listed.
//
// THE PICK PASS, k_transit_pick, a workgroup per pair: thread t owns the in-stations t, t + 256, ...; the out-stations go through LDS in
// tiles of 256 (out_j, s_j, the global sample index and the loop: 32 B each, 8 KiB), every thread reads the same j: a broadcast.  Per (i, j)
// of one loop three additions and a lexicographic compare.  The least (C, i, j) of a thread, then of a wavefront by xor-shuffles, then of
// the four wavefronts through LDS by thread 0: the order is total, so any reduction tree gives the same minimiser.
// k_transit_finish, a lane per pair: transit_finish -- both connectors of the pick by the sequential form of the rule, so word, seg, len
// and rank have solve_clear's bits; 2 solves and at most 2 x 48 tests per pair, beside n_st solves and tests per pair above.
//
// COUNTS AND FILL: the samplers' scan (k_path_counts of fcpp_samplefn.h) on transit_counts, then a lane per output sample: its pair by
// bisection of the offsets (sample_path), transit_eval -- a connector sample by Conn<MODE>::eval, a ride sample a copy.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_listfn.h"
#include "fcpp_samplefn.h"
#include "fcpp_solvegroupfn.h"
#include "fcpp_transit.h"

namespace fcpp {

static constexpr int TBLOCK = TRANSIT_BLOCK;
static constexpr int TWAVES = TBLOCK / 64;
static_assert(TBLOCK == SOLVECLEAR_BLOCK, "solve_clear_group's groups are laid out for that workgroup");

__global__ __launch_bounds__(TBLOCK) void k_transit_stations(TransitLoops L, TransitTemp T)
{
    const int lane = threadIdx.x & 63;
    const int64_t f = ((int64_t)blockIdx.x * TBLOCK + threadIdx.x) >> 6;
    if (f >= L.n_fields) return;                          // (uniform over the wavefront)
    const int64_t l0 = L.field_loops[f], l1 = L.field_loops[f + 1];
    const int64_t base = l1 > l0 ? L.loop_off[l0] : 0;
    int64_t count = 0;
    int ok = 1;
    for (int64_t l = l0; l < l1; ++l) {
        if (!transit_loop_ok(L, l)) ok = 0;
        const int64_t g1 = L.loop_off[l + 1];
        for (int64_t g0 = L.loop_off[l]; g0 < g1; g0 += 64) {
            const int64_t g = g0 + lane;
            const bool is = g < g1 && transit_is_station(L, l, g);
            const unsigned long long m = __ballot(is);
            if (is) {
                const int64_t at = base + count + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
                T.st_idx[at] = g;
                T.st_loop[at] = l;
            }
            count += (int64_t)__popcll(m);
        }
    }
    if (lane == 0) { T.n_st[f] = count; T.loops_ok[f] = ok; }
}

// item = (pair * 2 + side) * per + slot
struct TransitItem { int64_t pair, f; int side; double px, py, ph, sx, sy, sh; };

// the item's pair, field and poses; false: no work (no such pair, a pair whose status is not 0, a slot beyond the field's stations)
__device__ __forceinline__ bool transit_item(int64_t item, int64_t n, int64_t per, const TransitIo &io, const TransitLoops &L, const TransitTemp &T,
                                             TransitItem &it)
{
    it.pair = item / (2 * per);
    const int64_t r = item - it.pair * 2 * per, slot = r % per;
    it.side = (int)(r / per);
    it.f = -1;
    it.px = it.py = it.ph = it.sx = it.sy = it.sh = 0.0;
    if (item < 0 || it.pair >= n) return false;
    const int64_t p = it.pair;
    const int64_t f = io.pair_field[p];
    if (transit_pair_status(io.fx[p], io.fy[p], io.fh[p], io.tx[p], io.ty[p], io.th[p], f, L.n_fields, T.region_status, T.loops_ok, T.n_st) != TRANSIT_OK)
        return false;
    if (slot >= T.n_st[f]) return false;
    const int64_t g = T.st_idx[L.loop_off[L.field_loops[f]] + slot];
    it.f = f;
    it.px = it.side == 0 ? io.fx[p] : io.tx[p]; it.py = it.side == 0 ? io.fy[p] : io.ty[p]; it.ph = it.side == 0 ? io.fh[p] : io.th[p];
    it.sx = L.x[g]; it.sy = L.y[g]; it.sh = L.h[g];
    return true;
}

template <int MODE>
__global__ __launch_bounds__(TBLOCK) void k_transit_sides(int64_t n, int64_t per, TransitIo io, double R, ClearFields F, TransitLoops L, TransitTemp T,
                                                          int64_t *__restrict__ list, unsigned long long *__restrict__ count)
{
    const int64_t item = (int64_t)blockIdx.x * TBLOCK + threadIdx.x;
    TransitItem it;
    bool more = false;
    if (transit_item(item, n, per, io, L, T, it)) {
        SolveClearResult r;
        more = it.side == 0 ? solve_clear_first<MODE>(F, it.f, it.px, it.py, it.ph, it.sx, it.sy, it.sh, R, r)
                            : solve_clear_first<MODE>(F, it.f, it.sx, it.sy, it.sh, it.px, it.py, it.ph, R, r);
        T.val[item] = transit_side_len(r);
    }
    solve_clear_append(more, item, list, count);
}

template <int MODE>
__global__ __launch_bounds__(TBLOCK) void k_transit_words(int64_t count, const int64_t *__restrict__ list, int64_t n, int64_t per, TransitIo io, double R,
                                                          ClearFields F, TransitLoops L, TransitTemp T)
{
    constexpr int G = SolveClearGroup<MODE>::G;
    const int64_t t = (int64_t)blockIdx.x * TBLOCK + threadIdx.x, j = t / G;
    bool have = j < count;
    const int64_t item = have ? list[j] : -1;
    TransitItem it;
    have = transit_item(item, n, per, io, L, T, it) && have;      // (a listed item has work: checked again so that nothing is written beside val)
    const bool in = it.side == 0;
    solve_clear_group<MODE>(have, it.f, in ? it.px : it.sx, in ? it.py : it.sy, in ? it.ph : it.sh, in ? it.sx : it.px, in ? it.sy : it.py,
                            in ? it.sh : it.ph, R, F, [&](int, const double *, double total, int rank, int) {
                                if (rank >= 0) T.val[item] = total;
                            });
}

__global__ __launch_bounds__(TBLOCK) void k_transit_pick(int64_t n, int64_t per, TransitIo io, TransitLoops L, TransitTemp T)
{
    __shared__ double sh_out[TBLOCK], sh_s[TBLOCK];
    __shared__ int64_t sh_g[TBLOCK], sh_l[TBLOCK];
    __shared__ double red_C[TWAVES];
    __shared__ int64_t red_l[TWAVES], red_i[TWAVES], red_j[TWAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    if (p >= n) return;                                   // (uniform over the workgroup)
    const int64_t f = io.pair_field[p];
    const int status = transit_pair_status(io.fx[p], io.fy[p], io.fh[p], io.tx[p], io.ty[p], io.th[p], f, L.n_fields, T.region_status, T.loops_ok, T.n_st);
    TransitPick best = transit_pick_none();
    if (status == TRANSIT_OK) {                           // (uniform: nobody is left at a barrier)
        const int64_t n_st = T.n_st[f], base = n_st > 0 ? L.loop_off[L.field_loops[f]] : 0;
        const double *in = T.val + p * 2 * per, *out = in + per;
        for (int64_t j0 = 0; j0 < n_st; j0 += TBLOCK) {
            const int cnt = (int)(n_st - j0 < TBLOCK ? n_st - j0 : TBLOCK);
            __syncthreads();                              // (the tile before has been read by everybody)
            if (tid < cnt) {
                const int64_t g = T.st_idx[base + j0 + tid];
                sh_out[tid] = out[j0 + tid]; sh_s[tid] = L.s[g]; sh_g[tid] = g; sh_l[tid] = T.st_loop[base + j0 + tid];
            }
            __syncthreads();
            for (int64_t a = tid; a < n_st; a += TBLOCK) {
                const double in_i = in[a];
                if (!(in_i < INFINITY)) continue;
                const int64_t gi = T.st_idx[base + a], li = T.st_loop[base + a];
                const double si = L.s[gi], S = L.s[L.loop_off[li + 1] - 1];
                for (int jj = 0; jj < cnt; ++jj) {
                    if (sh_l[jj] != li) continue;
                    const int64_t gj = sh_g[jj];
                    transit_pick_take(best, transit_cost(in_i, transit_ride_s(si, sh_s[jj], S, gj >= gi), sh_out[jj]), li, gi, gj);
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oC = __shfl_xor(best.C, o);
        const int64_t ol = __shfl_xor(best.l, o), oi = __shfl_xor(best.i, o), oj = __shfl_xor(best.j, o);
        transit_pick_take(best, oC, ol, oi, oj);
    }
    if (lane == 0) { red_C[wave] = best.C; red_l[wave] = best.l; red_i[wave] = best.i; red_j[wave] = best.j; }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < TWAVES; ++w) transit_pick_take(best, red_C[w], red_l[w], red_i[w], red_j[w]);
    T.pick_l[p] = best.l; T.pick_i[p] = best.i; T.pick_j[p] = best.j;
}

template <int MODE>
__global__ __launch_bounds__(TBLOCK) void k_transit_finish(int64_t n, TransitIo io, double R, ClearFields F, TransitLoops L, TransitTemp T)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    const int64_t p = (int64_t)blockIdx.x * TBLOCK + threadIdx.x;
    if (p >= n) return;
    const int64_t f = io.pair_field[p];
    const double x0 = io.fx[p], y0 = io.fy[p], h0 = io.fh[p], x1 = io.tx[p], y1 = io.ty[p], h1 = io.th[p];
    const int status = transit_pair_status(x0, y0, h0, x1, y1, h1, f, L.n_fields, T.region_status, T.loops_ok, T.n_st);
    const TransitPick pick = { INFINITY, T.pick_l[p], T.pick_i[p], T.pick_j[p] };
    const TransitResult r = transit_finish<MODE>(F, L, f, x0, y0, h0, x1, y1, h1, R, status, pick);
    if (io.found) io.found[p] = r.found;
    if (io.loop) io.loop[p] = r.loop;
    if (io.i) io.i[p] = r.i;
    if (io.j) io.j[p] = r.j;
    if (io.in_word) io.in_word[p] = r.in.word;
    if (io.out_word) io.out_word[p] = r.out.word;
#pragma unroll
    for (int k = 0; k < NSEG; ++k) {
        if (io.in_seg) io.in_seg[p * NSEG + k] = r.in.seg[k];
        if (io.out_seg) io.out_seg[p * NSEG + k] = r.out.seg[k];
    }
    if (io.in_len) io.in_len[p] = r.in.len;
    if (io.out_len) io.out_len[p] = r.out.len;
    if (io.in_rank) io.in_rank[p] = r.in.rank;
    if (io.out_rank) io.out_rank[p] = r.out.rank;
    if (io.ride) io.ride[p] = r.ride;
    if (io.total) io.total[p] = r.total;
    if (io.status) io.status[p] = r.status;
}

// the samples of pair p as the scan takes them
template <int MODE> struct TransitCount {
    TransitRec rec;
    int64_t n_loops;
    const int64_t *loop_off;
    double spacing;
    __device__ int64_t operator()(int64_t p, int64_t &bad) const
    {
        int64_t a, b, c;
        transit_counts<MODE>(rec, n_loops, loop_off, spacing, p, a, b, c, bad);
        return a + b + c;
    }
};

template <int MODE>
__global__ __launch_bounds__(TBLOCK) void k_transit_fill(int64_t n, TransitRec rec, TransitLoops L, const double *__restrict__ fx,
                                                         const double *__restrict__ fy, const double *__restrict__ fh, double R, double spacing,
                                                         const int64_t *__restrict__ off, int64_t total_samples, double *__restrict__ xs,
                                                         double *__restrict__ ys, double *__restrict__ hs, double *__restrict__ kappas,
                                                         int8_t *__restrict__ parts, int8_t *__restrict__ gears)
{
    const int64_t q = (int64_t)blockIdx.x * TBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t p, k, K;
    sample_path(off, n, q, p, k, K);
    double x, y, h, kap;
    int part, gear;
    transit_eval<MODE>(rec, L, fx, fy, fh, R, spacing, p, k, K, x, y, h, kap, part, gear);
    if (xs) xs[q] = x;
    if (ys) ys[q] = y;
    if (hs) hs[q] = h;
    if (kappas) kappas[q] = kap;
    if (parts) parts[q] = (int8_t)part;
    if (gears) gears[q] = (int8_t)gear;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_transit_stations(hipStream_t st, const TransitLoops &L, const TransitTemp &T)
{
    if (L.n_fields <= 0) return 0;
    return launch(st, k_transit_stations, blocks_for(L.n_fields * 64, TBLOCK), TBLOCK, L, T);
}

int launch_transit_sides(hipStream_t st, int mode, int64_t n, int64_t per, const TransitIo &io, double R, const ClearFields &F, const TransitLoops &L,
                         const TransitTemp &T, int64_t *list, unsigned long long *count)
{
    if (n <= 0 || per <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_transit_sides<M()>, blocks_for(n * 2 * per, TBLOCK), TBLOCK, n, per, io, R, F, L, T, list, count);
    });
}

int launch_transit_words(hipStream_t st, int mode, int64_t count, const int64_t *list, int64_t n, int64_t per, const TransitIo &io, double R,
                         const ClearFields &F, const TransitLoops &L, const TransitTemp &T)
{
    if (count <= 0) return 0;
    const int64_t group = TBLOCK / (mode == 0 ? SolveClearGroup<0>::G : SolveClearGroup<1>::G);
    return by_mode(mode, [&](auto M) {
        return launch(st, k_transit_words<M()>, blocks_for(count, group), TBLOCK, count, list, n, per, io, R, F, L, T);
    });
}

int launch_transit_pick(hipStream_t st, int64_t n, int64_t per, const TransitIo &io, const TransitLoops &L, const TransitTemp &T)
{
    if (n <= 0) return 0;
    return launch(st, k_transit_pick, (unsigned)n, TBLOCK, n, per, io, L, T);
}

int launch_transit_finish(hipStream_t st, int mode, int64_t n, const TransitIo &io, double R, const ClearFields &F, const TransitLoops &L,
                          const TransitTemp &T)
{
    if (n <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_transit_finish<M()>, blocks_for(n, TBLOCK), TBLOCK, n, io, R, F, L, T);
    });
}

int launch_transit_counts(hipStream_t st, int mode, int64_t n, const TransitRec &rec, int64_t n_loops, const int64_t *loop_off, double spacing,
                          int64_t *out_offsets, int64_t *err)
{
    return by_mode(mode, [&](auto M) {
        return launch_path_counts<TBLOCK>(st, n, TransitCount<M()>{ rec, n_loops, loop_off, spacing }, out_offsets, err);
    });
}

int launch_transit_fill(hipStream_t st, int mode, int64_t n, const TransitRec &rec, const TransitLoops &L, const double *fx, const double *fy,
                        const double *fh, double R, double spacing, const int64_t *out_offsets, int64_t total_samples, double *x, double *y,
                        double *heading, double *kappa, int8_t *part, int8_t *gear)
{
    if (n <= 0 || total_samples <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_transit_fill<M()>, blocks_for(total_samples, TBLOCK), TBLOCK, n, rec, L, fx, fy, fh, R, spacing, out_offsets,
                      total_samples, x, y, heading, kappa, part, gear);
    });
}

}  // namespace fcpp
