// fcpp_clear.hip -- gfx950 (MI355X) kernels of the connector clearance: k_clear_transit (every canonical pair of every field's transit
// block: its connector solved again and tested against the field's rings), k_clear_conn (a lane per solved path against the field it
// names) and k_clear_field_status.  The rule is ONE set of host+device expressions, fcpp_clearfn.h; float64, -ffp-contract=off like every
// other translation unit, so the kernels give the bits fcpp_debug_route_transit_clear / fcpp_debug_conn_clear give on the host.
//
// k_clear_transit: a workgroup of 256 threads owns CLEAR_TILE = 256 consecutive entries of ONE field's block (the host hands it the
// fields' tile offsets; the field by bisection).  As in k_route_transit only the lane of an entry's CANONICAL pair works.  The canonical
// pairs are roughly the upper triangle of the block and a tile is cut at multiples of 256 entries, not of a row: a wavefront of a low
// row is nearly full, one of a high row nearly empty, and in between it is PARTLY idle through the whole edge loop -- about half of all
// lanes idle, which at 1 - 2 waves per SIMD shows in the rate.  A working lane solves its pair through Conn<MODE> and keeps the
// pieces (3 or 5 records of 8 doubles) in registers: every loop over them is unrolled, there is no per-thread array in memory.  The
// field's edges come through LDS in chunks of CLEAR_EDGE_CHUNK: thread j stages edge j as (x0, y0, x1, y1, ex, ey) -- the end vertex
// beside e = B - A, so that two edges at a vertex see the same bits -- 48 B per edge, 12 KiB per workgroup, and the chunk's bounding box
// is reduced by shuffles and one LDS step.  In the inner loop all lanes read the SAME edge: an LDS broadcast, no bank conflicts.  A lane
// skips a chunk whose box meets neither its path's box nor the ray of its start point; a wavefront whose lanes all skip branches over
// the loop.  The lane that owns the canonical pair writes both mirrored entries of B, and of T where the pair is blocked: no entry has
// two writers, no atomics.  Bound by fp64 vector issue: per (piece, edge) four cross products for a straight, a discriminant for an arc.
//
// k_clear_transit<MODE, true> is the FIRST PASS of the priced transit block (fcpp_route_transit_priced; the second one is
// k_route_priced_words of fcpp_solveclear.hip): the same walk, but T is out only -- the owning lane keeps the pair's total and writes a
// complete answer to both mirrored entries, the total with K = 0 where the shortest word is clear, fl(total + penalty) with K = -1 where
// it is not, +inf with K = 0 within one swath -- and it appends the entry's global index to the list iff the field is valid, the start is
// inside and the word crosses (solve_clear_first's decision; solve_clear_append of fcpp_listfn.h).  One body: the flag only changes what
// the owning lane does after the edge loop.
//
// k_clear_conn: the same edge loop with a lane per path, the edges read from GLOBAL memory through the field's CSR (clear_walk).  Paths
// grouped by field make all lanes of a wavefront read the same vertex -- one cache line, served by the vector L1 -- and paths that are not
// grouped are still right: nothing is staged per wavefront, so no result depends on the grouping and no uniformity has to be detected.
// The elementwise batches are small beside the matrix (the legs of a route: m + 1 per field, against (2 m)^2 / 2 pairs).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_clear.h"
#include "fcpp_clearfn.h"
#include "fcpp_launch.h"
#include "fcpp_listfn.h"

namespace fcpp {

static constexpr int CBLOCK = 256;            // k_clear_transit (= CLEAR_TILE = CLEAR_EDGE_CHUNK), k_clear_conn
static constexpr int CWAVES = CBLOCK / 64;
static_assert(CBLOCK == CLEAR_TILE && CBLOCK == CLEAR_EDGE_CHUNK, "a thread per entry of the tile and per staged edge");

struct __attribute__((aligned(16))) ClearEdge { double x0, y0, x1, y1, ex, ey; };

__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// PRICED: B is K (int8: 0 or -1 as a byte; may be NULL), T is out only, list / count take the entries to look at again
template <int MODE, bool PRICED>
__global__ __launch_bounds__(CBLOCK) void k_clear_transit(int64_t n, const int64_t *__restrict__ soff, const double *__restrict__ ax,
                                                          const double *__restrict__ ay, const double *__restrict__ bx,
                                                          const double *__restrict__ by, const double *__restrict__ angle, double R,
                                                          const int64_t *__restrict__ toff, const int64_t *__restrict__ tile_off,
                                                          ClearFields F, double penalty, double *__restrict__ T, uint8_t *__restrict__ B,
                                                          int64_t *__restrict__ list, unsigned long long *__restrict__ count)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    __shared__ ClearEdge sh_e[CLEAR_EDGE_CHUNK];
    __shared__ double sh_box[4][CWAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    int64_t lo = 0, hi = n;                    // the last field whose tiles start at or before this one: the one that owns it
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (tile_off[mid] <= tile) lo = mid; else hi = mid;
    }
    const int64_t i = lo, s0 = soff[i], m = soff[i + 1] - s0;
    // (the host has checked the offsets; a field without a block has no tile.  Uniform over the workgroup: nobody is left at a barrier)
    if (tile >= tile_off[i + 1] || m <= 0 || m > ROUTE_MAX_SWATHS || toff[i + 1] - toff[i] != route_block(m)) return;
    const int N = (int)(2 * m);
    const int64_t e = (tile - tile_off[i]) * CLEAR_TILE + tid;
    const bool have = e < (int64_t)N * N;
    const int p = have ? (int)(e / N) : 0, q = have ? (int)(e - (int64_t)p * N) : 0;
    const bool canon = have && route_canonical(p, q, N), pair = canon && (p >> 1) != (q >> 1);

    ClearPiece pc[NSEG];
    ClearBox box = { 0.0, 0.0, 0.0, 0.0 };
    double sx = 0.0, sy = 0.0, total = INFINITY;
    bool solved = false;
#pragma unroll
    for (int k = 0; k < NSEG; ++k) {
        pc[k].px = pc[k].py = pc[k].qx = pc[k].qy = pc[k].cx = pc[k].cy = pc[k].s0 = pc[k].len = 0.0;
        pc[k].kind = CLEAR_NONE;
        pc[k].wide = false;
    }
    if (pair) {
        double h0, x1, y1, h1, seg[NSEG];
        int word;
        route_pose(ax + s0, ay + s0, bx + s0, by + s0, angle[i], p, true, sx, sy, h0);
        route_pose(ax + s0, ay + s0, bx + s0, by + s0, angle[i], q, false, x1, y1, h1);
        Conn<MODE>::solve(sx, sy, h0, x1, y1, h1, R, word, seg, total);
        solved = clear_pieces<MODE>(sx, sy, h0, R, word, seg, pc, box);
    }
    const bool walk = pair && solved;

    // the field's rings: sizes first, the vertices as they are staged
    const int64_t r0 = F.ring_off[i], r1 = F.ring_off[i + 1];
    int bad = r1 <= r0 ? 1 : 0;
    for (int64_t r = r0 + tid; r < r1; r += CBLOCK)
        if (F.vert_off[r + 1] - F.vert_off[r] < 3) bad = 1;
    const int64_t v_lo = r1 > r0 ? F.vert_off[r0] : 0, v_hi = r1 > r0 ? F.vert_off[r1] : 0;
    ClearAcc acc = clear_begin();
    for (int64_t c0 = v_lo; c0 < v_hi; c0 += CLEAR_EDGE_CHUNK) {
        const int cnt = (int)(v_hi - c0 < CLEAR_EDGE_CHUNK ? v_hi - c0 : CLEAR_EDGE_CHUNK);
        double bx0 = INFINITY, by0 = INFINITY, bx1 = -INFINITY, by1 = -INFINITY;
        __syncthreads();                       // (the chunk before has been read by everybody)
        if (tid < cnt) {
            const int64_t v = c0 + tid;
            int64_t a = r0, b = r1;            // the last ring that starts at or before v: the one that holds it
            while (b - a > 1) {
                const int64_t mid = a + (b - a) / 2;
                if (F.vert_off[mid] <= v) a = mid; else b = mid;
            }
            const int64_t w = v + 1 < F.vert_off[a + 1] ? v + 1 : F.vert_off[a];
            const double x0 = F.x[v], y0 = F.y[v], x1 = F.x[w], y1 = F.y[w];
            if (!clear_vertex_ok(x0, y0)) bad = 1;
            sh_e[tid] = { x0, y0, x1, y1, x1 - x0, y1 - y0 };
            bx0 = fmin(x0, x1); bx1 = fmax(x0, x1);
            by0 = fmin(y0, y1); by1 = fmax(y0, y1);
        }
        bx0 = wave_min(bx0); by0 = wave_min(by0); bx1 = wave_max(bx1); by1 = wave_max(by1);
        if (lane == 0) { sh_box[0][wave] = bx0; sh_box[1][wave] = by0; sh_box[2][wave] = bx1; sh_box[3][wave] = by1; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < CWAVES; ++w) {
            bx0 = fmin(bx0, sh_box[0][w]); by0 = fmin(by0, sh_box[1][w]);
            bx1 = fmax(bx1, sh_box[2][w]); by1 = fmax(by1, sh_box[3][w]);
        }
        // (grown by far more than the rounding of e and of a hit: a skipped edge could not have counted)
        const double grow = 0x1p-30 * (fmax(fmax(fabs(bx0), fabs(bx1)), fmax(fabs(by0), fabs(by1))) + R);
        bx0 -= grow; by0 -= grow; bx1 += grow; by1 += grow;
        const bool meets = !(box.x1 < bx0 || box.x0 > bx1 || box.y1 < by0 || box.y0 > by1);
        const bool ray = sy >= by0 && sy <= by1 && sx <= bx1;
        if (walk && (meets || ray))
            for (int j = 0; j < cnt; ++j) {
                const ClearEdge ed = sh_e[j];
                clear_edge<NSEG>(pc, sx, sy, R, ed.x0, ed.y0, ed.x1, ed.y1, ed.ex, ed.ey, acc);
            }
    }
    const bool valid = __syncthreads_or(bad) == 0;
    const ClearResult res = clear_finish(solved, valid, acc);
    const bool blocked = pair && !res.clear;
    if constexpr (PRICED) {
        // (every lane of the wavefront: a lane that owns no pair lists nothing.  inside != 0 says solved and valid as well)
        solve_clear_append(blocked && res.inside != 0, toff[i] + e, list, count);
    }
    if (!canon) return;
    double *Tb = T + toff[i];
    const int64_t e2 = (int64_t)(q ^ 1) * N + (p ^ 1);
    if constexpr (PRICED) {
        const double v = blocked ? total + penalty : total;          // (within one swath: total is still the +inf it was set to)
        Tb[e] = v;
        Tb[e2] = v;
        if (B) {
            B[toff[i] + e] = blocked ? 0xff : 0;
            B[toff[i] + e2] = blocked ? 0xff : 0;
        }
    } else {
        uint8_t *Bb = B + toff[i];
        Bb[e] = blocked ? 1 : 0;
        Bb[e2] = blocked ? 1 : 0;
        if (blocked) {
            const double v = Tb[e] + penalty;
            Tb[e] = v;
            Tb[e2] = v;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(CBLOCK) void k_clear_conn(int64_t n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                       const double *__restrict__ fh, double R, const int32_t *__restrict__ word,
                                                       const double *__restrict__ seg, const int64_t *__restrict__ pair_field, ClearFields F,
                                                       int32_t *__restrict__ crossings, int8_t *__restrict__ inside,
                                                       double *__restrict__ first_s)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    const int64_t i = (int64_t)blockIdx.x * CBLOCK + threadIdx.x;
    if (i >= n) return;
    double sg[NSEG];
#pragma unroll
    for (int k = 0; k < NSEG; ++k) sg[k] = seg[i * NSEG + k];
    const ClearResult r = clear_path<MODE>(F, pair_field[i], fx[i], fy[i], fh[i], R, word[i], sg);
    if (crossings) crossings[i] = r.crossings;
    if (inside) inside[i] = r.inside;
    if (first_s) first_s[i] = r.first_s;
}

__global__ __launch_bounds__(CBLOCK) void k_clear_field_status(ClearFields F, int32_t *__restrict__ status)
{
    const int64_t f = (int64_t)blockIdx.x * CBLOCK + threadIdx.x;
    if (f < F.n) status[f] = clear_field_status(F, f);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_clear_field_status(hipStream_t st, const ClearFields &F, int32_t *status)
{
    if (F.n <= 0 || !status) return 0;
    return launch(st, k_clear_field_status, blocks_for(F.n, CBLOCK), CBLOCK, F, status);
}

int launch_clear_conn(hipStream_t st, int mode, int64_t n, const double *fx, const double *fy, const double *fh, double R, const int32_t *word,
                      const double *seg, const int64_t *pair_field, const ClearFields &F, int32_t *crossings, int8_t *inside, double *first_s)
{
    if (n <= 0 || (!crossings && !inside && !first_s)) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_clear_conn<M()>, blocks_for(n, CBLOCK), CBLOCK, n, fx, fy, fh, R, word, seg, pair_field, F, crossings, inside, first_s);
    });
}

int launch_clear_transit(hipStream_t st, int64_t n, const int64_t *soff, const double *ax, const double *ay, const double *bx, const double *by,
                         const double *angle, double R, int mode, const int64_t *toff, const int64_t *tile_off, int64_t n_tiles,
                         const ClearFields &F, double penalty, double *T, uint8_t *B)
{
    if (n <= 0 || n_tiles <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_clear_transit<M(), false>, (unsigned)n_tiles, CBLOCK, n, soff, ax, ay, bx, by, angle, R, toff, tile_off, F, penalty, T, B,
                      nullptr, nullptr);
    });
}

int launch_route_priced_first(hipStream_t st, int64_t n, const int64_t *soff, const double *ax, const double *ay, const double *bx,
                              const double *by, const double *angle, double R, int mode, const int64_t *toff, const int64_t *tile_off,
                              int64_t n_tiles, const ClearFields &F, double penalty, double *T, int8_t *K, int64_t *list, unsigned long long *count)
{
    if (n <= 0 || n_tiles <= 0) return 0;
    uint8_t *B = reinterpret_cast<uint8_t *>(K);
    return by_mode(mode, [&](auto M) {
        return launch(st, k_clear_transit<M(), true>, (unsigned)n_tiles, CBLOCK, n, soff, ax, ay, bx, by, angle, R, toff, tile_off, F, penalty, T, B,
                      list, count);
    });
}

}  // namespace fcpp
