// fcpp_inset.hip -- gfx950 (MI355X) kernels of the polygon inset: k_inset<.., false> (n fields x D distances: ring count, vertex count,
// status and gap of every pair -- the counting pass) and k_inset<.., true> (the rings at the CSR offsets the project's workgroup scan made of
// the counts).  The rule is ONE set of host+device expressions, fcpp_insetfn.h; float64, -ffp-contract=off like every other translation
// unit, so the kernels give the bits fcpp_debug_inset gives on the host.
//
// Mapping.  A workgroup takes a (field, distance) pair.  The field's vertices go to LDS, a lane per vertex; a lane per RING orients it (the
// shoelace sum in the rule's order, the reversal in place); a lane per edge adds unit direction and length: 40 bytes an edge.  The 2 E
// primitives are dealt to the lanes in contiguous runs, so that the pieces of a lane are consecutive in the rule's numbering.  A lane sweeps
// its primitive forward through ALL edges (every lane reads the same edge: an LDS broadcast) to count its pieces, keeping the first four in
// registers; after the workgroup's scan has given it its first number it stores them -- start, end, parameters, primitive -- and only a
// lane with more than four sweeps once more.  No lane keeps removed intervals; count and fill run the same sweep, hence the same pieces in
// the same order with the same bits.  Then a lane per piece
// finds its successor among all piece starts, lane 0 walks the rings through LDS (succ and the vertex offsets), and in the fill a lane
// per piece writes its vertices.  Plain vector stores only.
// Two shapes: fields of up to 64 edges -- the headland of a surveyed boundary -- run as ONE wavefront with the piece records in LDS too
// (18 KB a workgroup); larger ones, up to 1024 edges, as four wavefronts with 66 KB of LDS and the piece records in a slab of device memory
// a launch of at most 1024 pairs owns.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_inset.h"
#include "fcpp_insetfn.h"
#include "fcpp_launch.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int IBLOCK = 256;          // the offsets scan

// exclusive scan of v over the workgroup; total in every lane
template <int BLOCK>
__device__ __forceinline__ int inset_block_scan(int v, int32_t *s_scan, int &total)
{
    constexpr int NWAVE = BLOCK / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int pv = __shfl_up(inc, o);
        if (lane >= o) inc += pv;
    }
    if (lane == 63) s_scan[wave] = inc;
    __syncthreads();
    int pre = 0;
    total = 0;
    for (int w = 0; w < NWAVE; ++w) { if (w < wave) pre += s_scan[w]; total += s_scan[w]; }
    __syncthreads();
    return pre + inc - v;
}

// One (field, distance) pair by one workgroup.  FILL: also the rings, inside [ring0, ring1) and [v_lo, v_hi) only.
template <int BLOCK, int MAXE, bool LDSP, bool FILL>
__global__ __launch_bounds__(BLOCK) void k_inset(int64_t pair0, int64_t n_pairs, int64_t D, const int64_t *__restrict__ ring_offsets,
                                                 const int64_t *__restrict__ vert_offsets, const double *__restrict__ x,
                                                 const double *__restrict__ y, const double *__restrict__ dist, double arc_step,
                                                 double *scratch_d, int32_t *scratch_i, int32_t *__restrict__ n_rings,
                                                 int32_t *__restrict__ n_verts, int32_t *__restrict__ status, double *__restrict__ gap,
                                                 const int64_t *__restrict__ pair_ring_offsets, const int64_t *__restrict__ pair_vert_offsets,
                                                 int64_t total_rings, int64_t total_verts, int64_t *__restrict__ out_vert_offsets,
                                                 double *__restrict__ out_x, double *__restrict__ out_y, int32_t *__restrict__ out_src)
{
    constexpr int MAXP = INSET_PIECES_PER_EDGE * MAXE, NWAVE = BLOCK / 64;
    __shared__ double s_px[MAXE], s_py[MAXE], s_ux[MAXE], s_uy[MAXE], s_len[MAXE];
    __shared__ uint16_t s_nxt[MAXE], s_succ[MAXP];
    __shared__ int32_t s_pos[MAXP];
    __shared__ double s_pc[LDSP ? 6 * MAXP : 1];
    __shared__ int32_t s_pi[LDSP ? MAXP : 1];
    __shared__ int32_t s_scan[NWAVE];
    __shared__ double s_red[NWAVE];
    __shared__ int32_t s_out[3];

    const int tid = threadIdx.x;
    const int64_t pair = pair0 + blockIdx.x;
    if (pair >= n_pairs) return;
    const int64_t i = pair / D, j = pair - i * D;
    int64_t ring0 = 0, ring1 = 0, v_lo = 0, v_hi = 0;
    if (FILL) {
        if (pair == n_pairs - 1 && tid == 0 && out_vert_offsets) out_vert_offsets[total_rings] = total_verts;
        ring0 = pair_ring_offsets[pair]; ring1 = pair_ring_offsets[pair + 1];
        v_lo = pair_vert_offsets[pair]; v_hi = pair_vert_offsets[pair + 1];
        if (ring1 <= ring0 || ring0 < 0 || ring1 > total_rings || v_lo < 0 || v_hi > total_verts) return;      // nothing to write: empty, or a status
    }
    const double d = dist[j];
    const int64_t r0 = ring_offsets[i], r1 = ring_offsets[i + 1];
    // validity
    int bad = r1 <= r0;
    for (int64_t r = r0 + tid; r < r1; r += BLOCK) bad |= vert_offsets[r + 1] - vert_offsets[r] < 3;
    const int64_t v0 = r1 > r0 ? vert_offsets[r0] : 0, v1 = r1 > r0 ? vert_offsets[r1] : 0;
    for (int64_t v = v0 + tid; v < v1; v += BLOCK) bad |= !inset_finite(x[v]) || !inset_finite(y[v]);
    bad = __syncthreads_or(bad);
    int st = bad ? INSET_EINVAL : (v1 - v0 > INSET_MAX_EDGES || v1 - v0 > MAXE ? INSET_EUNSUPPORTED : INSET_OK);
    const int E = st == INSET_OK ? (int)(v1 - v0) : 0;
    constexpr int KEEP = 4;               // pieces a lane keeps in registers between the counting sweep and the store
    int P = 0, at = 0, cnt = 0;           // the field's pieces, the number of this lane's first, this lane's pieces
    double kt0[KEEP] = { 0.0, 0.0, 0.0, 0.0 }, kt1[KEEP] = { 0.0, 0.0, 0.0, 0.0 };
    int kq[KEEP] = { 0, 0, 0, 0 };
    double gmax = 0.0;
    double *const pc = LDSP ? s_pc : scratch_d + (size_t)blockIdx.x * 6 * MAXP;
    int32_t *const pi = LDSP ? s_pi : scratch_i + (size_t)blockIdx.x * MAXP;
    double *const sx = pc, *const sy = pc + MAXP, *const ex = pc + 2 * MAXP, *const ey = pc + 3 * MAXP, *const t0s = pc + 4 * MAXP,
                 *const t1s = pc + 5 * MAXP;
    const InsetEdges e = { s_px, s_py, s_ux, s_uy, s_len, s_nxt, E };
    if (st == INSET_OK) {                                                                   // (uniform)
        for (int v = tid; v < E; v += BLOCK) { s_px[v] = x[v0 + v]; s_py[v] = y[v0 + v]; }
        __syncthreads();
        for (int64_t r = r0 + tid; r < r1; r += BLOCK) {
            const int base = (int)(vert_offsets[r] - v0), m = (int)(vert_offsets[r + 1] - vert_offsets[r]);
            inset_orient_ring(s_px + base, s_py + base, s_nxt + base, base, m, r == r0);
        }
        __syncthreads();
        for (int g = tid; g < E; g += BLOCK) {
            const int h = s_nxt[g];
            inset_edge(s_px[g], s_py[g], s_px[h], s_py[h], s_ux[g], s_uy[g], s_len[g]);
        }
        __syncthreads();
        // the pieces: count, scan, store
        const int run = (2 * E + BLOCK - 1) / BLOCK, q0 = tid * run, q1 = min(2 * E, q0 + run);
        int over = 0;
        for (int q = q0; q < q1; ++q) {
            InsetPrim p;
            if (!inset_prim(e, q, d, p)) continue;
            double from = 0.0, t0, t1;
            while (inset_next_piece(e, p, d, from, t0, t1)) {
                from = t1;
                if (!inset_piece_kept(p, d, t0, t1)) continue;
                over |= inset_piece_verts(p, t0, t1, arc_step) == 0;
#pragma unroll
                for (int c = 0; c < KEEP; ++c)
                    if (cnt == c) { kt0[c] = t0; kt1[c] = t1; kq[c] = q; }
                ++cnt;
            }
        }
        at = inset_block_scan<BLOCK>(cnt, s_scan, P);
        over = __syncthreads_or(over);
        if (over || P > INSET_PIECES_PER_EDGE * E) { st = INSET_EUNSUPPORTED; P = 0; }
    }
    if (st == INSET_OK) {                                                                   // (uniform)
        const auto store = [&](int k, const InsetPrim &p, int q, double t0, double t1) {
            if (k >= P || k >= MAXP) return;
            double ax, ay, bx, by;
            inset_point(p, d, t0, ax, ay);
            inset_point(p, d, t1, bx, by);
            sx[k] = ax; sy[k] = ay; ex[k] = bx; ey[k] = by;
            t0s[k] = t0; t1s[k] = t1;
            pi[k] = q;
            s_pos[k] = -inset_piece_verts(p, t0, t1, arc_step);
        };
        if (cnt <= KEEP) {
            // the lane still holds its pieces from the counting sweep
#pragma unroll
            for (int c = 0; c < KEEP; ++c)
                if (c < cnt) {
                    InsetPrim p;
                    (void)inset_prim(e, kq[c], d, p);
                    store(at + c, p, kq[c], kt0[c], kt1[c]);
                }
        } else {
            // more than it could hold: the same sweep again
            const int run = (2 * E + BLOCK - 1) / BLOCK, q0 = tid * run, q1 = min(2 * E, q0 + run);
            for (int q = q0; q < q1; ++q) {
                InsetPrim p;
                if (!inset_prim(e, q, d, p)) continue;
                double from = 0.0, t0, t1;
                while (inset_next_piece(e, p, d, from, t0, t1)) {
                    from = t1;
                    if (!inset_piece_kept(p, d, t0, t1)) continue;
                    store(at, p, q, t0, t1);
                    ++at;
                }
            }
        }
        __syncthreads();
        // successors and the gap
        for (int k = tid; k < P; k += BLOCK) {
            double d2;
            s_succ[k] = (uint16_t)inset_succ(sx, sy, P, ex[k], ey[k], d2);
            gmax = fmax(gmax, d2);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o));
        if ((tid & 63) == 0) s_red[tid >> 6] = gmax;
        __syncthreads();
        if (tid == 0) {
            int32_t R = 0, V = 0;
            const int ws = inset_walk(P, s_succ, s_pos, R, V, [&](int32_t r, int32_t off) {
                if (FILL && out_vert_offsets && ring0 + r < ring1) out_vert_offsets[ring0 + r] = v_lo + off;
            });
            s_out[0] = ws; s_out[1] = R; s_out[2] = V;
        }
        __syncthreads();
        st = s_out[0];
    }
    if (!FILL) {
        if (tid != 0) return;
        double g = 0.0;
        if (st == INSET_OK)
            for (int w = 0; w < NWAVE; ++w) g = fmax(g, s_red[w]);
        if (n_rings) n_rings[pair] = st == INSET_OK ? s_out[1] : 0;
        if (n_verts) n_verts[pair] = st == INSET_OK ? s_out[2] : 0;
        if (status) status[pair] = st;
        if (gap) gap[pair] = sqrt(g);
        return;
    }
    if (st != INSET_OK) return;
    for (int k = tid; k < P; k += BLOCK) {
        const int q = pi[k];
        const int32_t first = s_pos[k];
        InsetPrim p;
        if (first < 0 || !inset_prim(e, q, d, p)) continue;
        const double t0 = t0s[k], t1 = t1s[k];
        const int m = inset_piece_verts(p, t0, t1, arc_step);
        for (int a = 0; a < m; ++a) {
            const int64_t at = v_lo + first + a;
            if (at >= v_hi) break;
            double vx, vy;
            inset_piece_vertex(p, d, t0, t1, m, a, vx, vy);
            if (out_x) out_x[at] = vx;
            if (out_y) out_y[at] = vy;
            if (out_src) out_src[at] = q;
        }
    }
}

// the count of pair p for the workgroup scan of fcpp_samplefn.h
struct InsetCount {
    const int32_t *counts;
    __device__ int64_t operator()(int64_t p, int64_t &) const { return counts[p]; }
};

// ---- launchers --------------------------------------------------------------------------------------------------------------------
void inset_scratch_size(int max_edges, int64_t n_pairs, size_t &doubles, size_t &ints)
{
    doubles = ints = 0;
    if (max_edges <= INSET_SMALL_EDGES || n_pairs <= 0) return;
    const size_t slabs = (size_t)(n_pairs < INSET_LAUNCH_PAIRS ? n_pairs : INSET_LAUNCH_PAIRS), pieces = (size_t)INSET_PIECES_PER_EDGE * INSET_MAX_EDGES;
    doubles = slabs * 6 * pieces;
    ints = slabs * pieces;
}

template <bool FILL>
static int inset_launch(hipStream_t st, int64_t n, int64_t D, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets,
                        const double *x, const double *y, const double *dist, double arc_step, double *scratch_d, int32_t *scratch_i,
                        int32_t *n_rings, int32_t *n_verts, int32_t *status, double *gap, const int64_t *pair_ring_offsets,
                        const int64_t *pair_vert_offsets, int64_t total_rings, int64_t total_verts, int64_t *out_vert_offsets, double *out_x,
                        double *out_y, int32_t *out_src)
{
    if (n <= 0 || D <= 0) return 0;
    const int64_t n_pairs = n * D;
    if (max_edges <= INSET_SMALL_EDGES) {
        return launch(st, k_inset<64, INSET_SMALL_EDGES, true, FILL>, (unsigned)n_pairs, 64, (int64_t)0, n_pairs, D, ring_offsets, vert_offsets, x, y,
                      dist, arc_step, scratch_d, scratch_i, n_rings, n_verts, status, gap, pair_ring_offsets, pair_vert_offsets, total_rings,
                      total_verts, out_vert_offsets, out_x, out_y, out_src);
    }
    if (!scratch_d || !scratch_i) return (int)hipErrorInvalidValue;
    // (launches on one stream run one after another: the slabs of a launch are free when the next one starts)
    for (int64_t pair0 = 0; pair0 < n_pairs; pair0 += INSET_LAUNCH_PAIRS) {
        const int64_t m = n_pairs - pair0 < INSET_LAUNCH_PAIRS ? n_pairs - pair0 : INSET_LAUNCH_PAIRS;
        if (int e = launch(st, k_inset<256, INSET_MAX_EDGES, false, FILL>, (unsigned)m, 256, pair0, n_pairs, D, ring_offsets, vert_offsets, x, y,
                           dist, arc_step, scratch_d, scratch_i, n_rings, n_verts, status, gap, pair_ring_offsets, pair_vert_offsets, total_rings,
                           total_verts, out_vert_offsets, out_x, out_y, out_src)) return e;
    }
    return 0;
}

int launch_inset_count(hipStream_t st, int64_t n, int64_t D, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets,
                       const double *x, const double *y, const double *dist, double arc_step, double *scratch_d, int32_t *scratch_i,
                       int32_t *n_rings, int32_t *n_verts, int32_t *status, double *gap)
{
    return inset_launch<false>(st, n, D, max_edges, ring_offsets, vert_offsets, x, y, dist, arc_step, scratch_d, scratch_i, n_rings, n_verts, status,
                               gap, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr);
}

int launch_inset_offsets(hipStream_t st, int64_t m, const int32_t *counts, int64_t *out_offsets, int64_t *err)
{
    return launch_path_counts<IBLOCK>(st, m, InsetCount{ counts }, out_offsets, err);
}

int launch_inset_fill(hipStream_t st, int64_t n, int64_t D, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets,
                      const double *x, const double *y, const double *dist, double arc_step, double *scratch_d, int32_t *scratch_i,
                      const int64_t *pair_ring_offsets, const int64_t *pair_vert_offsets, int64_t total_rings, int64_t total_verts,
                      int64_t *out_vert_offsets, double *out_x, double *out_y, int32_t *out_src)
{
    if ((n <= 0 || D <= 0) && out_vert_offsets && total_rings == 0) {
        const int64_t zero = 0;
        const hipError_t e = hipMemcpyAsync(out_vert_offsets, &zero, sizeof zero, hipMemcpyHostToDevice, st);
        return e == hipSuccess ? (int)hipStreamSynchronize(st) : (int)e;
    }
    return inset_launch<true>(st, n, D, max_edges, ring_offsets, vert_offsets, x, y, dist, arc_step, scratch_d, scratch_i, nullptr, nullptr, nullptr,
                              nullptr, pair_ring_offsets, pair_vert_offsets, total_rings, total_verts, out_vert_offsets, out_x, out_y, out_src);
}

}  // namespace fcpp
