// fcpp_cells.hip -- gfx950 (MI355X) kernels of the field cells: k_cells<.., false> (per field: cell count, vertex count, status, cuts and
// what min_area dropped -- the counting pass) and k_cells<.., true> (the cells at the CSR offsets the project's workgroup scan made of the
// counts).  The rule is ONE set of host+device expressions, fcpp_cellfn.h; float64, -ffp-contract=off like every other translation unit, so
// the kernels give the bits fcpp_debug_cells gives on the host.
//
// Mapping.  A workgroup takes a field, as in k_inset.  A lane per vertex checks it and puts its frame coordinates into LDS; a lane per RING
// orients it (shoelace sum, depth by the crossing test against the other rings); a lane per vertex shoots its two rays through ALL edges
// (every lane reads the same edge: an LDS broadcast).  Lane 0 numbers pieces, new nodes and cuts in the rule's order (a pass over 2 E rays);
// a lane per node places its boundary piece, a lane per half-edge finds its successor, lane 0 walks the cells through LDS, a lane per cell
// sums its area, lane 0 adds the totals up in cell order, and in the fill a lane per cell writes its vertices.  Count and fill run the same
// steps, hence the same cells in the same order with the same bits.  Plain vector stores only.
// Two shapes: fields of up to 64 edges -- a surveyed boundary's work area between its arcs -- run as ONE wavefront with 8 KB of LDS; larger
// ones, up to 1024 edges, as four wavefronts with 126 KB.  Every table of the rule (frame, links, 3 E nodes, 7 E half-edges, 2 E + 1 cells)
// fits in LDS, so no launch owns device memory of its own and a launch takes the whole batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_cellfn.h"
#include "fcpp_cells.h"
#include "fcpp_launch.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int CBLOCK = 256;          // the offsets scan

// One field by one workgroup.  FILL: also the cells, inside [cell0, cell1) and [v_lo, v_hi) only.
template <int BLOCK, int MAXE, bool FILL>
__global__ __launch_bounds__(BLOCK) void k_cells(int64_t n, const int64_t *__restrict__ ring_offsets, const int64_t *__restrict__ vert_offsets,
                                                 const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ angle,
                                                 int events, double min_area, int32_t *__restrict__ n_cells, int32_t *__restrict__ n_verts,
                                                 int32_t *__restrict__ status, int32_t *__restrict__ n_cuts, int32_t *__restrict__ dropped,
                                                 double *__restrict__ dropped_area, const int64_t *__restrict__ cell_offsets,
                                                 const int64_t *__restrict__ fvert_offsets, int64_t total_cells, int64_t total_verts,
                                                 int64_t *__restrict__ out_vert_offsets, double *__restrict__ out_x, double *__restrict__ out_y,
                                                 int32_t *__restrict__ out_src, int32_t *__restrict__ cell_field, double *__restrict__ out_area)
{
    constexpr int MAXN = CELL_NODES_PER_EDGE * MAXE, MAXH = CELL_HALF_PER_EDGE * MAXE, MAXC = 2 * MAXE + 1;
    __shared__ double s_u[MAXE], s_w[MAXE], s_area[MAXC];
    __shared__ int32_t s_ray[2 * MAXE];
    __shared__ uint16_t s_nxt[MAXE], s_prv[MAXE], s_org[MAXH], s_succ[MAXH], s_pos[MAXH], s_bout[MAXN], s_cutp[MAXN], s_cutm[MAXN];
    __shared__ uint16_t s_nray[2 * MAXE], s_ebase[MAXE + 1], s_cfirst[MAXC], s_clen[MAXC], s_cout[MAXC], s_cvoff[MAXC];
    __shared__ CellCounts s_n;
    __shared__ CellTotals s_t;
    __shared__ int32_t s_cells;

    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    int64_t cell0 = 0, cell1 = 0, v_lo = 0, v_hi = 0;
    if (FILL) {
        if (i == n - 1 && tid == 0 && out_vert_offsets) out_vert_offsets[total_cells] = total_verts;
        cell0 = cell_offsets[i]; cell1 = cell_offsets[i + 1];
        v_lo = fvert_offsets[i]; v_hi = fvert_offsets[i + 1];
        if (cell1 <= cell0 || cell0 < 0 || cell1 > total_cells || v_lo < 0 || v_hi > total_verts) return;      // nothing to write: empty, or a status
    }
    double sn, cs;
    fc_sincos(angle[i], sn, cs);
    const int64_t r0 = ring_offsets[i], r1 = ring_offsets[i + 1];
    // validity
    int bad = r1 <= r0;
    for (int64_t r = r0 + tid; r < r1; r += BLOCK) {
        const int64_t a = vert_offsets[r], m = vert_offsets[r + 1] - a;
        bad |= m < 3 || cell_ring_zero_edge(x + a, y + a, m);
    }
    const int64_t v0 = r1 > r0 ? vert_offsets[r0] : 0, v1 = r1 > r0 ? vert_offsets[r1] : 0;
    for (int64_t v = v0 + tid; v < v1; v += BLOCK) {
        double u, w;
        swath_uw(x[v], y[v], cs, sn, u, w);
        bad |= !swath_finite(x[v]) || !swath_finite(y[v]) || !swath_finite(u) || !swath_finite(w);
    }
    bad = __syncthreads_or(bad);
    int st = bad ? CELL_EINVAL : (v1 - v0 > CELL_MAX_EDGES || v1 - v0 > MAXE ? CELL_EUNSUPPORTED : CELL_OK);
    const int E = st == CELL_OK ? (int)(v1 - v0) : 0;
    CellView f;
    f.x = x + v0; f.y = y + v0; f.u = s_u; f.w = s_w; f.nxt = s_nxt; f.prv = s_prv; f.ray = s_ray; f.org = s_org; f.succ = s_succ; f.pos = s_pos;
    f.bout = s_bout; f.cutp = s_cutp; f.cutm = s_cutm; f.nray = s_nray; f.ebase = s_ebase; f.cfirst = s_cfirst; f.clen = s_clen; f.cout = s_cout;
    f.cvoff = s_cvoff; f.area = s_area; f.E = E; f.c = cs; f.s = sn;
    if (st == CELL_OK) {                                                                    // (uniform)
        for (int v = tid; v < E; v += BLOCK) swath_uw(f.x[v], f.y[v], cs, sn, s_u[v], s_w[v]);
        for (int k = tid; k < CELL_NODES_PER_EDGE * E; k += BLOCK) s_cutp[k] = s_cutm[k] = CELL_NONE;
        for (int k = tid; k < CELL_HALF_PER_EDGE * E; k += BLOCK) s_pos[k] = CELL_NONE;
        __syncthreads();
        for (int64_t r = r0 + tid; r < r1; r += BLOCK) cell_orient_ring(f, vert_offsets, r0, r1, r);
        __syncthreads();
        for (int v = tid; v < E; v += BLOCK) cell_rays(f, v, events);
        __syncthreads();
        if (tid == 0) {
            CellCounts c = { 0, 0, 0, 0 };
            s_t.status = cell_number(f, c);
            s_n = c;
        }
        __syncthreads();
        st = s_t.status;
    }
    CellCounts cn = { 0, 0, 0, 0 };
    if (st == CELL_OK) {                                                                    // (uniform)
        cn = s_n;
        for (int X = tid; X < E + cn.J; X += BLOCK) cell_place_node(f, cn.J, X);
        __syncthreads();
        for (int h = tid; h < cn.H; h += BLOCK) s_succ[h] = (uint16_t)cell_succ(f, cn, h);
        __syncthreads();
        if (tid == 0) {
            int C = 0;
            s_t.status = cell_walk(f, cn.H, C);
            s_cells = C;
        }
        __syncthreads();
        st = s_t.status;
    }
    if (st == CELL_OK) {                                                                    // (uniform)
        const int C = s_cells;
        for (int c = tid; c < C; c += BLOCK) s_area[c] = cell_area(f, c);
        __syncthreads();
        if (tid == 0) {
            CellTotals t = { CELL_OK, 0, 0, cn.K, 0, 0.0 };
            cell_totals(f, C, min_area, t);
            s_t = t;
        }
        __syncthreads();
    }
    if (!FILL) {
        if (tid != 0) return;
        const bool ok = st == CELL_OK;
        n_cells[i] = ok ? s_t.n_cells : 0;
        n_verts[i] = ok ? s_t.n_verts : 0;
        if (status) status[i] = st;
        if (n_cuts) n_cuts[i] = ok ? s_t.n_cuts : 0;
        if (dropped) dropped[i] = ok ? s_t.dropped : 0;
        if (dropped_area) dropped_area[i] = ok ? s_t.dropped_area : 0.0;
        return;
    }
    if (st != CELL_OK) return;
    for (int c = tid; c < s_cells; c += BLOCK) {
        if (s_cout[c] == CELL_NONE) continue;
        const int64_t ci = cell0 + s_cout[c], first = v_lo + s_cvoff[c];
        if (ci >= cell1) continue;
        if (out_vert_offsets) out_vert_offsets[ci] = first;
        if (cell_field) cell_field[ci] = (int32_t)i;
        if (out_area) out_area[ci] = s_area[c];
        int h = s_cfirst[c];
        for (int a = 0; a < s_clen[c]; ++a, h = s_succ[h]) {
            const int64_t at = first + a;
            if (at >= v_hi) break;
            double vx, vy;
            cell_node_xy(f, s_org[h], vx, vy);
            if (out_x) out_x[at] = vx;
            if (out_y) out_y[at] = vy;
            if (out_src) out_src[at] = cell_vertex_src(f, cn, h);
        }
    }
}

// the count of field i for the workgroup scan of fcpp_samplefn.h
struct CellCount {
    const int32_t *counts;
    __device__ int64_t operator()(int64_t p, int64_t &) const { return counts[p]; }
};

// ---- launchers --------------------------------------------------------------------------------------------------------------------
template <bool FILL>
static int cells_launch(hipStream_t st, int64_t n, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x,
                        const double *y, const double *angle, int events, double min_area, int32_t *n_cells, int32_t *n_verts, int32_t *status,
                        int32_t *n_cuts, int32_t *dropped, double *dropped_area, const int64_t *cell_offsets, const int64_t *fvert_offsets,
                        int64_t total_cells, int64_t total_verts, int64_t *out_vert_offsets, double *out_x, double *out_y, int32_t *out_src,
                        int32_t *cell_field, double *area)
{
    if (n <= 0) return 0;
    if (max_edges <= CELL_SMALL_EDGES)
        return launch(st, k_cells<64, CELL_SMALL_EDGES, FILL>, (unsigned)n, 64, n, ring_offsets, vert_offsets, x, y, angle, events, min_area, n_cells,
                      n_verts, status, n_cuts, dropped, dropped_area, cell_offsets, fvert_offsets, total_cells, total_verts, out_vert_offsets, out_x,
                      out_y, out_src, cell_field, area);
    return launch(st, k_cells<256, CELL_MAX_EDGES, FILL>, (unsigned)n, 256, n, ring_offsets, vert_offsets, x, y, angle, events, min_area, n_cells,
                  n_verts, status, n_cuts, dropped, dropped_area, cell_offsets, fvert_offsets, total_cells, total_verts, out_vert_offsets, out_x, out_y,
                  out_src, cell_field, area);
}

int launch_cells_count(hipStream_t st, int64_t n, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x,
                       const double *y, const double *angle, int events, double min_area, int32_t *n_cells, int32_t *n_verts, int32_t *status,
                       int32_t *n_cuts, int32_t *dropped, double *dropped_area)
{
    return cells_launch<false>(st, n, max_edges, ring_offsets, vert_offsets, x, y, angle, events, min_area, n_cells, n_verts, status, n_cuts, dropped,
                               dropped_area, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int launch_cells_offsets(hipStream_t st, int64_t n, const int32_t *counts, int64_t *out_offsets, int64_t *err)
{
    return launch_path_counts<CBLOCK>(st, n, CellCount{ counts }, out_offsets, err);
}

int launch_cells_fill(hipStream_t st, int64_t n, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x,
                      const double *y, const double *angle, int events, double min_area, const int64_t *cell_offsets,
                      const int64_t *fvert_offsets, int64_t total_cells, int64_t total_verts, int64_t *out_vert_offsets, double *out_x,
                      double *out_y, int32_t *out_src, int32_t *cell_field, double *area)
{
    if (n <= 0 && out_vert_offsets && total_cells == 0) {
        const int64_t zero = 0;
        const hipError_t e = hipMemcpyAsync(out_vert_offsets, &zero, sizeof zero, hipMemcpyHostToDevice, st);
        return e == hipSuccess ? (int)hipStreamSynchronize(st) : (int)e;
    }
    return cells_launch<true>(st, n, max_edges, ring_offsets, vert_offsets, x, y, angle, events, min_area, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr, cell_offsets, fvert_offsets, total_cells, total_verts, out_vert_offsets, out_x, out_y, out_src,
                              cell_field, area);
}

}  // namespace fcpp
