// fcpp_pcover.hip -- gfx950 (MI355X) kernels of the polygon coverage report (include/fcpp.h: fcpp_polygon_cover_sizes, fcpp_polygon_cover).  The
// rule is ONE set of host+device expressions, fcpp_pcoverfn.h; float64, -ffp-contract=off like every other translation unit, so the kernels
// give the bits fcpp_debug_polygon_cover gives on the host.  Plain C++: no inline assembly, no float atomics, every loop bounded.
//
// k_pcover_sizes: a wavefront per field: the rings' sizes, the vertices' bounding box (lanes stride over them, a xor butterfly of min / max:
// exact in any order), then lane 0 writes the grid and the status.  The offsets of the fields' cells and tiles are the samplers' scan
// (fcpp_samplefn.h, as it is): one workgroup.
//
// k_pcover_boxes: a path is cut into chunks of PCOVER_CHUNK = 256 segments (the glue derives the chunk table from the host offsets); a
// workgroup per chunk, a lane per segment, writes the bounding box of the chunk's WORKING segments -- an inverted box, which no tile hits,
// when it has none (a connector, a run of NaN).
//
// k_pcover_tiles: a workgroup of 256 per 64 x 64 tile of cells, fcpp_cover.hip's layout: thread t owns column t & 63 and the rows
// (t >> 6) + 4 q, q = 0 .. 15.  The tile finds its field by bisection of the fields' first tiles.
//   phase 1, inside   the field's edges 256 at a time, one per thread (its ring by bisection of the field's few rings), culled against the
//                     tile's rows, the survivors compacted into LDS as (u, w) pairs; every thread flips the parity of its 16 cells.
//   phase 2, covered  the field's chunk boxes 256 at a time against the tile grown by `reach`: ONE ballot per wavefront; only the hit chunks
//                     are loaded, a lane per segment, culled against the grown tile, the survivors compacted into LDS with their pass and
//                     the two round-end flags; every thread tests its 16 cells.  A tile stops once all its cells are overlapped.
//   A tile's work grows with its field's sample count by one box test per chunk (32 B per 256 segments) and no more.
//   Grid bytes are plain stores, the four counts a workgroup reduction and one integer atomic each (order-independent).
// fp64 VALU-bound like k_cover: about 20 operations per (cell, surviving segment), one division per (cell, surviving edge).
// LDS 9.3 KiB (four float64 columns of 256, pass, flags, the ballots' words).  Registers and occupancy: DESIGN.md section 5.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_pcover.h"
#include "fcpp_pcoverfn.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int PBLOCK = 256;
static constexpr int PT = PCOVER_TILE;
static constexpr int PQ = PT * PT / PBLOCK;        // cells per thread

__global__ __launch_bounds__(PBLOCK) void k_pcover_sizes(int64_t n, const int64_t *__restrict__ roff, const int64_t *__restrict__ voff,
                                                         const double *__restrict__ x, const double *__restrict__ y, double W, double res,
                                                         PcoverDims *__restrict__ dims, int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * (PBLOCK / 64) + (threadIdx.x >> 6);
    if (f >= n) return;                         // (a whole wavefront: nothing below synchronises the workgroup)
    const int64_t r0 = roff[f], r1 = roff[f + 1];
    bool bad = r1 <= r0;
    double x_min = INFINITY, x_max = -INFINITY, y_min = INFINITY, y_max = -INFINITY;
    if (!bad) {
        for (int64_t r = r0 + lane; r < r1; r += 64) bad |= voff[r + 1] - voff[r] < 3;
        const int64_t v1 = voff[r1];
        for (int64_t v = voff[r0] + lane; v < v1; v += 64) {
            const double vx = x[v], vy = y[v];
            bad |= !swath_finite(vx) || !swath_finite(vy);
            x_min = vx < x_min ? vx : x_min; x_max = vx > x_max ? vx : x_max;
            y_min = vy < y_min ? vy : y_min; y_max = vy > y_max ? vy : y_max;
        }
    }
    bad = __ballot(bad) != 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a = __shfl_xor(x_min, o), b = __shfl_xor(x_max, o), c = __shfl_xor(y_min, o), d = __shfl_xor(y_max, o);
        x_min = a < x_min ? a : x_min; x_max = b > x_max ? b : x_max;
        y_min = c < y_min ? c : y_min; y_max = d > y_max ? d : y_max;
    }
    if (lane != 0) return;
    PcoverDims d = { 0.0, 0.0, 0, 0 };
    const int st = bad ? PCOVER_EINVAL : pcover_dims(x_min, x_max, y_min, y_max, W, res, d);
    dims[f] = d;
    if (status) status[f] = st;
}

struct PcoverCellCount {
    const PcoverDims *dims;
    __device__ int64_t operator()(int64_t f, int64_t &) const { return dims[f].nx * dims[f].ny; }
};
struct PcoverTileCount {
    const PcoverDims *dims;
    __device__ int64_t operator()(int64_t f, int64_t &) const { return ((dims[f].nx + PT - 1) / PT) * ((dims[f].ny + PT - 1) / PT); }
};

__global__ __launch_bounds__(PBLOCK) void k_pcover_boxes(int64_t n_chunks, const PcoverChunk *__restrict__ chunks, PcoverPaths P,
                                                         PcoverBox *__restrict__ boxes)
{
    __shared__ double s_box[PBLOCK / 64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PcoverChunk C = chunks[blockIdx.x];
    double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    if (tid < C.count) {
        double ax, ay, bx, by;
        int32_t pass;
        bool ja, jb;
        if (pcover_segment(P, C.path, C.p0, C.p1, C.first + tid, 1, ax, ay, bx, by, pass, ja, jb)) {
            x0 = fmin(ax, bx); x1 = fmax(ax, bx); y0 = fmin(ay, by); y1 = fmax(ay, by);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = fmin(x0, __shfl_xor(x0, o)); y0 = fmin(y0, __shfl_xor(y0, o));
        x1 = fmax(x1, __shfl_xor(x1, o)); y1 = fmax(y1, __shfl_xor(y1, o));
    }
    if (lane == 0) { s_box[wave][0] = x0; s_box[wave][1] = y0; s_box[wave][2] = x1; s_box[wave][3] = y1; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PBLOCK / 64; ++w) {
            x0 = fmin(x0, s_box[w][0]); y0 = fmin(y0, s_box[w][1]); x1 = fmax(x1, s_box[w][2]); y1 = fmax(y1, s_box[w][3]);
        }
        boxes[blockIdx.x] = { x0, y0, x1, y1 };
    }
}

// the compaction k_cover uses: the kept lanes' positions among the workgroup's, and their number (two barriers; s_wave is reused behind them)
__device__ __forceinline__ int pcover_compact(bool keep, int lane, int wave, int *s_wave, int &total)
{
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
    for (int w = 0; w < PBLOCK / 64; ++w) { if (w < wave) off += s_wave[w]; total += s_wave[w]; }
    return off + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(PBLOCK) void k_pcover_tiles(int64_t n, PcoverFields F, double W, double res, int caps,
                                                         const PcoverChunk *__restrict__ chunks, const PcoverBox *__restrict__ boxes, PcoverPaths P,
                                                         uint8_t *__restrict__ grid, unsigned long long *__restrict__ counts)
{
    __shared__ double sax[PBLOCK], say[PBLOCK], sbx[PBLOCK], sby[PBLOCK];
    __shared__ int32_t s_pass[PBLOCK];
    __shared__ uint8_t s_flag[PBLOCK];
    __shared__ int s_wave[PBLOCK / 64];
    __shared__ unsigned long long s_hit[PBLOCK / 64];
    __shared__ unsigned s_red[PBLOCK / 64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // which field: the last one whose first tile is <= this block (a field without tiles shares its first tile with the next: never chosen)
    const int64_t blk = blockIdx.x;
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (F.tile_first[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    const int64_t f = lo;
    const PcoverDims d = F.dims[f];
    const int64_t nx = d.nx, ny = d.ny, tiles_x = (nx + PT - 1) / PT;
    const int64_t tile = blk - F.tile_first[f], tx = tile % tiles_x, ty = tile / tiles_x;
    const int64_t i = tx * PT + lane, j0 = ty * PT + wave;
    const double X = pcover_cell(d.gx, i, res);
    unsigned valid = 0;
    for (int q = 0; q < PQ; ++q) valid |= (i < nx && j0 + 4 * q < ny) ? (1u << q) : 0u;
    // the tile's cells span [bx0, bx1] x [by0, by1]
    const int64_t i1 = min(tx * PT + PT - 1, nx - 1), j1 = min(ty * PT + PT - 1, ny - 1);
    const double bx0 = pcover_cell(d.gx, tx * PT, res), bx1 = pcover_cell(d.gx, i1, res);
    const double by0 = pcover_cell(d.gy, ty * PT, res), by1 = pcover_cell(d.gy, j1, res);

    // ---- phase 1: inside ----
    unsigned par = 0;
    {
        const int64_t r0 = F.ring_offsets[f], r1 = F.ring_offsets[f + 1];
        const int64_t v0 = F.vert_offsets[r0], ne = F.vert_offsets[r1] - v0;
        for (int64_t base = 0; base < ne; base += PBLOCK) {
            __syncthreads();                    // (the LDS columns of the pass before are read)
            const int64_t e = base + tid;
            bool keep = false;
            double up = 0, wp = 0, uq = 0, wq = 0;
            if (e < ne) {
                const int64_t v = v0 + e;
                int64_t a = r0, b = r1;         // the last ring of the field whose first vertex lies at or before v
                while (b - a > 1) {
                    const int64_t mid = a + (b - a) / 2;
                    if (F.vert_offsets[mid] <= v) a = mid; else b = mid;
                }
                const int64_t nxt = v + 1 == F.vert_offsets[a + 1] ? F.vert_offsets[a] : v + 1;
                swath_uw(F.x[v], F.y[v], 1.0, 0.0, up, wp);
                swath_uw(F.x[nxt], F.y[nxt], 1.0, 0.0, uq, wq);
                keep = !(fmin(wp, wq) > by1 || fmax(wp, wq) < by0);       // an edge that crosses a row of the tile spans it
            }
            int total;
            const int pos = pcover_compact(keep, lane, wave, s_wave, total);
            if (keep) { sax[pos] = up; say[pos] = wp; sbx[pos] = uq; sby[pos] = wq; }
            __syncthreads();
            if (valid) {
                for (int k = 0; k < total; ++k) {
                    const double cup = sax[k], cwp = say[k], cuq = sbx[k], cwq = sby[k];
#pragma unroll
                    for (int q = 0; q < PQ; ++q) {
                        if ((valid >> q) & 1u) {
                            const double Y = pcover_cell(d.gy, j0 + 4 * q, res);
                            if (pcover_edge_left_uw(cup, cwp, cuq, cwq, X, Y)) par ^= 1u << q;
                        }
                    }
                }
            }
        }
    }

    // ---- phase 2: covered, overlapped ----
    const double r = W / 2.0, r2 = r * r, reach = pcover_reach(r);
    unsigned cov = 0, ovl = 0;
    int32_t first[PQ];
#pragma unroll
    for (int q = 0; q < PQ; ++q) first[q] = 0;
    const int64_t c0 = F.chunk_first[f], c1 = F.chunk_first[f + 1];
    for (int64_t base = c0; base < c1; base += PBLOCK) {
        if (__syncthreads_or((valid & ~ovl) != 0u) == 0) break;       // every cell of the tile is overlapped (also guards s_hit)
        const int64_t c = base + tid;
        bool hit = false;
        if (c < c1) {
            const PcoverBox B = boxes[c];
            hit = !(B.x0 - bx1 > reach || bx0 - B.x1 > reach || B.y0 - by1 > reach || by0 - B.y1 > reach);
        }
        const unsigned long long hm = __ballot(hit);
        if (lane == 0) s_hit[wave] = hm;
        __syncthreads();
        for (int w = 0; w < PBLOCK / 64; ++w) {
            unsigned long long m = s_hit[w];            // (the same word in every thread: the loops below are uniform)
            while (m) {
                const int bit = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                const PcoverChunk C = chunks[base + w * 64 + bit];
                __syncthreads();                // (the survivors of the chunk before are read)
                bool keep = false, ja = false, jb = false;
                double ax = 0, ay = 0, bx = 0, by = 0;
                int32_t pass = 0;
                if (tid < C.count && pcover_segment(P, C.path, C.p0, C.p1, C.first + tid, caps, ax, ay, bx, by, pass, ja, jb))
                    keep = !(fmin(ax, bx) - bx1 > reach || bx0 - fmax(ax, bx) > reach || fmin(ay, by) - by1 > reach || by0 - fmax(ay, by) > reach);
                int total;
                const int pos = pcover_compact(keep, lane, wave, s_wave, total);
                if (keep) {
                    sax[pos] = ax; say[pos] = ay; sbx[pos] = bx; sby[pos] = by;
                    s_pass[pos] = pass; s_flag[pos] = (uint8_t)((ja ? 1 : 0) | (jb ? 2 : 0));
                }
                __syncthreads();
                if (valid & ~ovl) {
                    for (int k = 0; k < total; ++k) {
                        const double cax = sax[k], cay = say[k], cbx = sbx[k], cby = sby[k];
                        const int32_t cp = s_pass[k];
                        const unsigned fl = s_flag[k];
#pragma unroll
                        for (int q = 0; q < PQ; ++q) {
                            if (((valid & ~ovl) >> q) & 1u) {
                                const double Y = pcover_cell(d.gy, j0 + 4 * q, res);
                                if (pcover_covers(cax, cay, cbx, cby, X, Y, r2, (fl & 1u) != 0u, (fl & 2u) != 0u)) {
                                    if (!((cov >> q) & 1u)) { cov |= 1u << q; first[q] = cp; }
                                    else if (first[q] != cp) ovl |= 1u << q;
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    const unsigned inside = par & valid;
    if (grid && i < nx) {
        const int64_t at = F.cell_first[f];
        for (int q = 0; q < PQ; ++q) {
            const int64_t j = j0 + 4 * q;
            if (j < ny) grid[at + j * nx + i] = (uint8_t)(((inside >> q) & 1u) | (((cov >> q) & 1u) << 1) | (((ovl >> q) & 1u) << 2));
        }
    }
    unsigned c4[4] = { (unsigned)__popc(inside), (unsigned)__popc(inside & cov), (unsigned)__popc(inside & ovl), (unsigned)__popc(cov & ~inside) };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned v = c4[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (tid < 4) {
        const unsigned v = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
        if (v) atomicAdd(&counts[4 * f + tid], (unsigned long long)v);
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_pcover_sizes(hipStream_t st, int64_t n, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x, const double *y,
                        double W, double res, PcoverDims *dims, int32_t *status)
{
    if (n <= 0) return 0;
    const int per = PBLOCK / 64;
    return launch(st, k_pcover_sizes, blocks_for(n, per), PBLOCK, n, ring_offsets, vert_offsets, x, y, W, res, dims, status);
}

int launch_pcover_offsets(hipStream_t st, int64_t n, const PcoverDims *dims, int64_t *cell_first, int64_t *tile_first, int64_t *err)
{
    if (cell_first) {
        if (int e = launch_path_counts<PBLOCK>(st, n, PcoverCellCount{ dims }, cell_first, err)) return e;
    }
    if (tile_first) {
        if (int e = launch_path_counts<PBLOCK>(st, n, PcoverTileCount{ dims }, tile_first, err)) return e;
    }
    return 0;
}

int launch_pcover_boxes(hipStream_t st, int64_t n_chunks, const PcoverChunk *chunks, const PcoverPaths &paths, PcoverBox *boxes)
{
    if (n_chunks <= 0) return 0;
    return launch(st, k_pcover_boxes, (unsigned)n_chunks, PBLOCK, n_chunks, chunks, paths, boxes);
}

int launch_pcover_tiles(hipStream_t st, int64_t n, int64_t n_tiles, const PcoverFields &f, double W, double res, int caps, const PcoverChunk *chunks,
                        const PcoverBox *boxes, const PcoverPaths &paths, uint8_t *grid, unsigned long long *counts)
{
    if (n <= 0 || n_tiles <= 0) return 0;
    return launch(st, k_pcover_tiles, (unsigned)n_tiles, PBLOCK, n, f, W, res, caps, chunks, boxes, paths, grid, counts);
}

}  // namespace fcpp
