// fcpp_glue_cells.cpp -- C-ABI glue of the field cells (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_cellfn.h"
#include "fcpp_cells.h"
#include "fcpp_parallel.h"

using namespace fcpp;

namespace {
// ---- what fcpp_cells_counts / _fill and fcpp_debug_cells check alike ------------------------------------------------------------------
int cells_params(int events, double min_area)
{
    if (events != CELL_REFLEX && events != CELL_EXTREMA) return fail(FCPP_EINVAL, "events must be 0 (reflex) or 1 (extrema)");
    if (!(min_area >= 0.0) || !isfinite(min_area)) return fail(FCPP_EINVAL, "min_area must be non-negative and finite");
    return FCPP_OK;
}

int cells_sizes(int64_t n, int64_t n_rings, int64_t n_verts)
{
    if (n < 0 || n_rings < 0 || n_verts < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

// the most edges of any field the kernels take
int cells_max_edges(int64_t n, const std::vector<int64_t> &rings, const std::vector<int64_t> &verts)
{
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t E = verts[(size_t)rings[(size_t)i + 1]] - verts[(size_t)rings[(size_t)i]];
        if (E <= CELL_MAX_EDGES) m = std::max(m, E);
    }
    return (int)m;
}

// the checks of a device entry behind its NULL tests: parameters, sizes, the CSR head and the angles, read back; -> the most edges
int cells_inputs(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                 const double *angle, int events, double min_area, int &max_edges)
{
    int rc = cells_params(events, min_area);
    if (rc == FCPP_OK) rc = cells_sizes(n, n_rings, n_verts);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> rings, verts;
    rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    if (rc) return rc;
    max_edges = cells_max_edges(n, rings, verts);
    return FCPP_OK;
}

// what one field gave on the host
struct CellsOfField {
    CellTotals t;
    std::vector<int32_t> off, src;
    std::vector<double> x, y, area;
};
}  // namespace

extern "C" {

// ---- field cells (fcpp_cells.hip; the rule: fcpp_cellfn.h) ----------------------------------------------------------------------------
int fcpp_cells_counts(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                      const double *x, const double *y, const double *angle, int events, double min_area, int64_t *cell_offsets,
                      int64_t *cell_offsets_host, int64_t *cvert_offsets, int64_t *cvert_offsets_host, int32_t *status, int32_t *n_cuts,
                      int32_t *dropped, double *dropped_area)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y)) || (n > 0 && !angle)) return fail(FCPP_EINVAL, "bad arguments");
    int max_edges = 0;
    int rc = cells_inputs(c, n, ring_offsets, n_rings, vert_offsets, n_verts, angle, events, min_area, max_edges);
    if (rc) return rc;
    hipStream_t st = c->stream;
    DevBuf<int32_t> counts;
    DevBuf<int64_t> err, spare;
    HIPCHK(counts.alloc((size_t)(2 * n + 1)));
    HIPCHK(err.alloc(2));
    if (!cell_offsets || !cvert_offsets) HIPCHK(spare.alloc((size_t)n + 1));
    int64_t *const co = cell_offsets ? cell_offsets : spare.p, *const vo = cvert_offsets ? cvert_offsets : spare.p;
    LAUNCHCHK(launch_cells_count(st, n, max_edges, ring_offsets, vert_offsets, x, y, angle, events, min_area, counts.p, counts.p + n, status, n_cuts,
                                 dropped, dropped_area));
    LAUNCHCHK(launch_cells_offsets(st, n, counts.p, co, err.p));
    if (cell_offsets_host) HIPCHK(hipMemcpyAsync(cell_offsets_host, co, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    LAUNCHCHK(launch_cells_offsets(st, n, counts.p + n, vo, err.p + 1));
    if (cvert_offsets_host) HIPCHK(hipMemcpyAsync(cvert_offsets_host, vo, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    int64_t bad[2] = { 0, 0 };
    HIPCHK(hipMemcpyAsync(bad, err.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad[0] || bad[1]) return fail(FCPP_ESIZE, "the cell counts could not be scanned");
    return FCPP_OK;
}

int fcpp_cells_fill(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                    const double *x, const double *y, const double *angle, int events, double min_area, const int64_t *cell_offsets,
                    const int64_t *cvert_offsets, int64_t total_cells, int64_t total_verts, int64_t *out_vert_offsets, double *out_x,
                    double *out_y, int32_t *out_src, int32_t *cell_field, double *area)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!ring_offsets || !vert_offsets || !cell_offsets || !cvert_offsets || (n_verts > 0 && (!x || !y)) || (n > 0 && !angle))
        return fail(FCPP_EINVAL, "bad arguments");
    if (total_cells < 0 || total_verts < 0) return fail(FCPP_ESIZE, "bad sizes");
    int max_edges = 0;
    int rc = cells_inputs(c, n, ring_offsets, n_rings, vert_offsets, n_verts, angle, events, min_area, max_edges);
    std::vector<int64_t> co, vo;
    if (rc == FCPP_OK) rc = host_offsets(c, n, cell_offsets, nullptr, total_cells, "cell_offsets", co);
    if (rc == FCPP_OK) rc = host_offsets(c, n, cvert_offsets, nullptr, total_verts, "vert_offsets", vo);
    if (rc) return rc;
    LAUNCHCHK(launch_cells_fill(c->stream, n, max_edges, ring_offsets, vert_offsets, x, y, angle, events, min_area, cell_offsets, cvert_offsets,
                                total_cells, total_verts, out_vert_offsets, out_x, out_y, out_src, cell_field, area));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_cells(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                     const double *y, const double *angle, int events, double min_area, int64_t *cell_offsets, int64_t *cvert_offsets,
                     int32_t *status, int32_t *n_cuts, int32_t *dropped, double *dropped_area, int64_t cell_cap, int64_t vert_cap,
                     int64_t *out_vert_offsets, double *out_x, double *out_y, int32_t *out_src, int32_t *cell_field, double *area)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y)) || (n > 0 && !angle)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = cells_params(events, min_area);
    if (rc == FCPP_OK) rc = cells_sizes(n, n_rings, n_verts);
    if (rc == FCPP_OK && (cell_cap < 0 || vert_cap < 0)) rc = fail(FCPP_ESIZE, "bad sizes");
    std::vector<int64_t> rings, verts;
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, n, angle, nullptr);
    if (rc) return rc;
    std::vector<CellsOfField> got;
    try {
        got.resize((size_t)n);
        // (a field's vectors grow inside the pool: std::bad_alloc comes back from parallel_for)
        WorkerPool::parallel_for(n, [&](int64_t i) {
            CellWork work;
            CellsOfField &g = got[(size_t)i];
            g.t = cell_field_host(verts.data(), rings[(size_t)i], rings[(size_t)i + 1], x, y, angle[i], events, min_area, work,
                [&](int32_t, int32_t off, double a) { g.off.push_back(off); g.area.push_back(a); },
                [&](int32_t at, double vx, double vy, int32_t src) {
                    if ((size_t)at >= g.x.size()) { g.x.resize((size_t)at + 1); g.y.resize((size_t)at + 1); g.src.resize((size_t)at + 1); }
                    g.x[(size_t)at] = vx; g.y[(size_t)at] = vy; g.src[(size_t)at] = src;
                });
        });
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    int64_t cell_at = 0, vert_at = 0;
    for (int64_t i = 0; i < n; ++i) {
        const CellsOfField &g = got[(size_t)i];
        store(cell_offsets, i, cell_at); store(cvert_offsets, i, vert_at);
        store(status, i, g.t.status); store(n_cuts, i, g.t.n_cuts); store(dropped, i, g.t.dropped); store(dropped_area, i, g.t.dropped_area);
        for (size_t k = 0; k < g.off.size(); ++k) {
            const int64_t ci = cell_at + (int64_t)k;
            if (ci >= cell_cap) break;
            store(out_vert_offsets, ci, vert_at + g.off[k]); store(cell_field, ci, (int32_t)i); store(area, ci, g.area[k]);
        }
        for (size_t k = 0; k < g.x.size(); ++k) {
            const int64_t at = vert_at + (int64_t)k;
            if (at >= vert_cap) break;
            store(out_x, at, g.x[k]); store(out_y, at, g.y[k]); store(out_src, at, g.src[k]);
        }
        cell_at += g.t.n_cells;
        vert_at += g.t.n_verts;
    }
    store(cell_offsets, n, cell_at); store(cvert_offsets, n, vert_at);
    if (out_vert_offsets && cell_at <= cell_cap) out_vert_offsets[cell_at] = vert_at;
    return FCPP_OK;
}

}  // extern "C"
