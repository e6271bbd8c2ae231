// fcpp_glue_tour.cpp -- C-ABI glue of the cell tour and its host twin (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_parallel.h"
#include "fcpp_tour.h"
#include "fcpp_tourfn.h"

using namespace fcpp;

namespace {
// ---- what fcpp_cell_tour_transit / _solve and their host twin check alike ------------------------------------------------------------------
int tour_search(int S, double min_gain, int max_sweeps)
{
    if (S < 1 || S > TOUR_MAX_STARTS) return fail(FCPP_EINVAL, "n_starts must lie in 1 .. 64");
    if (!(min_gain >= 0.0) || !isfinite(min_gain)) return fail(FCPP_EINVAL, "min_gain must be non-negative and finite");
    if (max_sweeps < 0 || max_sweeps > TOUR_MAX_SWEEPS) return fail(FCPP_EINVAL, "max_sweeps must lie in 0 .. 2^20");
    return FCPP_OK;
}

// the three offset tables on the host, checked against each other: block f holds N_f^2 entries, none beyond a cap
int tour_offsets(fcpp_ctx *c, int64_t n, const int64_t *coff_ptr, const int64_t *coff_host, int64_t n_cells, const int64_t *voff_ptr,
                 const int64_t *voff_host, int64_t n_vars, const int64_t *doff_ptr, const int64_t *doff_host, int64_t d_total,
                 std::vector<int64_t> &coff, std::vector<int64_t> &voff, std::vector<int64_t> &doff)
{
    if (n < 0 || n_cells < 0 || n_vars < 0 || d_total < 0 || n > INT32_MAX || n_vars > INT64_MAX / 4) return fail(FCPP_ESIZE, "bad sizes");
    int rc = host_offsets(c, n, coff_ptr, coff_host, n_cells, "cell_offsets", coff);
    if (rc == FCPP_OK) rc = host_offsets(c, n_cells, voff_ptr, voff_host, n_vars, "var_offsets", voff);
    if (rc == FCPP_OK) rc = host_offsets(c, n, doff_ptr, doff_host, d_total, "d_offsets", doff);
    if (rc) return rc;
    for (int64_t f = 0; f < n; ++f)
        if (doff[(size_t)f + 1] - doff[(size_t)f] != tour_block(voff.data(), coff[(size_t)f], coff[(size_t)f + 1]))
            return fail(FCPP_ESIZE, "d_offsets do not match the variant counts: block f holds N_f^2 entries, none for a field beyond a cap");
    return FCPP_OK;
}

bool tour_poses_missing(int64_t n_vars, const double *ix, const double *iy, const double *ih, const double *ox, const double *oy, const double *oh)
{
    return n_vars > 0 && (!ix || !iy || !ih || !ox || !oy || !oh);
}
}  // namespace

extern "C" {

// ---- cell tour (fcpp_tour.hip; the rule: fcpp_tourfn.h) ------------------------------------------------------------------------------
int fcpp_cell_tour_transit(fcpp_ctx *c, int64_t n, const int64_t *cell_offsets, const int64_t *cell_offsets_host, int64_t n_cells,
                           const int64_t *var_offsets, const int64_t *var_offsets_host, int64_t n_vars, const double *ix, const double *iy,
                           const double *ih, const double *ox, const double *oy, const double *oh, double radius, int mode,
                           const int64_t *d_offsets, const int64_t *d_offsets_host, int64_t d_total, double *D)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!cell_offsets || !var_offsets || !d_offsets || tour_poses_missing(n_vars, ix, iy, ih, ox, oy, oh) || (d_total > 0 && !D))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> coff, voff, doff;
    rc = tour_offsets(c, n, cell_offsets, cell_offsets_host, n_cells, var_offsets, var_offsets_host, n_vars, d_offsets, d_offsets_host, d_total, coff,
                      voff, doff);
    if (rc == FCPP_OK && (d_total + 255) / 256 > TOUR_MAX_GROUPS) rc = fail(FCPP_ESIZE, "2^39 joint entries or more");
    if (rc) return rc;
    LAUNCHCHK(launch_tour_transit(c->stream, n, cell_offsets, var_offsets, ix, iy, ih, ox, oy, oh, radius, mode, d_offsets, d_total, D));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_cell_tour_solve(fcpp_ctx *c, int64_t n, const int64_t *cell_offsets, const int64_t *cell_offsets_host, int64_t n_cells,
                         const int64_t *var_offsets, const int64_t *var_offsets_host, int64_t n_vars, const double *w, const int32_t *stored_node,
                         const int64_t *d_offsets, const int64_t *d_offsets_host, int64_t d_total, const double *D, const double *E, const double *X,
                         int n_starts, double min_gain, int max_sweeps, int32_t *order, int32_t *node, double *cost, double *stored,
                         double *joint_length, int32_t *winner, int32_t *sweeps, int32_t *skipped, int32_t *status, int32_t *tours, double *costs)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!cell_offsets || !var_offsets || !d_offsets || (n_vars > 0 && !w) || (d_total > 0 && !D)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = tour_search(n_starts, min_gain, max_sweeps);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> coff, voff, doff;
    rc = tour_offsets(c, n, cell_offsets, cell_offsets_host, n_cells, var_offsets, var_offsets_host, n_vars, d_offsets, d_offsets_host, d_total, coff,
                      voff, doff);
    if (rc == FCPP_OK && n > TOUR_MAX_GROUPS / n_starts) rc = fail(FCPP_ESIZE, "2^31 (field, candidate) pairs or more");
    if (rc) return rc;
    // what the pick reads is the solve's own when the caller does not want it
    DevBuf<int32_t> own_tours, applied;
    DevBuf<double> own_costs, stored_in;
    if (!tours) { HIPCHK(own_tours.alloc((size_t)n_starts * (size_t)n_cells)); tours = own_tours.p; }
    if (!costs) { HIPCHK(own_costs.alloc((size_t)n * (size_t)n_starts)); costs = own_costs.p; }
    HIPCHK(stored_in.alloc((size_t)n));
    HIPCHK(applied.alloc((size_t)n * (size_t)n_starts));
    LAUNCHCHK(launch_tour_solve(c->stream, n, n_starts, cell_offsets, n_cells, var_offsets, w, stored_node, d_offsets, D, E, X, min_gain, max_sweeps,
                                tours, costs, applied.p, stored_in.p));
    LAUNCHCHK(launch_tour_pick(c->stream, n, n_starts, cell_offsets, n_cells, var_offsets, w, stored_node, d_offsets, D, E, X, tours, costs, applied.p,
                               stored_in.p, order, node, cost, stored, joint_length, winner, sweeps, skipped, status));
    HIPCHK(hipStreamSynchronize(c->stream));      // (the temporaries die here)
    return FCPP_OK;
}

int fcpp_debug_cell_tour(int64_t n, const int64_t *cell_offsets, int64_t n_cells, const int64_t *var_offsets, int64_t n_vars, const double *ix,
                         const double *iy, const double *ih, const double *ox, const double *oy, const double *oh, const double *w,
                         const int32_t *stored_node, double radius, int mode, const int64_t *d_offsets, int64_t d_total, double *D, const double *E,
                         const double *X, int n_starts, double min_gain, int max_sweeps, int32_t *order, int32_t *node, double *cost, double *stored,
                         double *joint_length, int32_t *winner, int32_t *sweeps, int32_t *skipped, int32_t *status, int32_t *tours, double *costs)
{
    if (!cell_offsets || !var_offsets || !d_offsets || tour_poses_missing(n_vars, ix, iy, ih, ox, oy, oh) || (n_vars > 0 && !w))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc == FCPP_OK) rc = tour_search(n_starts, min_gain, max_sweeps);
    if (rc) return rc;
    std::vector<int64_t> coff, voff, doff;
    rc = tour_offsets(nullptr, n, cell_offsets, nullptr, n_cells, var_offsets, nullptr, n_vars, d_offsets, nullptr, d_total, coff, voff, doff);
    if (rc == FCPP_OK && n > TOUR_MAX_GROUPS / n_starts) rc = fail(FCPP_ESIZE, "2^31 (field, candidate) pairs or more");
    if (rc) return rc;
    std::vector<double> own_D;
    if (!D) {
        try { own_D.assign((size_t)d_total, 0.0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
        D = own_D.data();
    }
    WorkerPool::parallel_for(n, [&](int64_t f) {
        const int64_t c0 = coff[(size_t)f], c1 = coff[(size_t)f + 1], v0 = voff[(size_t)c0], d0 = doff[(size_t)f];
        const int64_t Nf = doff[(size_t)f + 1] == d0 ? 0 : 2 * (voff[(size_t)c1] - v0);
        for (int64_t a = 0; a < Nf; ++a) {
            const int64_t ca = tour_cell_of(voff.data(), c0, c1, a);
            for (int64_t b = 0; b < Nf; ++b) {
                double v = INFINITY;
                if (ca != tour_cell_of(voff.data(), c0, c1, b))
                    v = mode == 0 ? tour_transit<0>(ix, iy, ih, ox, oy, oh, radius, v0 + (a >> 1), (int)(a & 1), v0 + (b >> 1), (int)(b & 1))
                                  : tour_transit<1>(ix, iy, ih, ox, oy, oh, radius, v0 + (a >> 1), (int)(a & 1), v0 + (b >> 1), (int)(b & 1));
                D[d0 + a * Nf + b] = v;
            }
        }
        const TourResult r = tour_field_host(voff.data(), c0, c1, w, stored_node, D + d0, E, X, n_starts, min_gain, max_sweeps,
                                             order ? order + c0 : nullptr, node ? node + c0 : nullptr, tours ? tours + c0 : nullptr, n_cells,
                                             costs ? costs + f * n_starts : nullptr);
        store(cost, f, r.cost); store(stored, f, r.stored); store(joint_length, f, r.joint); store(winner, f, r.winner); store(sweeps, f, r.sweeps);
        store(skipped, f, r.skipped); store(status, f, r.status);
    });
    return FCPP_OK;
}

}  // extern "C"
