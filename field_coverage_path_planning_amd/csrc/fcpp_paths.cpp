// fcpp_paths.cpp -- C-ABI glue of the standalone path operators on caller-supplied paths: curvature, speed plan, verify / validate, the
// trajectory and its fixed-step sampler, and the small stateless operators.  Like fcpp_api.cpp: argument checking, device buffers, launches;
// every path operator drains the context's stream before it returns.  (The other families' glue: fcpp_glue_*.cpp; what they share: fcpp_glue.h.)
#include "fcpp_glue.h"
#include "fcpp_traj.h"

using namespace fcpp;

namespace fcpp {
// The trajectory scan's own tables of a path set (fcpp_trajectory): the blocks of its path-anchored spine and the scan's scratch, built
// from the offsets on the first trajectory call for them.
struct TrajTables {
    DevBuf<TrajBlock> blocks;
    DevBuf<int64_t> block_first;      // n_paths + 1
    DevBuf<TrajAgg> agg, pre;         // per tile: its own sums / what enters it, relative to its block
    DevBuf<TrajAgg> blk, cin;         // per block: its own sums / what enters it, relative to its path
    DevBuf<int64_t> path_first;       // per path: where its first non-zero step starts
    int64_t n_blocks = 0;
    bool built = false;
};

// The tile table of a path set, kept in the context between calls of the standalone operators: a caller that plans and verifies
// the same paths (the planner mirror does: speed plan, verify, verify again) pays for the host-side tiling and its upload once.
struct PathTiling {
    std::vector<int64_t> offs;
    DevTiling dt;
    TrajTables traj;
};

void free_paths_cache(fcpp_ctx *c) { delete c->paths_cache; c->paths_cache = nullptr; }

}  // namespace fcpp

namespace {
DevConst const_from_vehicle(const fcpp_vehicle &veh)
{
    fcpp_options o;
    fcpp_options_default(&o);
    return make_const(veh, o);
}

// The path set of a call, on the context's device: its offsets brought to the host and checked once, its tile table from the context's
// cache -- rebuilt only when the offsets differ from the cached set's.
int path_set(fcpp_ctx *c, int64_t n_paths, const int64_t *offsets_dev, const int64_t *offsets_host, int64_t total, PathTiling **out)
{
    HIPCHK(hipSetDevice(c->device));
    if (n_paths < 0 || total < 0 || n_paths > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    std::vector<int64_t> offs;
    const int rc = host_offsets(c, n_paths, offsets_dev, offsets_host, total, "offsets", offs);
    if (rc) return rc;
    if (!c->paths_cache || c->paths_cache->offs != offs) {
        PathTiling *pt = new (std::nothrow) PathTiling();
        if (!pt) return fail(FCPP_ENOMEM, "out of host memory");
        Tiling til;
        til.build(n_paths, offs.data());
        hipError_t e = pt->dt.upload(til, c->stream);
        if (e != hipSuccess) { delete pt; return fail(FCPP_EHIP, std::string("tile table upload: ") + hipGetErrorString(e)); }
        pt->offs.swap(offs);
        // (work of earlier calls on the old table has completed: every standalone operator synchronises before it returns)
        delete c->paths_cache;
        c->paths_cache = pt;
    }
    *out = c->paths_cache;
    return FCPP_OK;
}

// The standalone operators' statistics: a path per 64 lanes -- or, for a few LONG paths (one path of 6e7 points is 123 000 tiles: 1.2 ms
// through one wavefront), every path sliced over 64 workgroups and joined (the fused pipeline's class-3 reduction: 10 us).
int reduce_paths(fcpp_ctx *c, hipStream_t st, DevTiling &dt, fcpp_field_stats *stats)
{
    if (dt.n_paths > 0 && dt.n_paths <= 64 && dt.n_tiles / dt.n_paths > 2048) {
        const size_t need = (size_t)dt.n_paths * 64 * 104;
        if (c->verify_scratch_cap < need) {
            if (c->verify_scratch) { HIPCHK(hipStreamSynchronize(st)); (void)hipFree(c->verify_scratch); c->verify_scratch = nullptr; c->verify_scratch_cap = 0; }
            HIPCHK(hipMalloc(&c->verify_scratch, need));
            c->verify_scratch_cap = need;
        }
        LAUNCHCHK(launch_reduce_stats(st, dt.n_paths, dt.partial.p, dt.tile_first.p, nullptr, stats, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 256,
                                      c->verify_scratch, 0));
    } else LAUNCHCHK(launch_reduce_stats(st, dt.n_paths, dt.partial.p, dt.tile_first.p, nullptr, stats));
    return FCPP_OK;
}

// fcpp_verify, and the first half of fcpp_validate: curvature (left in kap), a_lat flags and the per-path metrics.  Enqueued, not
// drained: both temporaries are the caller's, to be released after it has drained the stream.
int path_metrics(fcpp_ctx *c, PathTiling &ps, const DevConst &cst, const double *x, const double *y, const double *v, DevBuf<double> &kap,
                 DevBuf<double> &vtmp, fcpp_field_stats *stats)
{
    hipStream_t st = c->stream;
    DevTiling &dt = ps.dt;
    HIPCHK(kap.alloc((size_t)ps.offs.back()));
    HIPCHK(vtmp.alloc((size_t)ps.offs.back()));
    LAUNCHCHK(launch_curv_clamp(st, dt.n_tiles, dt.tiles.p, dt.paths.p, cst, 0, x, y, v, vtmp.p, kap.p, nullptr));
    DevObstacles none = { nullptr, nullptr, nullptr, nullptr };
    LAUNCHCHK(launch_validate(st, dt.n_tiles, dt.tiles.p, dt.paths.p, nullptr, cst, none, x, y, kap.p, v, nullptr, dt.partial.p));
    return reduce_paths(c, st, dt, stats);
}

int ensure_traj(PathTiling &pt, hipStream_t st)
{
    TrajTables &tr = pt.traj;
    if (tr.built) return FCPP_OK;
    const int64_t n_paths = (int64_t)pt.offs.size() - 1;
    std::vector<TrajBlock> blocks;
    std::vector<int64_t> first((size_t)n_paths + 1, 0);
    try {
        int64_t tile0 = 0;
        for (int64_t p = 0; p < n_paths; ++p) {
            const int64_t n = pt.offs[(size_t)p + 1] - pt.offs[(size_t)p], nt = (n + TILE_POINTS - 1) / TILE_POINTS;   // (Tiling::build)
            first[(size_t)p] = (int64_t)blocks.size();
            for (int64_t k = 0; k < nt; k += TRAJ_BLOCK_TILES)
                blocks.push_back({ tile0 + k, (int32_t)p, (int32_t)std::min<int64_t>(TRAJ_BLOCK_TILES, nt - k) });
            tile0 += nt;
        }
        first[(size_t)n_paths] = (int64_t)blocks.size();
        if (tile0 != pt.dt.n_tiles) return fail(FCPP_ESIZE, "trajectory blocks do not match the tile table");
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    tr.n_blocks = (int64_t)blocks.size();
    HIPCHK(tr.blocks.upload(blocks, st));
    HIPCHK(tr.block_first.upload(first, st));
    HIPCHK(tr.agg.alloc((size_t)pt.dt.n_tiles));
    HIPCHK(tr.pre.alloc((size_t)pt.dt.n_tiles));
    HIPCHK(tr.blk.alloc((size_t)tr.n_blocks));
    HIPCHK(tr.cin.alloc((size_t)tr.n_blocks));
    HIPCHK(tr.path_first.alloc((size_t)n_paths));
    HIPCHK(hipStreamSynchronize(st));      // (the staging vectors die here)
    tr.built = true;
    return FCPP_OK;
}
}  // namespace

int fcpp::trajectory_paths(fcpp_ctx *c, int64_t n_paths, const int64_t *offsets, const int64_t *offsets_host, int64_t total, const double *x,
                           const double *y, const double *v, const uint32_t *fs, double *s, double *t, double *heading, double *totals)
{
    PathTiling *ps = nullptr;
    int rc = path_set(c, n_paths, offsets, offsets_host, total, &ps);
    if (rc) return rc;
    DevTiling &dt = ps->dt;
    hipStream_t st = c->stream;
    rc = ensure_traj(*ps, st);
    if (rc) return rc;
    TrajTables &tr = ps->traj;
    LAUNCHCHK(launch_traj_tiles(st, dt.n_tiles, dt.tiles.p, dt.paths.p, x, y, v, tr.agg.p));
    LAUNCHCHK(launch_traj_blocks(st, tr.n_blocks, tr.blocks.p, tr.agg.p, tr.pre.p, tr.blk.p));
    LAUNCHCHK(launch_traj_paths(st, n_paths, tr.block_first.p, tr.blk.p, tr.cin.p, tr.path_first.p, totals));
    if (s || t || heading)
        LAUNCHCHK(launch_traj_apply(st, dt.n_tiles, dt.tiles.p, dt.paths.p, dt.tile_first.p, tr.block_first.p, x, y, v, fs, tr.pre.p, tr.cin.p,
                                    tr.path_first.p, s, t, heading));
    HIPCHK(hipStreamSynchronize(st));
    return FCPP_OK;
}

int fcpp::path_tiling(fcpp_ctx *c, int64_t n_paths, const int64_t *offsets, const int64_t *offsets_host, int64_t total, DevTiling **out)
{
    PathTiling *ps = nullptr;
    const int rc = path_set(c, n_paths, offsets, offsets_host, total, &ps);
    if (rc == FCPP_OK) *out = &ps->dt;
    return rc;
}

extern "C" {

int fcpp_curvature(fcpp_ctx *c, int64_t n_paths, const int64_t *offsets, int64_t total, const double *x,
                   const double *y, double *kappa, const int64_t *offsets_host)
{
    if (!c || (!offsets && !offsets_host) || (total > 0 && (!x || !y || !kappa))) return fail(FCPP_EINVAL, "bad arguments");
    PathTiling *ps = nullptr;
    int rc = path_set(c, n_paths, offsets, offsets_host, total, &ps);
    if (rc) return rc;
    DevTiling &dt = ps->dt;
    fcpp_vehicle veh;
    fcpp_vehicle_default(&veh);
    DevConst cst = const_from_vehicle(veh);
    DevBuf<double> vtmp;
    HIPCHK(vtmp.alloc((size_t)total));
    HIPCHK(hipMemsetAsync(vtmp.p, 0, (size_t)total * sizeof(double), c->stream));
    LAUNCHCHK(launch_curv_clamp(c->stream, dt.n_tiles, dt.tiles.p, dt.paths.p, cst, 0, x, y, vtmp.p, vtmp.p, kappa, nullptr));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_speed_plan(fcpp_ctx *c, const fcpp_vehicle *veh, int clamp, int64_t n_paths, const int64_t *offsets,
                    int64_t total, const double *x, const double *y, const double *v_in, double *v_out, double *kappa,
                    int64_t *n_adjusted, const int64_t *offsets_host)
{
    if (!c || !veh || (!offsets && !offsets_host) || (total > 0 && (!x || !y || !v_in || !v_out))) return fail(FCPP_EINVAL, "bad arguments");
    if (!(veh->max_longitudinal_accel > 0) || !(veh->max_lateral_accel > 0)) return fail(FCPP_EINVAL, "accelerations must be positive");
    PathTiling *ps = nullptr;
    int rc = path_set(c, n_paths, offsets, offsets_host, total, &ps);
    if (rc) return rc;
    DevTiling &dt = ps->dt;
    DevConst cst = const_from_vehicle(*veh);
    hipStream_t st = c->stream;
    if (n_paths) HIPCHK(hipMemsetAsync(dt.n_adj.p, 0, (size_t)n_paths * sizeof(unsigned long long), st));
    LAUNCHCHK(launch_curv_clamp(st, dt.n_tiles, dt.tiles.p, dt.paths.p, cst, clamp ? 1 : 0, x, y, v_in, v_out, kappa, dt.n_adj.p));
    LAUNCHCHK(launch_scan_tiles(st, dt.n_tiles, dt.tiles.p, dt.paths.p, cst, x, y, v_out, dt.agg_f.p, dt.agg_b.p));
    LAUNCHCHK(launch_scan_spine(st, dt.n_tiles, dt.agg_f.p, dt.agg_b.p, dt.carry_f.p, dt.carry_b.p, dt.spine.p));
    LAUNCHCHK(launch_scan_apply(st, dt.n_tiles, dt.tiles.p, dt.paths.p, cst, clamp ? 3 : 2, x, y, v_out, v_out,
                                dt.carry_f.p, dt.carry_b.p));
    if (n_adjusted && n_paths)
        HIPCHK(hipMemcpyAsync(n_adjusted, dt.n_adj.p, (size_t)n_paths * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return FCPP_OK;
}

int fcpp_verify(fcpp_ctx *c, const fcpp_vehicle *veh, int64_t n_paths, const int64_t *offsets, int64_t total,
                const double *x, const double *y, const double *v, fcpp_field_stats *stats, const int64_t *offsets_host)
{
    if (!c || !veh || (!offsets && !offsets_host) || !stats || (total > 0 && (!x || !y || !v))) return fail(FCPP_EINVAL, "bad arguments");
    PathTiling *ps = nullptr;
    int rc = path_set(c, n_paths, offsets, offsets_host, total, &ps);
    if (rc) return rc;
    DevBuf<double> kap, vtmp;
    rc = path_metrics(c, *ps, const_from_vehicle(*veh), x, y, v, kap, vtmp, stats);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_validate(fcpp_ctx *c, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_paths, const int64_t *offsets, int64_t total,
                  const double *x, const double *y, const double *v, const fcpp_polys *field_polys, const fcpp_polys *obstacles,
                  const int64_t *obstacle_offsets, uint32_t *flags, fcpp_field_stats *stats, const int64_t *offsets_host)
{
    if (!c || !veh || !opt || (!offsets && !offsets_host) || !stats || (total > 0 && (!x || !y || !v || !flags))) return fail(FCPP_EINVAL, "bad arguments");
    if (!isfinite(opt->geofence_tol)) return fail(FCPP_EINVAL, "geofence_tol must be finite");
    std::string err;
    int rc = validate_polys(field_polys, err);
    if (rc == FCPP_OK) rc = validate_polys(obstacles, err);
    if (rc != FCPP_OK) return fail(rc, err);
    if (field_polys && field_polys->n_polys != n_paths) return fail(FCPP_ESIZE, "field_polys must hold one polygon per path");
    const int64_t n_obst = obstacles ? obstacles->n_polys : 0;
    if (obstacle_offsets) {
        if (obstacle_offsets[0] < 0 || obstacle_offsets[n_paths] > n_obst) return fail(FCPP_ESIZE, "obstacle_offsets outside the obstacle table");
        for (int64_t p = 0; p < n_paths; ++p)
            if (obstacle_offsets[p + 1] < obstacle_offsets[p]) return fail(FCPP_ESIZE, "obstacle_offsets must be non-decreasing");
    }
    PathTiling *ps = nullptr;
    rc = path_set(c, n_paths, offsets, offsets_host, total, &ps);
    if (rc) return rc;
    DevTiling &dt = ps->dt;
    DevConst cst = const_from_vehicle(*veh);
    hipStream_t st = c->stream;
    // curvature, a_lat flags and the metrics of fcpp_verify; then the polygon tests
    DevBuf<double> kap, vtmp;
    rc = path_metrics(c, *ps, cst, x, y, v, kap, vtmp, stats);
    if (rc) return rc;
    // the polygon tables: one upload (field vertices, obstacle vertices, their offsets, the per-path obstacle ranges)
    const int64_t nfv = field_polys && n_paths > 0 ? field_polys->offsets[n_paths] : 0, nov = n_obst > 0 ? obstacles->offsets[n_obst] : 0;
    std::vector<double> hv;
    std::vector<int64_t> hi;
    try {
        hv.reserve((size_t)(2 * (nfv + nov)));
        if (nfv) { hv.insert(hv.end(), field_polys->x, field_polys->x + nfv); hv.insert(hv.end(), field_polys->y, field_polys->y + nfv); }
        if (nov) { hv.insert(hv.end(), obstacles->x, obstacles->x + nov); hv.insert(hv.end(), obstacles->y, obstacles->y + nov); }
        if (field_polys) hi.insert(hi.end(), field_polys->offsets, field_polys->offsets + n_paths + 1);
        if (n_obst) hi.insert(hi.end(), obstacles->offsets, obstacles->offsets + n_obst + 1);
        if (obstacle_offsets && n_obst) hi.insert(hi.end(), obstacle_offsets, obstacle_offsets + n_paths + 1);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    DevBuf<double> dv;
    DevBuf<int64_t> di;
    HIPCHK(dv.upload(hv, st));
    HIPCHK(di.upload(hi, st));
    const double *fx = dv.p, *fy = dv.p ? dv.p + nfv : nullptr, *ox = dv.p ? dv.p + 2 * nfv : nullptr, *oy = dv.p ? dv.p + 2 * nfv + nov : nullptr;
    const int64_t *foff = field_polys ? di.p : nullptr;
    const int64_t *ooff = n_obst ? di.p + (field_polys ? n_paths + 1 : 0) : nullptr;
    const int64_t *orng = (obstacle_offsets && n_obst) ? ooff + n_obst + 1 : nullptr;
    LAUNCHCHK(launch_validate_polys(st, dt.n_tiles, dt.tiles.p, dt.paths.p, foff, fx, fy, field_polys ? n_paths : 0, ooff, ox, oy, n_obst, orng,
                                    opt->geofence_tol, cst.a_lat, x, y, kap.p, v, flags, stats));
    HIPCHK(hipStreamSynchronize(st));      // (the staging vectors die here)
    return FCPP_OK;
}

// ---- trajectory: arc length, time stamp and heading per point; fixed-rate sampling (fcpp_traj.hip) ---------------------------------
int fcpp_trajectory(fcpp_ctx *c, int64_t n_paths, const int64_t *offsets, int64_t total, const double *x, const double *y, const double *v,
                    const uint32_t *flagseg, double *s, double *t, double *heading, double *totals, const int64_t *offsets_host)
{
    if (!c || (!offsets && !offsets_host) || (total > 0 && (!x || !y || !v))) return fail(FCPP_EINVAL, "bad arguments");
    return trajectory_paths(c, n_paths, offsets, offsets_host, total, x, y, v, flagseg, s, t, heading, totals);
}

int fcpp_trajectory_counts(fcpp_ctx *c, int64_t n_paths, const double *totals, double dt, int include_end, int64_t *out_offsets,
                           int64_t *out_offsets_host)
{
    if (!c || !out_offsets || (n_paths > 0 && !totals)) return fail(FCPP_EINVAL, "bad arguments");
    if (!(dt > 0.0) || !isfinite(dt)) return fail(FCPP_EINVAL, "dt must be positive");
    if (n_paths < 0 || n_paths > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return sample_counts(c, n_paths, out_offsets, out_offsets_host, "a path's total time is negative or not finite, or it has 2^31 samples or more",
                         [&](hipStream_t st, int64_t *err) { return launch_traj_counts(st, n_paths, totals, dt, include_end ? 1 : 0, out_offsets, err); });
}

int fcpp_trajectory_sample(fcpp_ctx *c, int64_t n_paths, const int64_t *offsets, int64_t total, const double *x, const double *y,
                           const double *v, const double *s, const double *t, const double *heading, const uint32_t *flagseg, double dt,
                           int include_end, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *vs, double *ss,
                           double *hs, uint32_t *flagseg_s, int64_t *src_index, const int64_t *offsets_host, const int64_t *out_offsets_host)
{
    if (!c || (!offsets && !offsets_host) || (!out_offsets && !out_offsets_host) || (total > 0 && (!x || !y || !v || !s || !t || !heading)))
        return fail(FCPP_EINVAL, "bad arguments");
    if (!(dt > 0.0) || !isfinite(dt)) return fail(FCPP_EINVAL, "dt must be positive");
    if (n_paths < 0 || total < 0 || total_samples < 0 || n_paths > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    HIPCHK(hipSetDevice(c->device));
    SampleOffsets offs, outs;
    int rc = offs.get(c, n_paths, offsets, offsets_host, total, "offsets", false);
    if (rc == FCPP_OK) rc = outs.get(c, n_paths, out_offsets, out_offsets_host, total_samples, "out_offsets", true);
    if (rc) return rc;
    LAUNCHCHK(launch_traj_sample(c->stream, n_paths, offs.dev, outs.dev, total_samples, x, y, v, s, t, heading, flagseg, dt, include_end ? 1 : 0, xs,
                                 ys, vs, ss, hs, flagseg_s, src_index));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

// ---- the small stateless operators (enqueued on the context's stream, not drained) -------------------------------------------------
int fcpp_straight_segments(fcpp_ctx *c, int64_t n_seg, const double *seg, int32_t n_points, double *out)
{
    if (!c || n_seg < 0 || n_points < 1 || (n_seg > 0 && (!seg || !out))) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_straight(c->stream, n_seg, seg, n_points, nullptr, out));
    return FCPP_OK;
}

int fcpp_corner_turns(fcpp_ctx *c, const fcpp_vehicle *veh, int64_t n, const double *corners, const int32_t *ci, const int32_t *rev,
                      double L, double H, int32_t stride, double *out, int32_t *counts)
{
    if (!c || !veh || n < 0 || (n > 0 && (!corners || !ci || !rev || !out || !counts))) return fail(FCPP_EINVAL, "bad arguments");
    const double R = veh->min_turn_radius;
    if (!(R > 0)) return fail(FCPP_EINVAL, "min_turn_radius must be positive");
    const int64_t need = 15 + std::max<int64_t>(10, (int64_t)(3.0 * R / 0.5));
    if (stride < need) return fail(FCPP_ESIZE, "stride too small for 15 + max(10, int(3R / 0.5)) points");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_corner_turns(c->stream, n, corners, ci, rev, R, L, H, stride, out, counts));
    return FCPP_OK;
}

int fcpp_fresnel(fcpp_ctx *c, int64_t n, const double *t, double *cc, double *ss)
{
    if (!c || n < 0 || (n > 0 && (!t || !cc || !ss))) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_fresnel(c->stream, n, t, cc, ss));
    return FCPP_OK;
}

int fcpp_distance_matrix(fcpp_ctx *c, int32_t n, const double *x, const double *y, double *D)
{
    if (!c || n < 0 || n > 65535 || (n > 0 && (!x || !y || !D))) return fail(FCPP_EINVAL, "bad arguments (0 <= n <= 65535)");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_distance_matrix(c->stream, n, x, y, D));
    return FCPP_OK;
}

int fcpp_best_connections(fcpp_ctx *c, int64_t n_pairs, const int64_t *fo, const int64_t *to, const double *fx, const double *fy,
                          const double *tx, const double *ty, int32_t *bf, int32_t *bt, double *bd)
{
    if (!c || n_pairs < 0 || n_pairs > 0x7fffffffLL || (n_pairs > 0 && (!fo || !to || !bf || !bt || !bd)))
        return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_best_connections(c->stream, n_pairs, fo, to, fx, fy, tx, ty, bf, bt, bd));
    return FCPP_OK;
}

}  // extern "C"
