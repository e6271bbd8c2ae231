// fcpp_paths.cpp -- the standalone path operators of include/fcpp.h: curvature, speed plan, verify / validate and the trajectory of
// caller-supplied paths, the Dubins and Reeds-Shepp connectors, the fixed-step samplers, the polygon swaths and the small stateless
// operators, the polygon inset, the swath router, the connector clearance, the field paths, the headland paths, the polygon coverage, its regions and the patch passes over them.  Like fcpp_api.cpp:
// argument checking, device buffers, launches; every path operator drains the context's stream before it returns.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "fcpp_api_internal.h"
#include "fcpp_clear.h"
#include "fcpp_clearfn.h"
#include "fcpp_conn.h"
#include "fcpp_fpathfn.h"
#include "fcpp_hpathfn.h"
#include "fcpp_inset.h"
#include "fcpp_insetfn.h"
#include "fcpp_legs.h"
#include "fcpp_parallel.h"
#include "fcpp_patch.h"
#include "fcpp_patchfn.h"
#include "fcpp_pcover.h"
#include "fcpp_pcoverfn.h"
#include "fcpp_regionfn.h"
#include "fcpp_regions.h"
#include "fcpp_route.h"
#include "fcpp_routefn.h"
#include "fcpp_solveclear.h"
#include "fcpp_swath.h"
#include "fcpp_swathfn.h"
#include "fcpp_traj.h"
#include "fcpp_transit.h"
#include "fcpp_transitfn.h"

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
// CSR offsets on the host, checked: the caller's copy, or read back from the device (one copy + synchronisation)
int host_offsets(fcpp_ctx *c, int64_t n, const int64_t *dev, const int64_t *host, int64_t total, const char *what, std::vector<int64_t> &out)
{
    try { out.assign((size_t)n + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (host) memcpy(out.data(), host, out.size() * sizeof(int64_t));
    else {
        HIPCHK(hipMemcpyAsync(out.data(), dev, out.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (out[0] != 0 || out.back() != total) return fail(FCPP_ESIZE, std::string(what) + " do not span [0, total]");
    for (int64_t p = 0; p < n; ++p)
        if (out[(size_t)p + 1] < out[(size_t)p]) return fail(FCPP_ESIZE, std::string(what) + " must be non-decreasing");
    return FCPP_OK;
}

// m doubles on the host: the caller's copy, or read back from the device into `own` (one copy + synchronisation)
int host_doubles(fcpp_ctx *c, int64_t m, const double *dev, const double *&host, std::vector<double> &own)
{
    if (host || m <= 0) return FCPP_OK;
    try { own.assign((size_t)m, 0.0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    HIPCHK(hipMemcpyAsync(own.data(), dev, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    host = own.data();
    return FCPP_OK;
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

DevConst const_from_vehicle(const fcpp_vehicle &veh)
{
    fcpp_options o;
    fcpp_options_default(&o);
    return make_const(veh, o);
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

// ---- the fixed-step samplers (fcpp_samplefn.h): what fcpp_trajectory_, fcpp_dubins_ and fcpp_rs_counts / _sample share (the count rule itself: fcpp_connfn.h) ----------
// A *_counts entry behind its argument checks: launch(stream, err) fills out_offsets and the error word; both come back, the stream is
// drained, a bad path is FCPP_ESIZE with the entry's message.
template <class Launch>
int sample_counts(fcpp_ctx *c, int64_t n, int64_t *out_offsets, int64_t *out_offsets_host, const char *esize, Launch launch)
{
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf<int64_t> err;
    HIPCHK(err.alloc(1));
    LAUNCHCHK(launch(st, err.p));
    int64_t bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, err.p, sizeof bad, hipMemcpyDeviceToHost, st));
    if (out_offsets_host) HIPCHK(hipMemcpyAsync(out_offsets_host, out_offsets, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return fail(FCPP_ESIZE, esize);
    return FCPP_OK;
}

// An offsets table of a *_sample entry: on the host and checked (of_samples: every path below 2^31 of them), and on the device, where
// the kernel reads it -- uploaded when the caller brought only a host copy.  Lives until the entry has drained the stream.
struct SampleOffsets {
    std::vector<int64_t> host;
    DevBuf<int64_t> up;
    const int64_t *dev = nullptr;
    int get(fcpp_ctx *c, int64_t n, const int64_t *on_dev, const int64_t *on_host, int64_t total, const char *what, bool of_samples)
    {
        const int rc = host_offsets(c, n, on_dev, on_host, total, what, host);
        if (rc) return rc;
        for (int64_t p = 0; of_samples && p < n; ++p)
            if (host[(size_t)p + 1] - host[(size_t)p] > INT32_MAX) return fail(FCPP_ESIZE, "a path has 2^31 samples or more");
        if (!on_dev) HIPCHK(up.upload(host, c->stream));
        dev = on_dev ? on_dev : up.p;
        return FCPP_OK;
    }
};

// ---- connectors: what the Dubins (mode 0) and Reeds-Shepp (mode 1) entries share: the argument checks, the launch ---------------------------
int conn_solve(fcpp_ctx *c, int mode, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
               const double *th, double radius, int32_t *word, double *seg, double *len)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!(radius > 0.0) || !isfinite(radius)) return fail(FCPP_EINVAL, "radius must be positive and finite");
    if (n < 0 || n > ((int64_t)1 << 36)) return fail(FCPP_ESIZE, "bad sizes");
    if (n > 0 && (!fx || !fy || !fh || !tx || !ty || !th)) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_conn_solve(c->stream, mode, n, fx, fy, fh, tx, ty, th, radius, word, seg, len));
    return FCPP_OK;
}

int conn_matrix(fcpp_ctx *c, int mode, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to, const double *tx,
                const double *ty, const double *th, double radius, double *D, int8_t *word)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!(radius > 0.0) || !isfinite(radius)) return fail(FCPP_EINVAL, "radius must be positive and finite");
    if (n_from < 0 || n_to < 0 || n_from > CONN_MAX_POSES || n_to > CONN_MAX_POSES) return fail(FCPP_ESIZE, "bad sizes (at most 2^20 poses per side)");
    if ((n_from > 0 && (!fx || !fy || !fh)) || (n_to > 0 && (!tx || !ty || !th))) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_conn_matrix(c->stream, mode, n_from, fx, fy, fh, n_to, tx, ty, th, radius, D, word));
    return FCPP_OK;
}

int conn_sample(fcpp_ctx *c, int mode, int64_t n, const double *fx, const double *fy, const double *fh, double radius, const int32_t *word,
                const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                double *kappas, int8_t *gears, const int64_t *out_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!(radius > 0.0) || !isfinite(radius)) return fail(FCPP_EINVAL, "radius must be positive and finite");
    if (!(spacing > 0.0) || !isfinite(spacing)) return fail(FCPP_EINVAL, "spacing must be positive and finite");
    if (n < 0 || n > INT32_MAX || total_samples < 0 || total_samples > ((int64_t)1 << 38)) return fail(FCPP_ESIZE, "bad sizes");
    if ((!out_offsets && !out_offsets_host) || (n > 0 && (!fx || !fy || !fh || !word || !seg))) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    SampleOffsets outs;
    const int rc = outs.get(c, n, out_offsets, out_offsets_host, total_samples, "out_offsets", true);
    if (rc) return rc;
    LAUNCHCHK(launch_conn_sample(c->stream, mode, n, fx, fy, fh, radius, word, seg, spacing, outs.dev, total_samples, xs, ys, hs, kappas, gears));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

// ---- polygon swaths: what fcpp_swath_scores / _counts / _fill and fcpp_debug_swaths check alike ------------------------------------
int swath_params(double W, double first, double min_length)
{
    if (!(W > 0.0) || !isfinite(W)) return fail(FCPP_EINVAL, "width must be positive and finite");
    if (!(first >= 0.0) || !(first < W)) return fail(FCPP_EINVAL, "first must lie in [0, width)");
    if (!(min_length >= 0.0) || !isfinite(min_length)) return fail(FCPP_EINVAL, "min_length must be non-negative and finite");
    return FCPP_OK;
}

int swath_sizes(int64_t n, int64_t n_rings, int64_t n_verts, int64_t A)
{
    if (n < 0 || n_rings < 0 || n_verts < 0 || A < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    if (A > 0 && n > SWATH_MAX_PAIRS / A) return fail(FCPP_ESIZE, "2^31 (field, angle) pairs or more");
    return FCPP_OK;
}

// m angles on the host (the caller's, or read back from the device): finite and within fc_sincos' range
int swath_angles(fcpp_ctx *c, int64_t m, const double *dev, const double *host)
{
    std::vector<double> own;
    const int rc = host_doubles(c, m, dev, host, own);
    if (rc) return rc;
    for (int64_t j = 0; j < m; ++j)
        if (!(fabs(host[j]) <= SWATH_MAX_ANGLE)) return fail(FCPP_EINVAL, "angles must be finite, |angle| <= 1e5");
    return FCPP_OK;
}

// the two CSR levels of the fields, brought to the host and checked
int swath_fields(fcpp_ctx *c, int64_t n, const int64_t *ring_dev, const int64_t *ring_host, int64_t n_rings, const int64_t *vert_dev,
                 const int64_t *vert_host, int64_t n_verts, std::vector<int64_t> &rings, std::vector<int64_t> &verts)
{
    int rc = host_offsets(c, n, ring_dev, ring_host, n_rings, "ring_offsets", rings);
    if (rc == FCPP_OK) rc = host_offsets(c, n_rings, vert_dev, vert_host, n_verts, "vert_offsets", verts);
    return rc;
}

// ---- polygon inset: what fcpp_inset_counts / _fill and fcpp_debug_inset check alike --------------------------------------------------
int inset_sizes(int64_t n, int64_t n_rings, int64_t n_verts, int64_t D)
{
    if (n < 0 || n_rings < 0 || n_verts < 0 || D < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    if (D > 0 && n > INSET_MAX_PAIRS / D) return fail(FCPP_ESIZE, "2^31 (field, distance) pairs or more");
    return FCPP_OK;
}

// D distances on the host (the caller's, or read back from the device): positive and finite; arc_step in (0, pi/2]
int inset_params(fcpp_ctx *c, int64_t D, const double *dev, const double *host, double arc_step)
{
    if (!(arc_step > 0.0) || !(arc_step <= INSET_MAX_ARC_STEP)) return fail(FCPP_EINVAL, "arc_step must lie in (0, pi/2]");
    std::vector<double> own;
    const int rc = host_doubles(c, D, dev, host, own);
    if (rc) return rc;
    for (int64_t j = 0; j < D; ++j)
        if (!(host[j] > 0.0) || !isfinite(host[j])) return fail(FCPP_EINVAL, "distances must be positive and finite");
    return FCPP_OK;
}

// the most edges of any field the kernels take
int inset_max_edges(int64_t n, const std::vector<int64_t> &rings, const std::vector<int64_t> &verts)
{
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t E = verts[(size_t)rings[(size_t)i + 1]] - verts[(size_t)rings[(size_t)i]];
        if (E <= INSET_MAX_EDGES) m = std::max(m, E);
    }
    return (int)m;
}

// the piece records of the large fields' launches, alive until the entry has drained the stream
struct InsetScratch {
    DevBuf<double> d;
    DevBuf<int32_t> i;
    int get(int max_edges, int64_t n_pairs)
    {
        size_t nd, ni;
        inset_scratch_size(max_edges, n_pairs, nd, ni);
        if (nd) HIPCHK(d.alloc(nd));
        if (ni) HIPCHK(i.alloc(ni));
        return FCPP_OK;
    }
};

// ---- swath router: what fcpp_route_transit / _solve and their host twins check alike ---------------------------------------------------
int route_radius(double radius, int mode)
{
    if (!(radius > 0.0) || !isfinite(radius)) return fail(FCPP_EINVAL, "radius must be positive and finite");
    if (mode != 0 && mode != 1) return fail(FCPP_EINVAL, "mode must be 0 (Dubins) or 1 (Reeds-Shepp)");
    return FCPP_OK;
}

int route_search(int S, double min_gain, int max_sweeps)
{
    if (S < 1 || S > ROUTE_MAX_STARTS) return fail(FCPP_EINVAL, "n_starts must lie in 1 .. 64");
    if (!(min_gain >= 0.0) || !isfinite(min_gain)) return fail(FCPP_EINVAL, "min_gain must be non-negative and finite");
    if (max_sweeps < 0 || max_sweeps > ROUTE_MAX_SWEEPS) return fail(FCPP_EINVAL, "max_sweeps must lie in 0 .. 2^20");
    return FCPP_OK;
}

// the swath offsets and the block offsets on the host, checked against each other: block i holds (2 m_i)^2 entries, none beyond the cap
int route_offsets(fcpp_ctx *c, int64_t n, const int64_t *soff_dev, const int64_t *soff_host, int64_t n_total, const int64_t *toff_dev,
                  const int64_t *toff_host, int64_t t_total, std::vector<int64_t> &soff, std::vector<int64_t> &toff)
{
    if (n < 0 || n_total < 0 || t_total < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    int rc = host_offsets(c, n, soff_dev, soff_host, n_total, "swath_offsets", soff);
    if (rc == FCPP_OK) rc = host_offsets(c, n, toff_dev, toff_host, t_total, "t_offsets", toff);
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (toff[(size_t)i + 1] - toff[(size_t)i] != route_block(soff[(size_t)i + 1] - soff[(size_t)i]))
            return fail(FCPP_ESIZE, "t_offsets do not match the swath counts: block i holds (2 m_i)^2 entries, none for m_i > 512");
    return FCPP_OK;
}

// ---- connector clearance: what fcpp_conn_clear / fcpp_route_transit_clear and their host twins check alike -----------------------------------
int clear_conn_args(int mode, int64_t n, const double *fx, const double *fy, const double *fh, double radius, const int32_t *word, const double *seg,
                    const int64_t *pair_field, int64_t n_fields, const void *ring_offsets, int64_t n_rings, const void *vert_offsets,
                    int64_t n_verts, const double *x, const double *y)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y)) || (n > 0 && (!fx || !fy || !fh || !word || !seg || !pair_field)))
        return fail(FCPP_EINVAL, "bad arguments");
    const int rc = route_radius(radius, mode);
    if (rc) return rc;
    if (n < 0 || n_fields < 0 || n_rings < 0 || n_verts < 0 || n_fields > INT32_MAX || (n + CLEAR_TILE - 1) / CLEAR_TILE > CLEAR_MAX_GROUPS)
        return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

int clear_penalty(double penalty)
{
    if (!(penalty >= 0.0) || !isfinite(penalty)) return fail(FCPP_EINVAL, "penalty must be non-negative and finite");
    return FCPP_OK;
}

// the workgroups of k_clear_transit: CLEAR_TILE entries of one field's block each
int clear_tiles(int64_t n, const std::vector<int64_t> &toff, std::vector<int64_t> &tile_off)
{
    try { tile_off.assign((size_t)n + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (int64_t i = 0; i < n; ++i)
        tile_off[(size_t)i + 1] = tile_off[(size_t)i] + (toff[(size_t)i + 1] - toff[(size_t)i] + CLEAR_TILE - 1) / CLEAR_TILE;
    if (tile_off[(size_t)n] > CLEAR_MAX_GROUPS) return fail(FCPP_ESIZE, "2^39 transit entries or more");
    return FCPP_OK;
}

// ---- clear connectors: what fcpp_conn_solve_clear and its host twin check alike
int solve_clear_args(int mode, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
                            const double *th, double radius, const int64_t *pair_field, int64_t n_fields, const void *ring_offsets, int64_t n_rings,
                            const void *vert_offsets, int64_t n_verts, const double *x, const double *y)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y)) || (n > 0 && (!fx || !fy || !fh || !tx || !ty || !th || !pair_field)))
        return fail(FCPP_EINVAL, "bad arguments");
    const int rc = route_radius(radius, mode);
    if (rc) return rc;
    // (n below 2^31: the word kernel's grid, a wavefront per pair at most)
    if (n < 0 || n_fields < 0 || n_rings < 0 || n_verts < 0 || n_fields > INT32_MAX || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

// every candidate of every pair: fcpp_debug_conn_words
template <int MODE>
void debug_conn_words(int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty, const double *th,
                             double radius, uint8_t *ok, double *seg, double *total)
{
    constexpr int NW = SolveClearWords<MODE>::NW, NSEG = Conn<MODE>::NSEG;
    WorkerPool::parallel_for(n, [&](int64_t i) {
        SolveClearAll<MODE> all;
        const bool fin = solve_clear_words<MODE>(fx[i], fy[i], fh[i], tx[i], ty[i], th[i], radius, all);
        for (int w = 0; w < NW; ++w) {
            const bool have = fin && all.ok[w];
            if (ok) ok[i * NW + w] = have ? 1 : 0;
            if (total) total[i * NW + w] = have ? all.total[w] : __builtin_nan("");
            if (seg)
                for (int k = 0; k < NSEG; ++k) seg[(i * NW + w) * NSEG + k] = have ? all.seg[w][k] : __builtin_nan("");
        }
    });
}

// ---- field paths: what fcpp_field_path_counts / _fill and fcpp_debug_field_paths check alike ------------------------------------------------
// the arguments that need no offsets: NULLs, the poses' triples, radius, mode, spacing, the sizes
int fpath_args(int64_t n, const void *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx, const double *by,
               const double *length, const double *angle, double radius, int mode, double spacing, const double *ex, const double *ey,
               const double *eh, const double *xx, const double *xy, const double *xh)
{
    if (!swath_offsets || (n_total > 0 && (!ax || !ay || !bx || !by || !length)) || (n > 0 && !angle)) return fail(FCPP_EINVAL, "bad arguments");
    if (((ex || ey || eh) && !(ex && ey && eh)) || ((xx || xy || xh) && !(xx && xy && xh)))
        return fail(FCPP_EINVAL, "an entry or exit pose takes all three of x, y and heading");
    const int rc = route_radius(radius, mode);
    if (rc) return rc;
    if (!(spacing > 0.0) || !isfinite(spacing)) return fail(FCPP_EINVAL, "spacing must be positive and finite");
    if (n < 0 || n_total < 0 || n > INT32_MAX || n_total > FPATH_MAX_SWATHS) return fail(FCPP_ESIZE, "bad sizes (at most 2^30 swaths)");
    return FCPP_OK;
}

// the swath offsets on the host and the angles, checked (read back from the device where the caller has no host copy)
int fpath_offsets(fcpp_ctx *c, int64_t n, const int64_t *soff_dev, const int64_t *soff_host, int64_t n_total, const double *angle_dev,
                  const double *angle_host, std::vector<int64_t> &soff)
{
    int rc = host_offsets(c, n, soff_dev, soff_host, n_total, "swath_offsets", soff);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle_dev, angle_host);
    return rc;
}

// ---- headland paths: what fcpp_headland_path_counts / _fill and fcpp_debug_headland_paths check alike --------------------------------------
int hpath_args(int64_t n_rings, const void *ring_offsets, int64_t n_verts, const double *x, const double *y, const int32_t *src,
               const double *ring_dist, double radius, int mode, double spacing, int direction, double smooth_tol)
{
    if (!ring_offsets || (n_verts > 0 && (!x || !y || !src)) || (n_rings > 0 && !ring_dist)) return fail(FCPP_EINVAL, "bad arguments");
    const int rc = route_radius(radius, mode);
    if (rc) return rc;
    if (!(spacing > 0.0) || !isfinite(spacing)) return fail(FCPP_EINVAL, "spacing must be positive and finite");
    if (direction != 1 && direction != -1) return fail(FCPP_EINVAL, "direction must be +1 (as stored) or -1");
    if (!(smooth_tol >= 0.0)) return fail(FCPP_EINVAL, "smooth_tol must not be negative");
    if (n_rings < 0 || n_verts < 0 || n_rings > INT32_MAX || n_verts > HPATH_MAX_VERTS) return fail(FCPP_ESIZE, "bad sizes (at most 2^30 vertices)");
    return FCPP_OK;
}
// ---- leg paths: what the field paths' and the headland paths' three entries are behind their argument checks, on the leg set P ------------
// (FieldLegs / RingLegs of the rule headers; the kernels: fcpp_legs.hip).  A fill RECOMPUTES the leg records from its inputs (one more
// launch of the rule kernel) instead of keeping the counts call's in the context: the entries stay stateless, and the solves are a small
// part of the samples' cost.
// *_counts: the temporaries (n_scratch: the int32 scratch of the rule kernel), the call's own status buffer when the caller passes none
// stage(stream, legs, cnt, status) -> 0 or a hipError_t value: what an entry does to the records between the rule kernel and the scan
struct NoLegStage {
    template <class Leg> int operator()(hipStream_t, Leg *, int64_t *, const int32_t *) const { return 0; }
};

template <class P, class Stage = NoLegStage>
int legs_counts(fcpp_ctx *c, int64_t n_groups, int64_t n_slots, int64_t n_scratch, const typename P::In &in, int mode, const char *esize,
                int64_t *path_offsets, int64_t *path_offsets_host, int64_t *leg_offsets, const LegTotals &totals, int32_t *status,
                Stage &&stage = Stage())
{
    DevBuf<typename P::Leg> legs;
    DevBuf<int64_t> cnt;
    DevBuf<int32_t> scratch, own_status;
    HIPCHK(legs.alloc((size_t)n_slots));
    HIPCHK(cnt.alloc((size_t)n_slots));
    HIPCHK(scratch.alloc((size_t)n_scratch));
    if (!status) { HIPCHK(own_status.alloc((size_t)n_groups)); status = own_status.p; }
    return sample_counts(c, n_groups, path_offsets, path_offsets_host, esize, [&](hipStream_t st, int64_t *err) {
        if (n_scratch > 0) { const hipError_t e = hipMemsetAsync(scratch.p, 0, (size_t)n_scratch * sizeof(int32_t), st); if (e != hipSuccess) return (int)e; }
        if (n_groups > 0) { const hipError_t e = hipMemsetAsync(status, 0, (size_t)n_groups * sizeof(int32_t), st); if (e != hipSuccess) return (int)e; }
        int e = launch_legs(st, n_groups, n_slots, in, mode, legs.p, cnt.p, scratch.p, status);
        if (e == 0) e = stage(st, legs.p, cnt.p, status);
        return e ? e : launch_leg_offsets(st, n_groups, n_slots, in, legs.p, cnt.p, status, scratch.p, leg_offsets, path_offsets, totals, err);
    });      // (sample_counts has drained the stream: the temporaries die here)
}

// *_fill.  The ends of the slot offsets must match the output arrays.  (The fill writes sample q < total_samples of every array and reads
// the record of a slot below n_slots whatever lies between the ends: offsets that are not the counts call's give wrong samples, never an
// access outside the arrays.)
template <class P, class Stage = NoLegStage>
int legs_fill(fcpp_ctx *c, int64_t n_groups, int64_t n_slots, const typename P::In &in, int mode, const int64_t *leg_offsets, int64_t total_samples,
              double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg, Stage &&stage = Stage())
{
    int64_t ends[2] = { 0, 0 };
    HIPCHK(hipMemcpyAsync(&ends[0], leg_offsets, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&ends[1], leg_offsets + n_slots, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (ends[0] != 0 || ends[1] != total_samples) return fail(FCPP_ESIZE, "leg_offsets do not span [0, total_samples]");
    DevBuf<typename P::Leg> legs;
    HIPCHK(legs.alloc((size_t)n_slots));
    LAUNCHCHK(launch_legs(c->stream, n_groups, n_slots, in, mode, legs.p, nullptr, nullptr, nullptr));
    LAUNCHCHK(stage(c->stream, legs.p, (int64_t *)nullptr, (const int32_t *)nullptr));
    LAUNCHCHK(launch_leg_fill<P>(c->stream, n_slots, legs.p, leg_offsets, total_samples, in.R, in.spacing, x, y, heading, kappa, part, gear, leg));
    HIPCHK(hipStreamSynchronize(c->stream));      // (the records die here)
    return FCPP_OK;
}

// fcpp_debug_*: group(g, legs, cnt, t, oversize) -> status is the rule's host twin of one group (its records, its counts -- in off, one
// slot ahead: scanned below -- and its totals); groups go to the library's host threads.  `in` holds host pointers.
template <class P, class Group>
int legs_host(int64_t n_groups, int64_t n_slots, const typename P::In &in, const char *esize, Group group, int64_t *path_offsets, int64_t *leg_offsets,
              const LegTotals &totals, int32_t *status, int32_t *leg_kind, int32_t *leg_word, double *leg_seg, double *leg_total, int64_t cap, double *x,
              double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    std::vector<typename P::Leg> legs;
    std::vector<int64_t> off;
    std::vector<char> big;
    try {
        legs.resize((size_t)n_slots); off.assign((size_t)n_slots + 1, 0); big.assign((size_t)n_groups, 0);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    WorkerPool::parallel_for(n_groups, [&](int64_t g) {
        const int64_t first = P::first_slot(in, g);
        double t[P::N_TOTALS];
        bool oversize;
        const int st = group(g, legs.data() + first, off.data() + first + 1, t, oversize);
        big[(size_t)g] = oversize;
        if (status) status[g] = st;
        for (int k = 0; k < P::N_TOTALS; ++k)
            if (totals.p[k]) totals.p[k][g] = t[k];
    });
    for (int64_t g = 0; g < n_groups; ++g)
        if (big[(size_t)g]) return fail(FCPP_ESIZE, esize);
    for (int64_t p = 0; p < n_slots; ++p) {
        off[(size_t)p + 1] += off[(size_t)p];
        const FpathLeg &lg = P::base(legs[(size_t)p]);
        if (leg_kind) leg_kind[p] = lg.kind;
        if (leg_word) leg_word[p] = lg.kind == FPATH_DUBINS || lg.kind == FPATH_RS ? lg.word : -1;
        if (leg_seg) for (int k = 0; k < 5; ++k) leg_seg[5 * p + k] = lg.seg[k];
        if (leg_total) leg_total[p] = lg.total;
    }
    if (leg_offsets) memcpy(leg_offsets, off.data(), off.size() * sizeof(int64_t));
    if (path_offsets) {
        for (int64_t g = 0; g < n_groups; ++g) path_offsets[g] = off[(size_t)P::first_slot(in, g)];
        path_offsets[n_groups] = off[(size_t)n_slots];
    }
    if (cap == 0 || !(x || y || heading || kappa || part || gear || leg)) return FCPP_OK;
    WorkerPool::parallel_for(n_groups, [&](int64_t g) {
        for (int64_t p = P::first_slot(in, g); p < P::first_slot(in, g + 1); ++p) {
            const typename P::Leg &lg = legs[(size_t)p];
            const int64_t at = off[(size_t)p], K = off[(size_t)p + 1] - at;
            for (int64_t k = 0; k < K && at + k < cap; ++k) {
                double px, py, ph, pk;
                int pg;
                P::eval(lg, in.R, in.spacing, k, K, px, py, ph, pk, pg);
                if (x) x[at + k] = px;
                if (y) y[at + k] = py;
                if (heading) heading[at + k] = ph;
                if (kappa) kappa[at + k] = pk;
                if (part) part[at + k] = (int8_t)P::base(lg).part;
                if (gear) gear[at + k] = (int8_t)pg;
                if (leg) leg[at + k] = P::base(lg).slot;
            }
        }
    });
    return FCPP_OK;
}

// ---- the clear field paths: what the records go through between the rule kernel and the scan (kernels: fcpp_solveclear.hip) -----------------
// First pass, the list's length read back, the second pass unless it is 0, then (a counts call) the per-slot and per-field reports.  The
// fill passes no outputs: records only.  The buffers live in the stage, which outlives the entry's last synchronisation.
struct FpathClearStage {
    fcpp_ctx *c;
    int mode;
    int64_t n, n_total;
    FpathIn in;
    ClearFields F;
    int32_t *rank = nullptr, *crossings = nullptr, *leg_word = nullptr;
    double *leg_seg = nullptr, *leg_total = nullptr;
    int32_t *blocked = nullptr, *reshaped = nullptr, *region_status = nullptr;
    DevBuf<int64_t> list;
    DevBuf<unsigned long long> count;
    DevBuf<int32_t> own_rank;

    int operator()(hipStream_t st, FpathLeg *legs, int64_t *cnt, const int32_t *status)
    {
        const int64_t n_conn = n_total + n, n_slots = 2 * n_total + n;
        c->fpath_clear_listed = 0;
        if (n <= 0) return 0;
        hipError_t e = (hipError_t)launch_clear_field_status(st, F, region_status);
        if (e == hipSuccess) e = list.alloc((size_t)n_conn);
        if (e == hipSuccess) e = count.alloc(1);
        if (e == hipSuccess && !rank && (blocked || reshaped)) { e = own_rank.alloc((size_t)n_slots); rank = own_rank.p; }
        if (e == hipSuccess) e = hipMemsetAsync(count.p, 0, sizeof(unsigned long long), st);
        if (e == hipSuccess && rank) e = hipMemsetAsync(rank, 0, (size_t)n_slots * sizeof(int32_t), st);
        if (e == hipSuccess && crossings) e = hipMemsetAsync(crossings, 0, (size_t)n_slots * sizeof(int32_t), st);
        if (e != hipSuccess) return (int)e;
        int rc = launch_fpath_clear_slots(st, mode, n, n_conn, in.soff, in.R, legs, status, F, rank, crossings, list.p, count.p);
        if (rc) return rc;
        unsigned long long listed = 0;
        e = hipMemcpyAsync(&listed, count.p, sizeof listed, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        if (listed > (unsigned long long)n_conn) return (int)hipErrorUnknown;      // (more slots listed than there are)
        c->fpath_clear_listed = (int64_t)listed;
        if (listed > 0) {
            rc = launch_fpath_clear_words(st, mode, (int64_t)listed, list.p, in, F, legs, cnt, rank, crossings);
            if (rc) return rc;
            ++c->fpath_clear_word_launches;
        }
        return launch_fpath_clear_report(st, n, n_slots, in.soff, legs, rank, leg_word, leg_seg, leg_total, blocked, reshaped);
    }
};

// the region CSR of the clear field paths: what fcpp_conn_clear checks of its fields, for n fields
int fpath_region_args(int64_t n, const void *ring_offsets, int64_t n_rings, const void *vert_offsets, int64_t n_verts, const double *x, const double *y)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y))) return fail(FCPP_EINVAL, "bad arguments");
    if (n < 0 || n_rings < 0 || n_verts < 0) return fail(FCPP_ESIZE, "bad sizes");
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

// ---- Dubins and Reeds-Shepp connectors (fcpp_conn.hip; the mathematics: fcpp_dubinsfn.h / fcpp_rsfn.h) -----------------------------------
int fcpp_dubins_solve(fcpp_ctx *c, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
                      const double *th, double radius, int32_t *word, double *seg, double *len)
{
    return conn_solve(c, 0, n, fx, fy, fh, tx, ty, th, radius, word, seg, len);
}

int fcpp_rs_solve(fcpp_ctx *c, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
                  const double *th, double radius, int32_t *word, double *seg, double *len)
{
    return conn_solve(c, 1, n, fx, fy, fh, tx, ty, th, radius, word, seg, len);
}

int fcpp_dubins_matrix(fcpp_ctx *c, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to, const double *tx,
                       const double *ty, const double *th, double radius, double *D, int8_t *word)
{
    return conn_matrix(c, 0, n_from, fx, fy, fh, n_to, tx, ty, th, radius, D, word);
}

int fcpp_rs_matrix(fcpp_ctx *c, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to, const double *tx,
                   const double *ty, const double *th, double radius, double *D, int8_t *word)
{
    return conn_matrix(c, 1, n_from, fx, fy, fh, n_to, tx, ty, th, radius, D, word);
}

int fcpp_dubins_counts(fcpp_ctx *c, int64_t n, const double *len, double spacing, int64_t *out_offsets, int64_t *out_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!(spacing > 0.0) || !isfinite(spacing)) return fail(FCPP_EINVAL, "spacing must be positive and finite");
    if (n < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    if (!out_offsets || (n > 0 && !len)) return fail(FCPP_EINVAL, "bad arguments");
    return sample_counts(c, n, out_offsets, out_offsets_host, "a path's length is negative or infinite, or it has 2^31 samples or more",
                         [&](hipStream_t st, int64_t *err) { return launch_dubins_counts(st, n, len, spacing, out_offsets, err); });
}

int fcpp_rs_counts(fcpp_ctx *c, int64_t n, const int32_t *word, const double *seg, double spacing, int64_t *out_offsets, int64_t *out_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!(spacing > 0.0) || !isfinite(spacing)) return fail(FCPP_EINVAL, "spacing must be positive and finite");
    if (n < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    if (!out_offsets || (n > 0 && (!word || !seg))) return fail(FCPP_EINVAL, "bad arguments");
    return sample_counts(c, n, out_offsets, out_offsets_host, "a path has an infinite segment, or 2^31 samples or more",
                         [&](hipStream_t st, int64_t *err) { return launch_rs_counts(st, n, word, seg, spacing, out_offsets, err); });
}

int fcpp_dubins_sample(fcpp_ctx *c, int64_t n, const double *fx, const double *fy, const double *fh, double radius, const int32_t *word,
                       const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                       double *kappas, const int64_t *out_offsets_host)
{
    return conn_sample(c, 0, n, fx, fy, fh, radius, word, seg, spacing, out_offsets, total_samples, xs, ys, hs, kappas, nullptr, out_offsets_host);
}

int fcpp_rs_sample(fcpp_ctx *c, int64_t n, const double *fx, const double *fy, const double *fh, double radius, const int32_t *word,
                   const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                   double *kappas, int8_t *gears, const int64_t *out_offsets_host)
{
    return conn_sample(c, 1, n, fx, fy, fh, radius, word, seg, spacing, out_offsets, total_samples, xs, ys, hs, kappas, gears, out_offsets_host);
}

// ---- polygon swaths (fcpp_swath.hip; the rule: fcpp_swathfn.h) --------------------------------------------------------------------
int fcpp_swath_scores(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                      const double *x, const double *y, int64_t A, const double *angles, double W, double first, double min_length,
                      int32_t *n_swaths, int32_t *n_lines, double *length, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y)) || (A > 0 && !angles)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = swath_params(W, first, min_length);
    if (rc == FCPP_OK) rc = swath_sizes(n, n_rings, n_verts, A);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> rings, verts;
    rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(c, A, angles, nullptr);
    if (rc) return rc;
    LAUNCHCHK(launch_swath_count(c->stream, n, A, 0, ring_offsets, vert_offsets, x, y, angles, W, first, min_length, n_swaths, n_lines, length, status));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_swath_counts(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                      const double *x, const double *y, const double *angle, double W, double first, double min_length, int64_t *out_offsets,
                      int64_t *out_offsets_host, int32_t *n_lines, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!ring_offsets || !vert_offsets || !out_offsets || (n_verts > 0 && (!x || !y)) || (n > 0 && !angle)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = swath_params(W, first, min_length);
    if (rc == FCPP_OK) rc = swath_sizes(n, n_rings, n_verts, 1);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> rings, verts;
    rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    if (rc) return rc;
    DevBuf<int32_t> n_swaths;
    HIPCHK(n_swaths.alloc((size_t)n));
    return sample_counts(c, n, out_offsets, out_offsets_host, "the swath counts could not be scanned", [&](hipStream_t st, int64_t *err) {
        const int e = launch_swath_count(st, n, 1, 1, ring_offsets, vert_offsets, x, y, angle, W, first, min_length, n_swaths.p, n_lines, nullptr, status);
        return e ? e : launch_swath_offsets(st, n, n_swaths.p, out_offsets, err);
    });
}

int fcpp_swath_fill(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                    const double *x, const double *y, const double *angle, double W, double first, double min_length, const int64_t *offsets,
                    int64_t n_total, double *ax, double *ay, double *bx, double *by, int32_t *line, double *length)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!ring_offsets || !vert_offsets || !offsets || (n_verts > 0 && (!x || !y)) || (n > 0 && !angle)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = swath_params(W, first, min_length);
    if (rc == FCPP_OK) rc = swath_sizes(n, n_rings, n_verts, 1);
    if (rc == FCPP_OK && n_total < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> rings, verts;
    rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    SampleOffsets outs;
    if (rc == FCPP_OK) rc = outs.get(c, n, offsets, nullptr, n_total, "offsets", true);
    if (rc) return rc;
    LAUNCHCHK(launch_swath_fill(c->stream, n, ring_offsets, vert_offsets, x, y, angle, W, first, min_length, outs.dev, ax, ay, bx, by, line, length));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_swaths(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                      const double *y, int64_t A, const double *angles, int per_field, double W, double first, double min_length,
                      int32_t *n_swaths, int32_t *n_lines, double *length, int32_t *status, int64_t *out_offsets, int64_t cap, double *ax,
                      double *ay, double *bx, double *by, int32_t *line, double *seg_length)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y)) || (A > 0 && n > 0 && !angles)) return fail(FCPP_EINVAL, "bad arguments");
    if ((per_field || out_offsets) && A != 1) return fail(FCPP_EINVAL, "per-field angles and records take A = 1");
    int rc = swath_params(W, first, min_length);
    if (rc == FCPP_OK) rc = swath_sizes(n, n_rings, n_verts, A);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> rings, verts;
    rc = swath_fields(nullptr, n, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, per_field ? n : A, nullptr, angles);
    if (rc) return rc;
    std::vector<double> u, w;
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t nv = verts[(size_t)rings[(size_t)i + 1]] - verts[(size_t)rings[(size_t)i]];
        try { u.resize((size_t)nv); w.resize((size_t)nv); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
        if (out_offsets) out_offsets[i] = at;
        for (int64_t j = 0; j < A; ++j) {
            const SwathTotals t = swath_field_host(verts.data(), rings[(size_t)i], rings[(size_t)i + 1], x, y, angles[per_field ? i : j], W, first, min_length,
                                                   u.data(), w.data(), [&](int64_t k, double ua, double ub, double wk, double c, double s, double len) {
                if (!out_offsets) return;
                if (at < cap) {
                    double px, py, qx, qy;
                    swath_point(ua, wk, c, s, px, py);
                    swath_point(ub, wk, c, s, qx, qy);
                    if (ax) ax[at] = px;
                    if (ay) ay[at] = py;
                    if (bx) bx[at] = qx;
                    if (by) by[at] = qy;
                    if (line) line[at] = (int32_t)k;
                    if (seg_length) seg_length[at] = len;
                }
                ++at;
            });
            if (n_swaths) n_swaths[i * A + j] = t.n_swaths;
            if (n_lines) n_lines[i * A + j] = t.n_lines;
            if (length) length[i * A + j] = t.length;
            if (status) status[i * A + j] = t.status;
        }
    }
    if (out_offsets) out_offsets[n] = at;
    return FCPP_OK;
}

// ---- polygon inset (fcpp_inset.hip; the rule: fcpp_insetfn.h) -----------------------------------------------------------------------
int fcpp_inset_counts(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                      const double *x, const double *y, int64_t D, const double *dist, double arc_step, int64_t *pair_ring_offsets,
                      int64_t *pair_ring_offsets_host, int64_t *pair_vert_offsets, int64_t *pair_vert_offsets_host, int32_t *status, double *gap)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!ring_offsets || !vert_offsets || !pair_ring_offsets || !pair_vert_offsets || (n_verts > 0 && (!x || !y)) || (D > 0 && !dist))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = inset_sizes(n, n_rings, n_verts, D);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = inset_params(c, D, dist, nullptr, arc_step);
    std::vector<int64_t> rings, verts;
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const int64_t m = n * D;
    const int max_edges = inset_max_edges(n, rings, verts);
    hipStream_t st = c->stream;
    InsetScratch scratch;
    rc = scratch.get(max_edges, m);
    if (rc) return rc;
    DevBuf<int32_t> counts;
    DevBuf<int64_t> err;
    HIPCHK(counts.alloc((size_t)(2 * m + 1)));
    HIPCHK(err.alloc(2));
    LAUNCHCHK(launch_inset_count(st, n, D, max_edges, ring_offsets, vert_offsets, x, y, dist, arc_step, scratch.d.p, scratch.i.p, counts.p, counts.p + m,
                                 status, gap));
    LAUNCHCHK(launch_inset_offsets(st, m, counts.p, pair_ring_offsets, err.p));
    LAUNCHCHK(launch_inset_offsets(st, m, counts.p + m, pair_vert_offsets, err.p + 1));
    int64_t bad[2] = { 0, 0 };
    HIPCHK(hipMemcpyAsync(bad, err.p, sizeof bad, hipMemcpyDeviceToHost, st));
    if (pair_ring_offsets_host) HIPCHK(hipMemcpyAsync(pair_ring_offsets_host, pair_ring_offsets, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (pair_vert_offsets_host) HIPCHK(hipMemcpyAsync(pair_vert_offsets_host, pair_vert_offsets, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad[0] || bad[1]) return fail(FCPP_ESIZE, "the inset counts could not be scanned");
    return FCPP_OK;
}

int fcpp_inset_fill(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                    const double *x, const double *y, int64_t D, const double *dist, double arc_step, const int64_t *pair_ring_offsets,
                    const int64_t *pair_vert_offsets, int64_t total_rings, int64_t total_verts, int64_t *out_vert_offsets, double *out_x,
                    double *out_y, int32_t *out_src)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!ring_offsets || !vert_offsets || !pair_ring_offsets || !pair_vert_offsets || (n_verts > 0 && (!x || !y)) || (D > 0 && !dist))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = inset_sizes(n, n_rings, n_verts, D);
    if (rc == FCPP_OK && (total_rings < 0 || total_verts < 0)) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = inset_params(c, D, dist, nullptr, arc_step);
    std::vector<int64_t> rings, verts, pro, pvo;
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = host_offsets(c, n * D, pair_ring_offsets, nullptr, total_rings, "pair_ring_offsets", pro);
    if (rc == FCPP_OK) rc = host_offsets(c, n * D, pair_vert_offsets, nullptr, total_verts, "pair_vert_offsets", pvo);
    if (rc) return rc;
    const int max_edges = inset_max_edges(n, rings, verts);
    InsetScratch scratch;
    rc = scratch.get(max_edges, n * D);
    if (rc) return rc;
    LAUNCHCHK(launch_inset_fill(c->stream, n, D, max_edges, ring_offsets, vert_offsets, x, y, dist, arc_step, scratch.d.p, scratch.i.p, pair_ring_offsets,
                                pair_vert_offsets, total_rings, total_verts, out_vert_offsets, out_x, out_y, out_src));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_inset(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                     const double *y, int64_t D, const double *dist, double arc_step, int64_t *pair_ring_offsets, int64_t *pair_vert_offsets,
                     int32_t *status, double *gap, int64_t ring_cap, int64_t vert_cap, int64_t *out_vert_offsets, double *out_x, double *out_y,
                     int32_t *out_src)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y)) || (D > 0 && !dist)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = inset_sizes(n, n_rings, n_verts, D);
    if (rc == FCPP_OK && (ring_cap < 0 || vert_cap < 0)) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc == FCPP_OK) rc = inset_params(nullptr, D, nullptr, dist, arc_step);
    std::vector<int64_t> rings, verts;
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc) return rc;
    int64_t ring_at = 0, vert_at = 0;
    try {
        InsetWork work;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < D; ++j) {
                const int64_t pair = i * D + j;
                if (pair_ring_offsets) pair_ring_offsets[pair] = ring_at;
                if (pair_vert_offsets) pair_vert_offsets[pair] = vert_at;
                const InsetTotals t = inset_field_host(verts.data(), rings[(size_t)i], rings[(size_t)i + 1], x, y, dist[j], arc_step, work,
                    [&](int32_t r, int32_t off) { if (out_vert_offsets && ring_at + r < ring_cap) out_vert_offsets[ring_at + r] = vert_at + off; },
                    [&](int32_t at, double vx, double vy, int32_t src) {
                        if (vert_at + at >= vert_cap) return;
                        if (out_x) out_x[vert_at + at] = vx;
                        if (out_y) out_y[vert_at + at] = vy;
                        if (out_src) out_src[vert_at + at] = src;
                    });
                if (status) status[pair] = t.status;
                if (gap) gap[pair] = t.gap;
                ring_at += t.n_rings;
                vert_at += t.n_verts;
            }
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (pair_ring_offsets) pair_ring_offsets[n * D] = ring_at;
    if (pair_vert_offsets) pair_vert_offsets[n * D] = vert_at;
    if (out_vert_offsets && ring_at <= ring_cap) out_vert_offsets[ring_at] = vert_at;
    return FCPP_OK;
}

// ---- swath router (fcpp_route.hip; the rule: fcpp_routefn.h) ------------------------------------------------------------------------
int fcpp_route_transit(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                       const double *ax, const double *ay, const double *bx, const double *by, const double *angle, double radius, int mode,
                       const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, double *T)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!swath_offsets || !t_offsets || (n_total > 0 && (!ax || !ay || !bx || !by)) || (n > 0 && !angle) || (t_total > 0 && !T))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc == FCPP_OK && (t_total + 255) / 256 > ROUTE_MAX_GROUPS) rc = fail(FCPP_ESIZE, "2^39 transit entries or more");
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    if (rc) return rc;
    LAUNCHCHK(launch_route_transit(c->stream, n, swath_offsets, ax, ay, bx, by, angle, radius, mode, t_offsets, t_total, T));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_route_solve(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                     const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, const double *T, const double *E, const double *X,
                     int n_starts, double min_gain, int max_sweeps, int32_t *tours, double *costs, int32_t *route, double *cost, int32_t *winner,
                     int32_t *sweeps, int32_t *status, double *stored)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!swath_offsets || !t_offsets || (t_total > 0 && !T)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_search(n_starts, min_gain, max_sweeps);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc == FCPP_OK && n > ROUTE_MAX_GROUPS / n_starts) rc = fail(FCPP_ESIZE, "2^31 (field, candidate) pairs or more");
    if (rc) return rc;
    // what the pick reads is the solve's own when the caller does not want it
    DevBuf<int32_t> own_tours, applied;
    DevBuf<double> own_costs, own_stored;
    if (!tours) { HIPCHK(own_tours.alloc((size_t)n_starts * (size_t)n_total)); tours = own_tours.p; }
    if (!costs) { HIPCHK(own_costs.alloc((size_t)n * (size_t)n_starts)); costs = own_costs.p; }
    if (!stored) { HIPCHK(own_stored.alloc((size_t)n)); stored = own_stored.p; }
    HIPCHK(applied.alloc((size_t)n * (size_t)n_starts));
    LAUNCHCHK(launch_route_solve(c->stream, n, n_starts, swath_offsets, n_total, t_offsets, T, E, X, min_gain, max_sweeps, tours, costs, applied.p,
                                 stored));
    LAUNCHCHK(launch_route_pick(c->stream, n, n_starts, swath_offsets, n_total, tours, costs, applied.p, stored, route, cost, winner, sweeps, status));
    HIPCHK(hipStreamSynchronize(c->stream));      // (the temporaries die here)
    return FCPP_OK;
}

int fcpp_debug_route_transit(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                             const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total, double *T)
{
    if (!swath_offsets || !t_offsets || (n_total > 0 && (!ax || !ay || !bx || !by)) || (n > 0 && !angle) || (t_total > 0 && !T))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc) return rc;
    std::vector<int64_t> soff, toff;
    rc = route_offsets(nullptr, n, nullptr, swath_offsets, n_total, nullptr, t_offsets, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, n, nullptr, angle);
    if (rc) return rc;
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const int64_t s0 = soff[(size_t)i];
        const int N = (int)(toff[(size_t)i + 1] == toff[(size_t)i] ? 0 : 2 * (soff[(size_t)i + 1] - s0));
        double *blk = T + toff[(size_t)i];
        for (int p = 0; p < N; ++p)
            for (int q = 0; q < N; ++q) {
                if (!route_canonical(p, q, N)) continue;
                const double v = mode == 0 ? route_transit<0>(ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, p, q)
                                           : route_transit<1>(ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, p, q);
                blk[p * N + q] = v;
                blk[(q ^ 1) * N + (p ^ 1)] = v;
            }
    });
    return FCPP_OK;
}

int fcpp_debug_route(int64_t n, const int64_t *swath_offsets, int64_t n_total, const int64_t *t_offsets, int64_t t_total, const double *T,
                     const double *E, const double *X, int n_starts, double min_gain, int max_sweeps, int32_t *tours, double *costs, int32_t *route,
                     double *cost, int32_t *winner, int32_t *sweeps, int32_t *status, double *stored)
{
    if (!swath_offsets || !t_offsets || (t_total > 0 && !T)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_search(n_starts, min_gain, max_sweeps);
    if (rc) return rc;
    std::vector<int64_t> soff, toff;
    rc = route_offsets(nullptr, n, nullptr, swath_offsets, n_total, nullptr, t_offsets, t_total, soff, toff);
    if (rc == FCPP_OK && n > ROUTE_MAX_GROUPS / n_starts) rc = fail(FCPP_ESIZE, "2^31 (field, candidate) pairs or more");
    if (rc) return rc;
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const int64_t s0 = soff[(size_t)i];
        const RouteField f = route_field_host(T + toff[(size_t)i], E ? E + 2 * s0 : nullptr, X ? X + 2 * s0 : nullptr, soff[(size_t)i + 1] - s0, n_starts,
                                              min_gain, max_sweeps, tours ? tours + s0 : nullptr, n_total, costs ? costs + i * n_starts : nullptr,
                                              route ? route + s0 : nullptr);
        if (cost) cost[i] = f.cost;
        if (winner) winner[i] = f.winner;
        if (sweeps) sweeps[i] = f.sweeps;
        if (status) status[i] = f.status;
        if (stored) stored[i] = f.stored;
    });
    return FCPP_OK;
}

// ---- connector clearance (fcpp_clear.hip; the rule: fcpp_clearfn.h) -------------------------------------------------------------------
int fcpp_conn_clear(fcpp_ctx *c, int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, double radius,
                    const int32_t *word, const double *seg, const int64_t *pair_field, int64_t n_fields, const int64_t *ring_offsets,
                    int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y, int32_t *crossings,
                    int8_t *inside, double *first_s, int32_t *field_status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = clear_conn_args(mode, n, from_x, from_y, from_h, radius, word, seg, pair_field, n_fields, ring_offsets, n_rings, vert_offsets, n_verts, x, y);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> rings, verts;
    rc = swath_fields(c, n_fields, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    LAUNCHCHK(launch_clear_field_status(c->stream, F, field_status));
    LAUNCHCHK(launch_clear_conn(c->stream, mode, n, from_x, from_y, from_h, radius, word, seg, pair_field, F, crossings, inside, first_s));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_route_transit_clear(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                             const double *ax, const double *ay, const double *bx, const double *by, const double *angle, double radius, int mode,
                             const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, const int64_t *ring_offsets,
                             int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y, double penalty,
                             double *T, uint8_t *B)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!swath_offsets || !t_offsets || !ring_offsets || !vert_offsets || (n_total > 0 && (!ax || !ay || !bx || !by)) || (n > 0 && !angle) ||
        (t_total > 0 && (!T || !B)) || (n_verts > 0 && (!x || !y)))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc == FCPP_OK) rc = clear_penalty(penalty);
    if (rc == FCPP_OK && (n_rings < 0 || n_verts < 0)) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff, rings, verts, tile_off;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = clear_tiles(n, toff, tile_off);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    if (rc) return rc;
    DevBuf<int64_t> tiles;
    HIPCHK(tiles.alloc((size_t)n + 1));
    HIPCHK(hipMemcpyAsync(tiles.p, tile_off.data(), tile_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    const ClearFields F = { n, ring_offsets, vert_offsets, x, y };
    LAUNCHCHK(launch_clear_transit(c->stream, n, swath_offsets, ax, ay, bx, by, angle, radius, mode, t_offsets, tiles.p, tile_off[(size_t)n], F, penalty,
                                   T, B));
    HIPCHK(hipStreamSynchronize(c->stream));      // (the tile offsets die here)
    return FCPP_OK;
}

int fcpp_debug_conn_clear(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, double radius, const int32_t *word,
                          const double *seg, const int64_t *pair_field, int64_t n_fields, const int64_t *ring_offsets, int64_t n_rings,
                          const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y, int32_t *crossings, int8_t *inside,
                          double *first_s, int32_t *field_status)
{
    int rc = clear_conn_args(mode, n, from_x, from_y, from_h, radius, word, seg, pair_field, n_fields, ring_offsets, n_rings, vert_offsets, n_verts, x, y);
    if (rc) return rc;
    std::vector<int64_t> rings, verts;
    rc = swath_fields(nullptr, n_fields, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc) return rc;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    if (field_status) WorkerPool::parallel_for(n_fields, [&](int64_t f) { field_status[f] = clear_field_status(F, f); });
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const ClearResult r = mode == 0 ? clear_path<0>(F, pair_field[i], from_x[i], from_y[i], from_h[i], radius, word[i], seg + 3 * i)
                                        : clear_path<1>(F, pair_field[i], from_x[i], from_y[i], from_h[i], radius, word[i], seg + 5 * i);
        if (crossings) crossings[i] = r.crossings;
        if (inside) inside[i] = r.inside;
        if (first_s) first_s[i] = r.first_s;
    });
    return FCPP_OK;
}

int fcpp_debug_route_transit_clear(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                   const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total,
                                   const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                   const double *y, double penalty, double *T, uint8_t *B)
{
    if (!swath_offsets || !t_offsets || !ring_offsets || !vert_offsets || (n_total > 0 && (!ax || !ay || !bx || !by)) || (n > 0 && !angle) ||
        (t_total > 0 && (!T || !B)) || (n_verts > 0 && (!x || !y)))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc == FCPP_OK) rc = clear_penalty(penalty);
    if (rc == FCPP_OK && (n_rings < 0 || n_verts < 0)) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> soff, toff, rings, verts;
    rc = route_offsets(nullptr, n, nullptr, swath_offsets, n_total, nullptr, t_offsets, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, n, nullptr, angle);
    if (rc) return rc;
    const ClearFields F = { n, ring_offsets, vert_offsets, x, y };
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const int64_t s0 = soff[(size_t)i];
        const int N = (int)(toff[(size_t)i + 1] == toff[(size_t)i] ? 0 : 2 * (soff[(size_t)i + 1] - s0));
        double *Tb = T + toff[(size_t)i];
        uint8_t *Bb = B + toff[(size_t)i];
        for (int p = 0; p < N; ++p)
            for (int q = 0; q < N; ++q) {
                if (!route_canonical(p, q, N)) continue;
                const int e = p * N + q, e2 = (q ^ 1) * N + (p ^ 1);
                bool blocked = false;
                if ((p >> 1) != (q >> 1))
                    blocked = mode == 0 ? clear_transit_blocked<0>(F, i, ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, p, q)
                                        : clear_transit_blocked<1>(F, i, ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, p, q);
                Bb[e] = Bb[e2] = blocked ? 1 : 0;
                if (blocked) { const double v = Tb[e] + penalty; Tb[e] = v; Tb[e2] = v; }
            }
    });
    return FCPP_OK;
}

// ---- clear connectors (fcpp_solveclear.hip; the rule: fcpp_solveclearfn.h) -------------------------------------------------------------
int fcpp_conn_solve_clear(fcpp_ctx *c, int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                          const double *to_y, const double *to_h, double radius, const int64_t *pair_field, int64_t n_fields,
                          const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y,
                          int32_t *word, double *seg, double *len, int32_t *rank, int32_t *crossings, int32_t *field_status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = solve_clear_args(mode, n, from_x, from_y, from_h, to_x, to_y, to_h, radius, pair_field, n_fields, ring_offsets, n_rings, vert_offsets,
                              n_verts, x, y);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> rings, verts;
    rc = swath_fields(c, n_fields, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    const SolveClearIo io = { from_x, from_y, from_h, to_x, to_y, to_h, pair_field, word, seg, len, rank, crossings };
    LAUNCHCHK(launch_clear_field_status(c->stream, F, field_status));
    c->solve_clear_listed = 0;
    if (n > 0 && (word || seg || len || rank || crossings)) {
        DevBuf<int64_t> list;
        DevBuf<unsigned long long> count;
        HIPCHK(list.alloc((size_t)n));
        HIPCHK(count.alloc(1));
        HIPCHK(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), c->stream));
        LAUNCHCHK(launch_solve_clear_pairs(c->stream, mode, n, io, radius, F, list.p, count.p));
        unsigned long long listed = 0;
        HIPCHK(hipMemcpyAsync(&listed, count.p, sizeof listed, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (listed > (unsigned long long)n) return fail(FCPP_EHIP, "the first pass listed more pairs than there are");
        c->solve_clear_listed = (int64_t)listed;
        if (listed > 0) {
            LAUNCHCHK(launch_solve_clear_words(c->stream, mode, (int64_t)listed, list.p, io, radius, F));
            ++c->solve_clear_word_launches;
        }
        HIPCHK(hipStreamSynchronize(c->stream));          // (the list dies here)
        return FCPP_OK;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_ctx_solve_clear_passes(const fcpp_ctx *c, int64_t *listed, int64_t *word_launches)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (listed) *listed = c->solve_clear_listed;
    if (word_launches) *word_launches = c->solve_clear_word_launches;
    return FCPP_OK;
}

int fcpp_debug_conn_words(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                          const double *to_y, const double *to_h, double radius, uint8_t *ok, double *seg, double *total)
{
    if (n > 0 && (!from_x || !from_y || !from_h || !to_x || !to_y || !to_h)) return fail(FCPP_EINVAL, "bad arguments");
    const int rc = route_radius(radius, mode);
    if (rc) return rc;
    if (n < 0) return fail(FCPP_ESIZE, "bad sizes");
    if (mode == 0) debug_conn_words<0>(n, from_x, from_y, from_h, to_x, to_y, to_h, radius, ok, seg, total);
    else debug_conn_words<1>(n, from_x, from_y, from_h, to_x, to_y, to_h, radius, ok, seg, total);
    return FCPP_OK;
}

int fcpp_debug_conn_solve_clear(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                                const double *to_y, const double *to_h, double radius, const int64_t *pair_field, int64_t n_fields,
                                const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                const double *y, int32_t *word, double *seg, double *len, int32_t *rank, int32_t *crossings, int32_t *field_status)
{
    int rc = solve_clear_args(mode, n, from_x, from_y, from_h, to_x, to_y, to_h, radius, pair_field, n_fields, ring_offsets, n_rings, vert_offsets,
                              n_verts, x, y);
    if (rc) return rc;
    std::vector<int64_t> rings, verts;
    rc = swath_fields(nullptr, n_fields, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc) return rc;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    if (field_status) WorkerPool::parallel_for(n_fields, [&](int64_t f) { field_status[f] = clear_field_status(F, f); });
    const int nseg = mode == 0 ? 3 : 5;
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const SolveClearResult r = mode == 0 ? solve_clear<0>(F, pair_field[i], from_x[i], from_y[i], from_h[i], to_x[i], to_y[i], to_h[i], radius)
                                             : solve_clear<1>(F, pair_field[i], from_x[i], from_y[i], from_h[i], to_x[i], to_y[i], to_h[i], radius);
        if (word) word[i] = r.word;
        if (seg)
            for (int k = 0; k < nseg; ++k) seg[i * nseg + k] = r.seg[k];
        if (len) len[i] = r.len;
        if (rank) rank[i] = r.rank;
        if (crossings) crossings[i] = r.crossings;
    });
    return FCPP_OK;
}

// ---- the priced transit block (fcpp_clear.hip, fcpp_solveclear.hip; the rule: priced_transit of fcpp_solveclearfn.h) ---------------------
// what fcpp_route_transit_priced and its host twin check alike before the offsets
static int route_priced_args(const void *swath_offsets, const void *t_offsets, const void *ring_offsets, const void *vert_offsets, int64_t n,
                             int64_t n_total, const double *ax, const double *ay, const double *bx, const double *by, const double *angle, double radius,
                             int mode, int64_t t_total, int64_t n_rings, int64_t n_verts, const double *x, const double *y, double penalty, const double *T)
{
    if (!swath_offsets || !t_offsets || !ring_offsets || !vert_offsets || (n_total > 0 && (!ax || !ay || !bx || !by)) || (n > 0 && !angle) ||
        (t_total > 0 && !T) || (n_verts > 0 && (!x || !y)))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc == FCPP_OK) rc = clear_penalty(penalty);
    if (rc == FCPP_OK && (n_rings < 0 || n_verts < 0)) rc = fail(FCPP_ESIZE, "bad sizes");
    return rc;
}

int fcpp_route_transit_priced(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                              const double *ax, const double *ay, const double *bx, const double *by, const double *angle, double radius, int mode,
                              const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, const int64_t *ring_offsets,
                              int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y, double penalty,
                              double *T, int8_t *K)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = route_priced_args(swath_offsets, t_offsets, ring_offsets, vert_offsets, n, n_total, ax, ay, bx, by, angle, radius, mode, t_total, n_rings,
                               n_verts, x, y, penalty, T);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff, rings, verts, tile_off;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = clear_tiles(n, toff, tile_off);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    // (the second pass's grid: at most a workgroup per 4 listed entries, t_total / 2 of them)
    if (rc == FCPP_OK && t_total / 8 >= CLEAR_MAX_GROUPS) rc = fail(FCPP_ESIZE, "2^34 transit entries or more");
    if (rc) return rc;
    c->route_priced_listed = 0;
    if (n <= 0 || t_total <= 0) return FCPP_OK;
    DevBuf<int64_t> tiles, list;
    DevBuf<unsigned long long> count;
    const int64_t room = t_total / 2;                     // the canonical pairs of different swaths: half of a block less its 2 N own-swath entries
    HIPCHK(tiles.alloc((size_t)n + 1));
    HIPCHK(list.alloc((size_t)(room > 0 ? room : 1)));
    HIPCHK(count.alloc(1));
    HIPCHK(hipMemcpyAsync(tiles.p, tile_off.data(), tile_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), c->stream));
    const ClearFields F = { n, ring_offsets, vert_offsets, x, y };
    LAUNCHCHK(launch_route_priced_first(c->stream, n, swath_offsets, ax, ay, bx, by, angle, radius, mode, t_offsets, tiles.p, tile_off[(size_t)n], F,
                                        penalty, T, K, list.p, count.p));
    unsigned long long listed = 0;
    HIPCHK(hipMemcpyAsync(&listed, count.p, sizeof listed, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (listed > (unsigned long long)room) return fail(FCPP_EHIP, "the first pass listed more entries than there are canonical pairs");
    c->route_priced_listed = (int64_t)listed;
    if (listed > 0) {
        LAUNCHCHK(launch_route_priced_words(c->stream, mode, (int64_t)listed, list.p, n, swath_offsets, ax, ay, bx, by, angle, radius, t_offsets, t_total,
                                            F, T, K));
        ++c->route_priced_word_launches;
    }
    HIPCHK(hipStreamSynchronize(c->stream));              // (the tile offsets and the list die here)
    return FCPP_OK;
}

int fcpp_ctx_route_priced_passes(const fcpp_ctx *c, int64_t *listed, int64_t *word_launches)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (listed) *listed = c->route_priced_listed;
    if (word_launches) *word_launches = c->route_priced_word_launches;
    return FCPP_OK;
}

int fcpp_debug_route_transit_priced(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                    const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total,
                                    const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                    const double *y, double penalty, double *T, int8_t *K)
{
    int rc = route_priced_args(swath_offsets, t_offsets, ring_offsets, vert_offsets, n, n_total, ax, ay, bx, by, angle, radius, mode, t_total, n_rings,
                               n_verts, x, y, penalty, T);
    if (rc) return rc;
    std::vector<int64_t> soff, toff, rings, verts;
    rc = route_offsets(nullptr, n, nullptr, swath_offsets, n_total, nullptr, t_offsets, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, n, nullptr, angle);
    if (rc) return rc;
    const ClearFields F = { n, ring_offsets, vert_offsets, x, y };
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const int64_t s0 = soff[(size_t)i];
        const int N = (int)(toff[(size_t)i + 1] == toff[(size_t)i] ? 0 : 2 * (soff[(size_t)i + 1] - s0));
        double *Tb = T + toff[(size_t)i];
        int8_t *Kb = K ? K + toff[(size_t)i] : nullptr;
        for (int p = 0; p < N; ++p)
            for (int q = 0; q < N; ++q) {
                if (!route_canonical(p, q, N)) continue;
                const int e = p * N + q, e2 = (q ^ 1) * N + (p ^ 1);
                PricedTransit r = { INFINITY, 0, false };
                if ((p >> 1) != (q >> 1))
                    r = mode == 0 ? priced_transit<0>(F, i, ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, penalty, p, q)
                                  : priced_transit<1>(F, i, ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, penalty, p, q);
                Tb[e] = Tb[e2] = r.t;
                if (Kb) Kb[e] = Kb[e2] = (int8_t)r.rank;
            }
    });
    return FCPP_OK;
}

// ---- field paths and headland paths (fcpp_legs.hip; the rules: fcpp_fpathfn.h, fcpp_hpathfn.h): argument checks, then the leg paths' skeleton ----
int fcpp_field_path_counts(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                           const double *ax, const double *ay, const double *bx, const double *by, const double *length, const double *angle,
                           const int32_t *order, double radius, int mode, double spacing, const double *entry_x, const double *entry_y,
                           const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h, int64_t *path_offsets,
                           int64_t *path_offsets_host, int64_t *leg_offsets, double *work_length, double *transit_length, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!path_offsets || !leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff;
    rc = fpath_offsets(c, n, swath_offsets, swath_offsets_host, n_total, angle, nullptr, soff);
    if (rc) return rc;
    const FpathIn in = { swath_offsets, ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    return legs_counts<FieldLegs>(c, n, n > 0 ? 2 * n_total + n : 0, n_total, in, mode, "a leg or a field has 2^31 samples or more", path_offsets,
                                  path_offsets_host, leg_offsets, { { work_length, transit_length, nullptr } }, status);
}

int fcpp_field_path_fill(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                         const double *ax, const double *ay, const double *bx, const double *by, const double *length, const double *angle,
                         const int32_t *order, double radius, int mode, double spacing, const double *entry_x, const double *entry_y,
                         const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h, const int64_t *leg_offsets,
                         int64_t total_samples, double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK && (total_samples < 0 || total_samples > ((int64_t)1 << 38))) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff;
    rc = fpath_offsets(c, n, swath_offsets, swath_offsets_host, n_total, angle, nullptr, soff);
    if (rc) return rc;
    const FpathIn in = { swath_offsets, ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    return legs_fill<FieldLegs>(c, n, n > 0 ? 2 * n_total + n : 0, in, mode, leg_offsets, total_samples, x, y, heading, kappa, part, gear, leg);
}

int fcpp_debug_field_paths(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                           const double *by, const double *length, const double *angle, const int32_t *order, double radius, int mode,
                           double spacing, const double *entry_x, const double *entry_y, const double *entry_h, const double *exit_x,
                           const double *exit_y, const double *exit_h, int64_t *path_offsets, int64_t *leg_offsets, double *work_length,
                           double *transit_length, int32_t *status, int32_t *leg_word, double *leg_seg, double *leg_total, int64_t cap,
                           double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> soff;
    rc = fpath_offsets(nullptr, n, nullptr, swath_offsets, n_total, nullptr, angle, soff);
    if (rc) return rc;
    const FpathIn in = { soff.data(), ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    std::vector<int32_t> seen;
    try { seen.assign((size_t)n_total, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    return legs_host<FieldLegs>(n, n > 0 ? 2 * n_total + n : 0, in, "a leg or a field has 2^31 samples or more",
                                [&](int64_t i, FpathLeg *legs, int64_t *cnt, double *t, bool &oversize) {
                                    int32_t *sn = seen.data() + soff[(size_t)i];
                                    return mode == 0 ? fpath_field_host<0>(in, i, legs, cnt, sn, t[0], t[1], oversize)
                                                     : fpath_field_host<1>(in, i, legs, cnt, sn, t[0], t[1], oversize);
                                },
                                path_offsets, leg_offsets, { { work_length, transit_length, nullptr } }, status, nullptr, leg_word, leg_seg, leg_total, cap,
                                x, y, heading, kappa, part, gear, leg);
}

// ---- the clear field paths: the entries above with the region CSR and the stage between the records and the scan ----------------------------
int fcpp_field_path_counts_clear(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                                 const double *ax, const double *ay, const double *bx, const double *by, const double *length, const double *angle,
                                 const int32_t *order, double radius, int mode, double spacing, const double *entry_x, const double *entry_y,
                                 const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h,
                                 const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                 const double *y, int64_t *path_offsets, int64_t *path_offsets_host, int64_t *leg_offsets, double *work_length,
                                 double *transit_length, int32_t *status, int32_t *leg_rank, int32_t *leg_crossings, int32_t *leg_word,
                                 double *leg_seg, double *leg_total, int32_t *blocked, int32_t *reshaped, int32_t *region_status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!path_offsets || !leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK) rc = fpath_region_args(n, ring_offsets, n_rings, vert_offsets, n_verts, x, y);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, rings, verts;
    rc = fpath_offsets(c, n, swath_offsets, swath_offsets_host, n_total, angle, nullptr, soff);
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const FpathIn in = { swath_offsets, ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    FpathClearStage stage = { c, mode, n, n_total, in, { n, ring_offsets, vert_offsets, x, y } };
    stage.rank = leg_rank; stage.crossings = leg_crossings; stage.leg_word = leg_word; stage.leg_seg = leg_seg; stage.leg_total = leg_total;
    stage.blocked = blocked; stage.reshaped = reshaped; stage.region_status = region_status;
    return legs_counts<FieldLegs>(c, n, n > 0 ? 2 * n_total + n : 0, n_total, in, mode, "a leg or a field has 2^31 samples or more", path_offsets,
                                  path_offsets_host, leg_offsets, { { work_length, transit_length, nullptr } }, status, stage);
}

int fcpp_field_path_fill_clear(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                               const double *ax, const double *ay, const double *bx, const double *by, const double *length, const double *angle,
                               const int32_t *order, double radius, int mode, double spacing, const double *entry_x, const double *entry_y,
                               const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h,
                               const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *rx,
                               const double *ry, const int64_t *leg_offsets, int64_t total_samples, double *x, double *y, double *heading,
                               double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK) rc = fpath_region_args(n, ring_offsets, n_rings, vert_offsets, n_verts, rx, ry);
    if (rc == FCPP_OK && (total_samples < 0 || total_samples > ((int64_t)1 << 38))) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, rings, verts;
    rc = fpath_offsets(c, n, swath_offsets, swath_offsets_host, n_total, angle, nullptr, soff);
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const FpathIn in = { swath_offsets, ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    FpathClearStage stage = { c, mode, n, n_total, in, { n, ring_offsets, vert_offsets, rx, ry } };
    return legs_fill<FieldLegs>(c, n, n > 0 ? 2 * n_total + n : 0, in, mode, leg_offsets, total_samples, x, y, heading, kappa, part, gear, leg, stage);
}

int fcpp_ctx_field_path_clear_passes(const fcpp_ctx *c, int64_t *listed, int64_t *word_launches)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (listed) *listed = c->fpath_clear_listed;
    if (word_launches) *word_launches = c->fpath_clear_word_launches;
    return FCPP_OK;
}

int fcpp_debug_field_paths_clear(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                 const double *by, const double *length, const double *angle, const int32_t *order, double radius, int mode,
                                 double spacing, const double *entry_x, const double *entry_y, const double *entry_h, const double *exit_x,
                                 const double *exit_y, const double *exit_h, const int64_t *ring_offsets, int64_t n_rings,
                                 const int64_t *vert_offsets, int64_t n_verts, const double *rx, const double *ry, int64_t *path_offsets,
                                 int64_t *leg_offsets, double *work_length, double *transit_length, int32_t *status, int32_t *leg_rank,
                                 int32_t *leg_crossings, int32_t *leg_word, double *leg_seg, double *leg_total, int32_t *blocked,
                                 int32_t *reshaped, int32_t *region_status, int64_t cap, double *x, double *y, double *heading, double *kappa,
                                 int8_t *part, int8_t *gear, int32_t *leg)
{
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK) rc = fpath_region_args(n, ring_offsets, n_rings, vert_offsets, n_verts, rx, ry);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> soff, rings, verts;
    rc = fpath_offsets(nullptr, n, nullptr, swath_offsets, n_total, nullptr, angle, soff);
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc) return rc;
    const FpathIn in = { soff.data(), ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    const ClearFields F = { n, ring_offsets, vert_offsets, rx, ry };
    const int64_t n_slots = n > 0 ? 2 * n_total + n : 0;
    std::vector<int32_t> seen, rank, cross;
    try {
        seen.assign((size_t)n_total, 0); rank.assign((size_t)n_slots, 0); cross.assign((size_t)n_slots, 0);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (region_status) WorkerPool::parallel_for(n, [&](int64_t f) { region_status[f] = clear_field_status(F, f); });
    rc = legs_host<FieldLegs>(n, n_slots, in, "a leg or a field has 2^31 samples or more",
                              [&](int64_t i, FpathLeg *legs, int64_t *cnt, double *t, bool &oversize) {
                                  int32_t *sn = seen.data() + soff[(size_t)i];
                                  int32_t *rk = rank.data() + fpath_first_slot(soff.data(), i), *cr = cross.data() + fpath_first_slot(soff.data(), i);
                                  int32_t b, r;
                                  const int st = mode == 0 ? fpath_field_clear_host<0>(in, F, i, legs, cnt, sn, rk, cr, b, r, t[0], t[1], oversize)
                                                           : fpath_field_clear_host<1>(in, F, i, legs, cnt, sn, rk, cr, b, r, t[0], t[1], oversize);
                                  if (blocked) blocked[i] = b;
                                  if (reshaped) reshaped[i] = r;
                                  return st;
                              },
                              path_offsets, leg_offsets, { { work_length, transit_length, nullptr } }, status, nullptr, leg_word, leg_seg, leg_total, cap,
                              x, y, heading, kappa, part, gear, leg);
    if (rc) return rc;
    if (leg_rank && n_slots > 0) memcpy(leg_rank, rank.data(), rank.size() * sizeof(int32_t));
    if (leg_crossings && n_slots > 0) memcpy(leg_crossings, cross.data(), cross.size() * sizeof(int32_t));
    return FCPP_OK;
}

int fcpp_headland_path_counts(fcpp_ctx *c, int64_t n_rings, const int64_t *ring_offsets, const int64_t *ring_offsets_host, int64_t n_verts,
                              const double *x, const double *y, const int32_t *src, const double *ring_dist, double radius, int mode,
                              double spacing, int direction, double smooth_tol, int64_t *path_offsets, int64_t *path_offsets_host,
                              int64_t *leg_offsets, double *work_length, double *transit_length, double *skipped_length, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!path_offsets || !leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = hpath_args(n_rings, ring_offsets, n_verts, x, y, src, ring_dist, radius, mode, spacing, direction, smooth_tol);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> roff;
    rc = host_offsets(c, n_rings, ring_offsets, ring_offsets_host, n_verts, "ring_offsets", roff);
    if (rc) return rc;
    const HpathIn in = { ring_offsets, x, y, src, ring_dist, radius, spacing, smooth_tol, direction };
    return legs_counts<RingLegs>(c, n_rings, n_rings > 0 ? 2 * n_verts : 0, n_rings, in, mode, "a leg or a ring has 2^31 samples or more", path_offsets,
                                 path_offsets_host, leg_offsets, { { work_length, transit_length, skipped_length } }, status);
}

int fcpp_headland_path_fill(fcpp_ctx *c, int64_t n_rings, const int64_t *ring_offsets, const int64_t *ring_offsets_host, int64_t n_verts,
                            const double *x, const double *y, const int32_t *src, const double *ring_dist, double radius, int mode, double spacing,
                            int direction, double smooth_tol, const int64_t *leg_offsets, int64_t total_samples, double *out_x, double *out_y,
                            double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = hpath_args(n_rings, ring_offsets, n_verts, x, y, src, ring_dist, radius, mode, spacing, direction, smooth_tol);
    if (rc == FCPP_OK && (total_samples < 0 || total_samples > ((int64_t)1 << 38))) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> roff;
    rc = host_offsets(c, n_rings, ring_offsets, ring_offsets_host, n_verts, "ring_offsets", roff);
    if (rc) return rc;
    const HpathIn in = { ring_offsets, x, y, src, ring_dist, radius, spacing, smooth_tol, direction };
    return legs_fill<RingLegs>(c, n_rings, n_rings > 0 ? 2 * n_verts : 0, in, mode, leg_offsets, total_samples, out_x, out_y, heading, kappa, part, gear,
                               leg);
}

int fcpp_debug_headland_paths(int64_t n_rings, const int64_t *ring_offsets, int64_t n_verts, const double *x, const double *y, const int32_t *src,
                              const double *ring_dist, double radius, int mode, double spacing, int direction, double smooth_tol,
                              int64_t *path_offsets, int64_t *leg_offsets, double *work_length, double *transit_length, double *skipped_length,
                              int32_t *status, int32_t *leg_kind, int32_t *leg_word, double *leg_seg, double *leg_total, int64_t cap, double *out_x,
                              double *out_y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    int rc = hpath_args(n_rings, ring_offsets, n_verts, x, y, src, ring_dist, radius, mode, spacing, direction, smooth_tol);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> roff;
    rc = host_offsets(nullptr, n_rings, nullptr, ring_offsets, n_verts, "ring_offsets", roff);
    if (rc) return rc;
    const HpathIn in = { roff.data(), x, y, src, ring_dist, radius, spacing, smooth_tol, direction };
    return legs_host<RingLegs>(n_rings, n_rings > 0 ? 2 * n_verts : 0, in, "a leg or a ring has 2^31 samples or more",
                               [&](int64_t r, HpathLeg *legs, int64_t *cnt, double *t, bool &oversize) {
                                   return mode == 0 ? hpath_ring_host<0>(in, r, legs, cnt, t[0], t[1], t[2], oversize)
                                                    : hpath_ring_host<1>(in, r, legs, cnt, t[0], t[1], t[2], oversize);
                               },
                               path_offsets, leg_offsets, { { work_length, transit_length, skipped_length } }, status, leg_kind, leg_word, leg_seg, leg_total,
                               cap, out_x, out_y, heading, kappa, part, gear, leg);
}

}  // extern "C"

// ---- loop transits (fcpp_transit.hip; the rule: fcpp_transitfn.h) -------------------------------------------------------------------------
namespace {
// what the loop-transit entries and the host twin check alike of their loop set, before the offsets
int transit_loop_args(int64_t n_loops, const void *loop_offsets, int64_t n_samples, bool arrays)
{
    if (!loop_offsets || (n_samples > 0 && !arrays)) return fail(FCPP_EINVAL, "bad arguments");
    if (n_loops < 0 || n_samples < 0 || n_loops > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

int transit_solve_args(int mode, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty, const double *th,
                       double radius, const int64_t *pair_field, int64_t n_fields, const void *ring_offsets, int64_t n_rings, const void *vert_offsets,
                       int64_t n_verts, const double *x, const double *y, int64_t n_loops, const void *loop_offsets, int64_t n_samples, bool arrays,
                       const void *field_loops, int64_t stride)
{
    int rc = solve_clear_args(mode, n, fx, fy, fh, tx, ty, th, radius, pair_field, n_fields, ring_offsets, n_rings, vert_offsets, n_verts, x, y);
    if (rc == FCPP_OK) rc = transit_loop_args(n_loops, loop_offsets, n_samples, arrays);
    if (rc) return rc;
    if (!field_loops) return fail(FCPP_EINVAL, "bad arguments");
    if (stride < 1) return fail(FCPP_EINVAL, "stride must be at least 1");
    return FCPP_OK;
}

int transit_spacing(double radius, int mode, double spacing)
{
    const int rc = route_radius(radius, mode);
    if (rc) return rc;
    if (!(spacing > 0.0) || !isfinite(spacing)) return fail(FCPP_EINVAL, "spacing must be positive and finite");
    return FCPP_OK;
}

bool transit_rec_args(int64_t n, const TransitRec &rec)
{
    return n <= 0 || (rec.found && rec.loop && rec.i && rec.j && rec.in_word && rec.in_seg && rec.out_word && rec.out_seg);
}
}  // namespace

extern "C" {

int fcpp_loop_transit_solve(fcpp_ctx *c, int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                            const double *to_y, const double *to_h, double radius, const int64_t *pair_field, int64_t n_fields,
                            const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y,
                            int64_t n_loops, const int64_t *loop_offsets, const int64_t *loop_offsets_host, int64_t n_samples, const double *loop_x,
                            const double *loop_y, const double *loop_h, const double *loop_s, const int8_t *loop_part, const int8_t *loop_gear,
                            const int64_t *field_loops, const int64_t *field_loops_host, int64_t stride, int32_t *found, int64_t *loop, int64_t *st_i,
                            int64_t *st_j, int32_t *in_word, double *in_seg, double *in_len, int32_t *in_rank, int32_t *out_word, double *out_seg,
                            double *out_len, int32_t *out_rank, double *ride, double *total, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = transit_solve_args(mode, n, from_x, from_y, from_h, to_x, to_y, to_h, radius, pair_field, n_fields, ring_offsets, n_rings, vert_offsets,
                                n_verts, x, y, n_loops, loop_offsets ? (const void *)loop_offsets : (const void *)loop_offsets_host, n_samples,
                                loop_x && loop_y && loop_h && loop_s && loop_part && loop_gear,
                                field_loops ? (const void *)field_loops : (const void *)field_loops_host, stride);
    if (rc) return rc;
    if (!loop_offsets || !field_loops) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<int64_t> rings, verts, loff, floops;
    rc = swath_fields(c, n_fields, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = host_offsets(c, n_loops, loop_offsets, loop_offsets_host, n_samples, "loop_offsets", loff);
    if (rc == FCPP_OK) rc = host_offsets(c, n_fields, field_loops, field_loops_host, n_loops, "field_loops", floops);
    if (rc) return rc;
    c->transit_listed = 0;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    const TransitLoops L = { n_fields, n_loops, field_loops, loop_offsets, loop_x, loop_y, loop_h, nullptr, loop_s, loop_part, loop_gear, stride };
    const TransitIo io = { from_x, from_y, from_h, to_x, to_y, to_h, pair_field, found, loop, st_i, st_j, in_word, in_seg, in_len, in_rank,
                           out_word, out_seg, out_len, out_rank, ride, total, status };
    if (n <= 0) return FCPP_OK;
    DevBuf<int64_t> st_idx, st_loop, n_st, pick_l, pick_i, pick_j, list;
    DevBuf<int32_t> loops_ok, region_status;
    DevBuf<double> val;
    DevBuf<unsigned long long> count;
    HIPCHK(st_idx.alloc((size_t)n_samples));
    HIPCHK(st_loop.alloc((size_t)n_samples));
    HIPCHK(n_st.alloc((size_t)n_fields));
    HIPCHK(loops_ok.alloc((size_t)n_fields));
    HIPCHK(region_status.alloc((size_t)n_fields));
    HIPCHK(pick_l.alloc((size_t)n));
    HIPCHK(pick_i.alloc((size_t)n));
    HIPCHK(pick_j.alloc((size_t)n));
    HIPCHK(count.alloc(1));
    TransitTemp T = { st_idx.p, st_loop.p, n_st.p, loops_ok.p, region_status.p, nullptr, pick_l.p, pick_i.p, pick_j.p };
    LAUNCHCHK(launch_clear_field_status(st, F, region_status.p));
    LAUNCHCHK(launch_transit_stations(st, L, T));
    // the station counts come back: the stations pass's grid is sized by the largest a pair can use
    std::vector<int64_t> nst;
    try { nst.assign((size_t)n_fields, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (n_fields > 0) HIPCHK(hipMemcpyAsync(nst.data(), n_st.p, (size_t)n_fields * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t most = 0;
    for (int64_t f = 0; f < n_fields; ++f) most = std::max(most, std::min<int64_t>(nst[(size_t)f], TRANSIT_MAX_STATIONS));
    const int64_t per = (most + TRANSIT_BLOCK - 1) / TRANSIT_BLOCK * TRANSIT_BLOCK;
    if (per > 0 && n > (((int64_t)1 << 36) / (2 * per))) return fail(FCPP_ESIZE, "2^36 (pair, side, station) items or more");
    const int64_t items = n * 2 * per;
    if (items > 0) {
        HIPCHK(val.alloc((size_t)items));
        HIPCHK(list.alloc((size_t)items));
        T.val = val.p;
        HIPCHK(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), st));
        LAUNCHCHK(launch_transit_sides(st, mode, n, per, io, radius, F, L, T, list.p, count.p));
        unsigned long long listed = 0;
        HIPCHK(hipMemcpyAsync(&listed, count.p, sizeof listed, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (listed > (unsigned long long)items) return fail(FCPP_EHIP, "the first pass listed more items than there are");
        c->transit_listed = (int64_t)listed;
        if (listed > 0) {
            LAUNCHCHK(launch_transit_words(st, mode, (int64_t)listed, list.p, n, per, io, radius, F, L, T));
            ++c->transit_word_launches;
        }
    }
    LAUNCHCHK(launch_transit_pick(st, n, per, io, L, T));
    LAUNCHCHK(launch_transit_finish(st, mode, n, io, radius, F, L, T));
    HIPCHK(hipStreamSynchronize(st));          // (the temporaries die here)
    return FCPP_OK;
}

int fcpp_ctx_loop_transit_passes(const fcpp_ctx *c, int64_t *listed, int64_t *word_launches)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (listed) *listed = c->transit_listed;
    if (word_launches) *word_launches = c->transit_word_launches;
    return FCPP_OK;
}

int fcpp_loop_transit_counts(fcpp_ctx *c, int mode, int64_t n, const int32_t *found, const int64_t *loop, const int64_t *st_i, const int64_t *st_j,
                             const int32_t *in_word, const double *in_seg, const int32_t *out_word, const double *out_seg, int64_t n_loops,
                             const int64_t *loop_offsets, const int64_t *loop_offsets_host, int64_t n_samples, double spacing,
                             int64_t *path_offsets, int64_t *path_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    const TransitRec rec = { found, loop, st_i, st_j, in_word, in_seg, out_word, out_seg };
    int rc = transit_spacing(1.0, mode, spacing);
    if (rc == FCPP_OK) rc = transit_loop_args(n_loops, loop_offsets, n_samples, true);
    if (rc) return rc;
    if (!transit_rec_args(n, rec) || !path_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (n < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> loff;
    rc = host_offsets(c, n_loops, loop_offsets, loop_offsets_host, n_samples, "loop_offsets", loff);
    if (rc) return rc;
    return sample_counts(c, n, path_offsets, path_offsets_host, "a transit has 2^31 samples or more", [&](hipStream_t st, int64_t *err) {
        return launch_transit_counts(st, mode, n, rec, n_loops, loop_offsets, spacing, path_offsets, err);
    });
}

int fcpp_loop_transit_fill(fcpp_ctx *c, int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, double radius,
                           const int32_t *found, const int64_t *loop, const int64_t *st_i, const int64_t *st_j, const int32_t *in_word,
                           const double *in_seg, const int32_t *out_word, const double *out_seg, int64_t n_loops, const int64_t *loop_offsets,
                           const int64_t *loop_offsets_host, int64_t n_samples, const double *loop_x, const double *loop_y, const double *loop_h,
                           const double *loop_kappa, const int8_t *loop_gear, double spacing, const int64_t *path_offsets,
                           const int64_t *path_offsets_host, int64_t total_samples, double *out_x, double *out_y, double *heading, double *kappa,
                           int8_t *part, int8_t *gear)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    const TransitRec rec = { found, loop, st_i, st_j, in_word, in_seg, out_word, out_seg };
    int rc = transit_spacing(radius, mode, spacing);
    if (rc == FCPP_OK) rc = transit_loop_args(n_loops, loop_offsets, n_samples, loop_x && loop_y && loop_h && loop_kappa && loop_gear);
    if (rc) return rc;
    if (!transit_rec_args(n, rec) || !path_offsets || (n > 0 && (!from_x || !from_y || !from_h))) return fail(FCPP_EINVAL, "bad arguments");
    if (n < 0 || n > INT32_MAX || total_samples < 0 || total_samples > ((int64_t)1 << 38)) return fail(FCPP_ESIZE, "bad sizes");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> loff;
    rc = host_offsets(c, n_loops, loop_offsets, loop_offsets_host, n_samples, "loop_offsets", loff);
    if (rc) return rc;
    SampleOffsets outs;
    rc = outs.get(c, n, path_offsets, path_offsets_host, total_samples, "path_offsets", true);
    if (rc) return rc;
    const TransitLoops L = { 0, n_loops, nullptr, loop_offsets, loop_x, loop_y, loop_h, loop_kappa, nullptr, nullptr, loop_gear, 1 };
    LAUNCHCHK(launch_transit_fill(c->stream, mode, n, rec, L, from_x, from_y, from_h, radius, spacing, outs.dev, total_samples, out_x, out_y, heading,
                                  kappa, part, gear));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_loop_transits(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                             const double *to_y, const double *to_h, double radius, const int64_t *pair_field, int64_t n_fields,
                             const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y,
                             int64_t n_loops, const int64_t *loop_offsets, int64_t n_samples, const double *loop_x, const double *loop_y,
                             const double *loop_h, const double *loop_kappa, const double *loop_s, const int8_t *loop_part, const int8_t *loop_gear,
                             const int64_t *field_loops, int64_t stride, double spacing, int32_t *found, int64_t *loop, int64_t *st_i, int64_t *st_j,
                             int32_t *in_word, double *in_seg, double *in_len, int32_t *in_rank, int32_t *out_word, double *out_seg, double *out_len,
                             int32_t *out_rank, double *ride, double *total, int32_t *status, int64_t *path_offsets, int64_t cap, double *out_x,
                             double *out_y, double *heading, double *kappa, int8_t *part, int8_t *gear)
{
    int rc = transit_solve_args(mode, n, from_x, from_y, from_h, to_x, to_y, to_h, radius, pair_field, n_fields, ring_offsets, n_rings, vert_offsets,
                                n_verts, x, y, n_loops, loop_offsets, n_samples, loop_x && loop_y && loop_h && loop_kappa && loop_s && loop_part && loop_gear,
                                field_loops, stride);
    if (rc == FCPP_OK) rc = transit_spacing(radius, mode, spacing);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> rings, verts, loff, floops;
    rc = swath_fields(nullptr, n_fields, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = host_offsets(nullptr, n_loops, nullptr, loop_offsets, n_samples, "loop_offsets", loff);
    if (rc == FCPP_OK) rc = host_offsets(nullptr, n_fields, nullptr, field_loops, n_loops, "field_loops", floops);
    if (rc) return rc;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    const TransitLoops L = { n_fields, n_loops, field_loops, loop_offsets, loop_x, loop_y, loop_h, loop_kappa, loop_s, loop_part, loop_gear, stride };
    const int nseg = mode == 0 ? 3 : 5;
    // per field: the region's status, the loops' validity, the stations (at the place of the field's first sample)
    std::vector<int32_t> region_status, loops_ok;
    std::vector<int64_t> n_st, st_idx, st_loop, cnt;
    std::vector<TransitResult> res;
    try {
        region_status.assign((size_t)n_fields, 0); loops_ok.assign((size_t)n_fields, 0); n_st.assign((size_t)n_fields, 0);
        st_idx.assign((size_t)n_samples, 0); st_loop.assign((size_t)n_samples, 0); cnt.assign((size_t)n + 1, 0); res.resize((size_t)n);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    WorkerPool::parallel_for(n_fields, [&](int64_t f) {
        region_status[(size_t)f] = clear_field_status(F, f);
        loops_ok[(size_t)f] = transit_field_loops_ok(L, f) ? 1 : 0;
        const int64_t base = field_loops[f + 1] > field_loops[f] ? loop_offsets[field_loops[f]] : 0;
        n_st[(size_t)f] = transit_field_stations(L, f, st_idx.data() + base, st_loop.data() + base);
    });
    std::vector<char> big((size_t)n, 0), nomem((size_t)n, 0);
    WorkerPool::parallel_for(n, [&](int64_t p) {
        const int64_t f = pair_field[p];
        const double x0 = from_x[p], y0 = from_y[p], h0 = from_h[p], x1 = to_x[p], y1 = to_y[p], h1 = to_h[p];
        const int stt = transit_pair_status(x0, y0, h0, x1, y1, h1, f, n_fields, region_status.data(), loops_ok.data(), n_st.data());
        TransitPick pick = transit_pick_none();
        if (stt == TRANSIT_OK && n_st[(size_t)f] > 0) {
            const int64_t base = loop_offsets[field_loops[f]], m = n_st[(size_t)f];
            std::vector<double> in, out;
            try { in.assign((size_t)m, 0.0); out.assign((size_t)m, 0.0); } catch (const std::bad_alloc &) { nomem[(size_t)p] = 1; return; }
            pick = mode == 0 ? transit_pick_host<0>(F, L, f, x0, y0, h0, x1, y1, h1, radius, m, st_idx.data() + base, st_loop.data() + base, in.data(), out.data())
                             : transit_pick_host<1>(F, L, f, x0, y0, h0, x1, y1, h1, radius, m, st_idx.data() + base, st_loop.data() + base, in.data(), out.data());
        }
        const TransitResult r = mode == 0 ? transit_finish<0>(F, L, f, x0, y0, h0, x1, y1, h1, radius, stt, pick)
                                          : transit_finish<1>(F, L, f, x0, y0, h0, x1, y1, h1, radius, stt, pick);
        res[(size_t)p] = r;
        if (found) found[p] = r.found;
        if (loop) loop[p] = r.loop;
        if (st_i) st_i[p] = r.i;
        if (st_j) st_j[p] = r.j;
        if (in_word) in_word[p] = r.in.word;
        if (out_word) out_word[p] = r.out.word;
        for (int k = 0; k < nseg; ++k) {
            if (in_seg) in_seg[p * nseg + k] = r.in.seg[k];
            if (out_seg) out_seg[p * nseg + k] = r.out.seg[k];
        }
        if (in_len) in_len[p] = r.in.len;
        if (out_len) out_len[p] = r.out.len;
        if (in_rank) in_rank[p] = r.in.rank;
        if (out_rank) out_rank[p] = r.out.rank;
        if (ride) ride[p] = r.ride;
        if (total) total[p] = r.total;
        if (status) status[p] = r.status;
    });
    for (int64_t p = 0; p < n; ++p)
        if (nomem[(size_t)p]) return fail(FCPP_ENOMEM, "out of host memory");
    if (!path_offsets && (cap == 0 || !(out_x || out_y || heading || kappa || part || gear))) return FCPP_OK;
    // the sampled paths, from the results as a caller would hand them back (one pair at a time: NSEG segments in place)
    auto rec_of = [&](const TransitResult &r, int32_t &fnd, int64_t *ids, int32_t *words) {
        fnd = r.found; ids[0] = r.loop; ids[1] = r.i; ids[2] = r.j; words[0] = r.in.word; words[1] = r.out.word;
        return TransitRec{ &fnd, ids, ids + 1, ids + 2, words, r.in.seg, words + 1, r.out.seg };
    };
    WorkerPool::parallel_for(n, [&](int64_t p) {
        int32_t fnd, words[2];
        int64_t ids[3], a, b, c2, bad = 0;
        const TransitRec rec = rec_of(res[(size_t)p], fnd, ids, words);
        if (mode == 0) transit_counts<0>(rec, n_loops, loop_offsets, spacing, 0, a, b, c2, bad);
        else transit_counts<1>(rec, n_loops, loop_offsets, spacing, 0, a, b, c2, bad);
        cnt[(size_t)p + 1] = a + b + c2;
        big[(size_t)p] = bad != 0;
    });
    for (int64_t p = 0; p < n; ++p) {
        if (big[(size_t)p]) return fail(FCPP_ESIZE, "a transit has 2^31 samples or more");
        cnt[(size_t)p + 1] += cnt[(size_t)p];
    }
    if (path_offsets) memcpy(path_offsets, cnt.data(), cnt.size() * sizeof(int64_t));
    if (cap == 0 || !(out_x || out_y || heading || kappa || part || gear)) return FCPP_OK;
    WorkerPool::parallel_for(n, [&](int64_t p) {
        int32_t fnd, words[2];
        int64_t ids[3];
        const TransitRec rec = rec_of(res[(size_t)p], fnd, ids, words);
        const int64_t at = cnt[(size_t)p], K = cnt[(size_t)p + 1] - at;
        for (int64_t k = 0; k < K && at + k < cap; ++k) {
            double px, py, ph, pk;
            int pp, pg;
            if (mode == 0) transit_eval<0>(rec, L, from_x + p, from_y + p, from_h + p, radius, spacing, 0, k, K, px, py, ph, pk, pp, pg);
            else transit_eval<1>(rec, L, from_x + p, from_y + p, from_h + p, radius, spacing, 0, k, K, px, py, ph, pk, pp, pg);
            if (out_x) out_x[at + k] = px;
            if (out_y) out_y[at + k] = py;
            if (heading) heading[at + k] = ph;
            if (kappa) kappa[at + k] = pk;
            if (part) part[at + k] = (int8_t)pp;
            if (gear) gear[at + k] = (int8_t)pg;
        }
    });
    return FCPP_OK;
}

}  // extern "C"

// ---- polygon coverage (fcpp_pcover.hip; the rule: fcpp_pcoverfn.h) ----------------------------------------------------------------------
namespace {
// what fcpp_polygon_cover_sizes, fcpp_polygon_cover and fcpp_debug_polygon_cover check alike
int pcover_args(int64_t n, const void *ring_offsets, int64_t n_rings, const void *vert_offsets, int64_t n_verts, const double *x, const double *y,
                double W, double res)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y))) return fail(FCPP_EINVAL, "bad arguments");
    if (!(W > 0.0) || !isfinite(W)) return fail(FCPP_EINVAL, "width must be positive and finite");
    if (!(res > 0.0) || !isfinite(res)) return fail(FCPP_EINVAL, "res must be positive and finite");
    if (n < 0 || n_rings < 0 || n_verts < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

int pcover_path_args(int64_t n, int caps, int64_t n_paths, const void *path_offsets, int64_t total_points, const double *x, const double *y,
                     const void *field_path_offsets)
{
    if (!path_offsets || !field_path_offsets || (total_points > 0 && (!x || !y))) return fail(FCPP_EINVAL, "bad arguments");
    if (caps != 0 && caps != 1) return fail(FCPP_EINVAL, "caps must be 0 (flat) or 1 (round)");
    if (n_paths < 0 || total_points < 0 || n_paths > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

// The paths of the fields, on the host and checked: poff (n_paths + 1), fpo (n + 1) and ids (fpo[n] entries, or NULL for the identity).
// -> the chunk table in field order and the fields' first chunks.
int pcover_chunks(int64_t n, int64_t n_paths, const std::vector<int64_t> &poff, const std::vector<int64_t> &fpo, const int64_t *ids,
                  std::vector<PcoverChunk> &chunks, std::vector<int64_t> &chunk_first)
{
    const int64_t S = fpo[(size_t)n];
    if (!ids && S > n_paths) return fail(FCPP_ESIZE, "field_path_offsets name more paths than there are");
    try {
        chunk_first.assign((size_t)n + 1, 0);
        chunks.clear();
        for (int64_t i = 0; i < n; ++i) {
            chunk_first[(size_t)i] = (int64_t)chunks.size();
            for (int64_t s = fpo[(size_t)i]; s < fpo[(size_t)i + 1]; ++s) {
                const int64_t p = ids ? ids[s] : s;
                if (p < 0 || p >= n_paths) return fail(FCPP_EINVAL, "path_ids must lie in [0, n_paths)");
                const int64_t p0 = poff[(size_t)p], p1 = poff[(size_t)p + 1];
                for (int64_t k = p0; k + 1 < p1; k += PCOVER_CHUNK)
                    chunks.push_back({ k, p0, p1, (int32_t)std::min<int64_t>(PCOVER_CHUNK, p1 - 1 - k), (int32_t)p });
            }
            if ((int64_t)chunks.size() > INT32_MAX) return fail(FCPP_ESIZE, "2^31 chunks of paths or more");
        }
        chunk_first[(size_t)n] = (int64_t)chunks.size();
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    return FCPP_OK;
}
}  // namespace

extern "C" {

int fcpp_polygon_cover_sizes(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                             const double *x, const double *y, double width, double res, void *dims, int64_t *cell_offsets,
                             int64_t *cell_offsets_host, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!dims || !cell_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = pcover_args(n, ring_offsets, n_rings, vert_offsets, n_verts, x, y, width, res);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> rings, verts;
    rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    return sample_counts(c, n, cell_offsets, cell_offsets_host, "the cells could not be scanned", [&](hipStream_t st, int64_t *err) {
        const int e = launch_pcover_sizes(st, n, ring_offsets, vert_offsets, x, y, width, res, (PcoverDims *)dims, status);
        return e ? e : launch_pcover_offsets(st, n, (const PcoverDims *)dims, cell_offsets, nullptr, err);
    });
}

// Like the path operators' fill entries, the cover call RECOMPUTES the grids from its inputs: the two entries stay stateless, and the
// kernels place every field by the offsets computed here -- the caller's offsets only have to end at the same total.
int fcpp_polygon_cover(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                       const double *x, const double *y, double width, double res, int caps, int64_t n_paths, const int64_t *path_offsets,
                       const int64_t *path_offsets_host, int64_t total_points, const double *px, const double *py, const uint8_t *work,
                       const int32_t *pass, const int64_t *field_path_offsets, const int64_t *path_ids, const int64_t *cell_offsets,
                       const int64_t *cell_offsets_host, uint8_t *grid, int64_t *counts, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && !counts) || (grid && !cell_offsets && !cell_offsets_host)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = pcover_args(n, ring_offsets, n_rings, vert_offsets, n_verts, x, y, width, res);
    if (rc == FCPP_OK) rc = pcover_path_args(n, caps, n_paths, path_offsets, total_points, px, py, field_path_offsets);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<int64_t> rings, verts, poff, fpo, ids;
    rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = host_offsets(c, n_paths, path_offsets, path_offsets_host, total_points, "path_offsets", poff);
    if (rc) return rc;
    try { fpo.assign((size_t)n + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    HIPCHK(hipMemcpyAsync(fpo.data(), field_path_offsets, fpo.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (fpo[0] != 0) return fail(FCPP_ESIZE, "field_path_offsets must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (fpo[(size_t)i + 1] < fpo[(size_t)i]) return fail(FCPP_ESIZE, "field_path_offsets must be non-decreasing");
    if (fpo[(size_t)n] > ((int64_t)1 << 31)) return fail(FCPP_ESIZE, "field_path_offsets name 2^31 paths or more");
    if (path_ids && fpo[(size_t)n] > 0) {
        try { ids.assign((size_t)fpo[(size_t)n], 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
        HIPCHK(hipMemcpyAsync(ids.data(), path_ids, ids.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    std::vector<PcoverChunk> chunks;
    std::vector<int64_t> chunk_first;
    rc = pcover_chunks(n, n_paths, poff, fpo, path_ids ? ids.data() : nullptr, chunks, chunk_first);
    if (rc) return rc;

    DevBuf<PcoverDims> dims;
    DevBuf<int64_t> cell_first, tile_first, err, d_chunk_first;
    DevBuf<int32_t> own_status;
    DevBuf<PcoverChunk> d_chunks;
    DevBuf<PcoverBox> boxes;
    HIPCHK(dims.alloc((size_t)n));
    HIPCHK(cell_first.alloc((size_t)n + 1));
    HIPCHK(tile_first.alloc((size_t)n + 1));
    HIPCHK(err.alloc(1));
    if (!status) { HIPCHK(own_status.alloc((size_t)n)); status = own_status.p; }
    LAUNCHCHK(launch_pcover_sizes(st, n, ring_offsets, vert_offsets, x, y, width, res, dims.p, status));
    LAUNCHCHK(launch_pcover_offsets(st, n, dims.p, cell_first.p, tile_first.p, err.p));
    int64_t totals[3] = { 0, 0, 0 };           // cells, tiles, the caller's cells
    HIPCHK(hipMemcpyAsync(&totals[0], cell_first.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&totals[1], tile_first.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (grid) {
        if (cell_offsets_host) totals[2] = cell_offsets_host[n];
        else HIPCHK(hipMemcpyAsync(&totals[2], cell_offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    if (n > 0) HIPCHK(hipMemsetAsync(counts, 0, (size_t)n * 4 * sizeof(int64_t), st));
    HIPCHK(d_chunks.upload(chunks, st));
    HIPCHK(d_chunk_first.upload(chunk_first, st));
    HIPCHK(boxes.alloc(chunks.size()));
    HIPCHK(hipStreamSynchronize(st));
    if (grid && totals[2] != totals[0]) return fail(FCPP_ESIZE, "cell_offsets do not end at the cells of these fields: call fcpp_polygon_cover_sizes");
    if (totals[1] > INT32_MAX) return fail(FCPP_ESIZE, "2^31 tiles or more");
    const PcoverPaths P = { px, py, work, pass };
    const PcoverFields F = { ring_offsets, vert_offsets, x, y, dims.p, cell_first.p, tile_first.p, d_chunk_first.p };
    LAUNCHCHK(launch_pcover_boxes(st, (int64_t)chunks.size(), d_chunks.p, P, boxes.p));
    LAUNCHCHK(launch_pcover_tiles(st, n, totals[1], F, width, res, caps, d_chunks.p, boxes.p, P, grid, (unsigned long long *)counts));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

int fcpp_debug_polygon_cover(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                             const double *y, double width, double res, int caps, int64_t n_paths, const int64_t *path_offsets, int64_t total_points,
                             const double *px, const double *py, const uint8_t *work, const int32_t *pass, const int64_t *field_path_offsets,
                             const int64_t *path_ids, void *dims_out, int64_t *cell_offsets, int64_t cell_cap, uint8_t *grid, int64_t *counts,
                             int32_t *status)
{
    int rc = pcover_args(n, ring_offsets, n_rings, vert_offsets, n_verts, x, y, width, res);
    if (rc == FCPP_OK && counts) rc = pcover_path_args(n, caps, n_paths, path_offsets, total_points, px, py, field_path_offsets);
    if (rc == FCPP_OK && cell_cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> rings, verts, poff, fpo, cells;
    rc = swath_fields(nullptr, n, nullptr, ring_offsets, n_rings, nullptr, vert_offsets, n_verts, rings, verts);
    if (rc) return rc;
    std::vector<PcoverDims> dims;
    try { dims.resize((size_t)n); cells.assign((size_t)n + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (int64_t i = 0; i < n; ++i) {
        const int st = pcover_field_dims_host(verts.data(), rings[(size_t)i], rings[(size_t)i + 1], x, y, width, res, dims[(size_t)i]);
        if (status) status[i] = st;
        cells[(size_t)i + 1] = cells[(size_t)i] + dims[(size_t)i].nx * dims[(size_t)i].ny;
    }
    if (dims_out && n > 0) memcpy(dims_out, dims.data(), dims.size() * sizeof(PcoverDims));
    if (cell_offsets) memcpy(cell_offsets, cells.data(), cells.size() * sizeof(int64_t));
    if (!counts) return FCPP_OK;
    rc = host_offsets(nullptr, n_paths, nullptr, path_offsets, total_points, "path_offsets", poff);
    if (rc) return rc;
    try { fpo.assign(field_path_offsets, field_path_offsets + n + 1); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    std::vector<PcoverChunk> chunks;          // (built only for the checks the device entry makes: the same errors for the same arguments)
    std::vector<int64_t> chunk_first;
    if (fpo[0] != 0) return fail(FCPP_ESIZE, "field_path_offsets must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (fpo[(size_t)i + 1] < fpo[(size_t)i]) return fail(FCPP_ESIZE, "field_path_offsets must be non-decreasing");
    if (fpo[(size_t)n] > ((int64_t)1 << 31)) return fail(FCPP_ESIZE, "field_path_offsets name 2^31 paths or more");
    rc = pcover_chunks(n, n_paths, poff, fpo, path_ids, chunks, chunk_first);
    if (rc) return rc;
    const bool want_grid = grid && cells[(size_t)n] <= cell_cap;
    const PcoverPaths P = { px, py, work, pass };
    // fields to the library's host threads: every field writes only its own counts and cells
    try {
        WorkerPool::parallel_for(n, [&](int64_t i) {
            const PcoverDims &d = dims[(size_t)i];
            const int64_t nc = d.nx * d.ny, r0 = rings[(size_t)i], r1 = rings[(size_t)i + 1];
            int64_t *cnt = counts + 4 * i;
            cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
            if (nc == 0) return;
            std::vector<uint8_t> own;
            std::vector<int32_t> first((size_t)nc);
            std::vector<double> cross((size_t)(verts[(size_t)r1] - verts[(size_t)r0]));
            uint8_t *bits = want_grid ? grid + cells[(size_t)i] : (own.resize((size_t)nc), own.data());
            pcover_field_host(verts.data(), r0, r1, x, y, d, width, res, caps, poff.data(), P, path_ids, fpo[(size_t)i], fpo[(size_t)i + 1], bits,
                              first.data(), cross.data(), cnt);
        });
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    return FCPP_OK;
}

}  // extern "C"

// ---- coverage regions (fcpp_regions.hip; the rule: fcpp_regionfn.h) ---------------------------------------------------------------------
namespace {
// The grids of a call on the host, checked before any kernel runs: the fields' dims and cell offsets (the caller's host copy, or read
// back), and what the kernels place their work by: the fields' first tiles and first numbering blocks.
struct RegionTables {
    std::vector<RegionDims> dims;
    std::vector<int64_t> cells, tile_first, block_first;
};

int region_tables(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host, RegionTables &T)
{
    if (n < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    try {
        T.dims.resize((size_t)n); T.cells.assign((size_t)n + 1, 0); T.tile_first.assign((size_t)n + 1, 0); T.block_first.assign((size_t)n + 1, 0);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (c) {
        if (n > 0) HIPCHK(hipMemcpyAsync(T.dims.data(), dims, (size_t)n * sizeof(RegionDims), hipMemcpyDeviceToHost, c->stream));
        if (!cell_offsets_host) HIPCHK(hipMemcpyAsync(T.cells.data(), cell_offsets, T.cells.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (cell_offsets_host) memcpy(T.cells.data(), cell_offsets_host, T.cells.size() * sizeof(int64_t));
    } else {
        if (n > 0) memcpy(T.dims.data(), dims, (size_t)n * sizeof(RegionDims));
        memcpy(T.cells.data(), cell_offsets, T.cells.size() * sizeof(int64_t));
    }
    if (T.cells[0] != 0) return fail(FCPP_ESIZE, "cell_offsets must start at 0");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t nx = T.dims[(size_t)i].nx, ny = T.dims[(size_t)i].ny, nc = T.cells[(size_t)i + 1] - T.cells[(size_t)i];
        if (nc < 0) return fail(FCPP_ESIZE, "cell_offsets must be non-decreasing");
        if (nx < 0 || ny < 0 || nx > REGION_MAX_CELLS || ny > REGION_MAX_CELLS || nx * ny > REGION_MAX_CELLS)
            return fail(FCPP_ESIZE, "a field's grid is negative or has more than 2^28 cells");
        if (nx * ny != nc) return fail(FCPP_ESIZE, "cell_offsets disagree with dims: a field's cells are not nx ny");
        T.tile_first[(size_t)i + 1] = T.tile_first[(size_t)i] + ((nx + REGION_TILE - 1) / REGION_TILE) * ((ny + REGION_TILE - 1) / REGION_TILE);
        T.block_first[(size_t)i + 1] = T.block_first[(size_t)i] + (nc + REGION_BLOCK_CELLS - 1) / REGION_BLOCK_CELLS;
    }
    if (T.tile_first[(size_t)n] > INT32_MAX || T.block_first[(size_t)n] > INT32_MAX) return fail(FCPP_ESIZE, "2^31 tiles or numbering blocks or more");
    return FCPP_OK;
}

// region offsets on the host, checked: start at 0, never decrease, end at n_regions
int region_offsets_check(const std::vector<int64_t> &ro, int64_t n, int64_t n_regions)
{
    if (ro[0] != 0) return fail(FCPP_ESIZE, "region_offsets must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (ro[(size_t)i + 1] < ro[(size_t)i]) return fail(FCPP_ESIZE, "region_offsets must be non-decreasing");
    if (ro[(size_t)n] != n_regions) return fail(FCPP_ESIZE, "n_regions is not the total of region_offsets");
    return FCPP_OK;
}

// the seam kernel's launch: workgroups per compute unit of the context's device (each strides over the seam lanes)
int region_seam_blocks(const fcpp_ctx *c) { return 4 * (c->n_cu > 0 ? c->n_cu : 64); }

struct RegionDevice {
    DevBuf<int64_t> tile_first, block_first, block_count, block_prefix, err;
    RegionFields F;
    int upload(fcpp_ctx *c, const RegionTables &T, const void *dims, const int64_t *cell_offsets)
    {
        HIPCHK(tile_first.upload(T.tile_first, c->stream));
        HIPCHK(block_first.upload(T.block_first, c->stream));
        HIPCHK(block_count.alloc((size_t)T.block_first.back()));
        HIPCHK(block_prefix.alloc((size_t)T.block_first.back() + 1));
        HIPCHK(err.alloc(1));
        F = { (const RegionDims *)dims, cell_offsets, tile_first.p, block_first.p };
        return FCPP_OK;
    }
};
}  // namespace

extern "C" {

int fcpp_cover_regions_counts(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host,
                              const uint8_t *grid, int mask, int value, int connectivity, int32_t *labels, int64_t *region_offsets,
                              int64_t *region_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && !dims) || !cell_offsets || !region_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (!region_args_ok(mask, value, connectivity))
        return fail(FCPP_EINVAL, "mask and value must lie in 0 .. 255 with value & ~mask == 0, connectivity must be 4 or 8");
    HIPCHK(hipSetDevice(c->device));
    RegionTables T;
    int rc = region_tables(c, n, dims, cell_offsets, cell_offsets_host, T);
    if (rc) return rc;
    if (T.cells[(size_t)n] > 0 && (!grid || !labels)) return fail(FCPP_EINVAL, "bad arguments");
    hipStream_t st = c->stream;
    RegionDevice D;
    rc = D.upload(c, T, dims, cell_offsets);
    if (rc) return rc;
    const int64_t n_tiles = T.tile_first[(size_t)n], n_blocks = T.block_first[(size_t)n];
    LAUNCHCHK(launch_region_tiles(st, n, n_tiles, D.F, grid, mask, value, connectivity, labels));
    LAUNCHCHK(launch_region_seams(st, n, n_tiles, D.F, connectivity, labels, region_seam_blocks(c)));
    LAUNCHCHK(launch_region_count(st, n, n_blocks, D.F, 1, labels, D.block_count.p));
    LAUNCHCHK(launch_region_offsets(st, n, n_blocks, D.F, D.block_count.p, D.block_prefix.p, D.err.p, region_offsets));
    if (region_offsets_host)
        HIPCHK(hipMemcpyAsync(region_offsets_host, region_offsets, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

// Like the cover call, the fill call RECOMPUTES what it needs (the roots' ranks) from its inputs: nothing is kept in the context.
int fcpp_cover_regions_fill(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host, int32_t *labels,
                            const int64_t *region_offsets, const int64_t *region_offsets_host, int64_t n_regions, void *records)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && !dims) || !cell_offsets || !region_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (n_regions < 0) return fail(FCPP_ESIZE, "bad sizes");
    HIPCHK(hipSetDevice(c->device));
    RegionTables T;
    int rc = region_tables(c, n, dims, cell_offsets, cell_offsets_host, T);
    if (rc) return rc;
    if ((T.cells[(size_t)n] > 0 && !labels) || (n_regions > 0 && !records)) return fail(FCPP_EINVAL, "bad arguments");
    hipStream_t st = c->stream;
    std::vector<int64_t> ro;
    try { ro.assign((size_t)n + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (region_offsets_host) memcpy(ro.data(), region_offsets_host, ro.size() * sizeof(int64_t));
    else {
        HIPCHK(hipMemcpyAsync(ro.data(), region_offsets, ro.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    rc = region_offsets_check(ro, n, n_regions);
    if (rc) return rc;
    RegionDevice D;
    rc = D.upload(c, T, dims, cell_offsets);
    if (rc) return rc;
    const int64_t n_blocks = T.block_first[(size_t)n];
    if (n_regions > 0) HIPCHK(hipMemsetAsync(records, 0, (size_t)n_regions * sizeof(RegionRecord), st));
    LAUNCHCHK(launch_region_count(st, n, n_blocks, D.F, 0, labels, D.block_count.p));
    LAUNCHCHK(launch_region_offsets(st, n, n_blocks, D.F, D.block_count.p, D.block_prefix.p, D.err.p, nullptr));
    LAUNCHCHK(launch_region_first(st, n, n_blocks, D.F, labels, D.block_prefix.p, region_offsets, (RegionRecord *)records));
    LAUNCHCHK(launch_region_fill(st, n, n_blocks, D.F, labels, region_offsets, (RegionRecord *)records));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

int fcpp_debug_cover_regions(int64_t n, const void *dims, const int64_t *cell_offsets, const uint8_t *grid, int mask, int value, int connectivity,
                             int64_t *region_offsets, int64_t region_cap, void *records, int32_t *labels_counts, int32_t *labels_fill)
{
    if ((n > 0 && !dims) || !cell_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (!region_args_ok(mask, value, connectivity))
        return fail(FCPP_EINVAL, "mask and value must lie in 0 .. 255 with value & ~mask == 0, connectivity must be 4 or 8");
    if (region_cap < 0) return fail(FCPP_ESIZE, "bad sizes");
    RegionTables T;
    const int rc = region_tables(nullptr, n, dims, cell_offsets, nullptr, T);
    if (rc) return rc;
    if (T.cells[(size_t)n] > 0 && !grid) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<std::vector<RegionRecord>> per;
    std::vector<int64_t> ro;
    // fields to the library's host threads: every field writes only its own records and labels
    try {
        per.resize((size_t)n); ro.assign((size_t)n + 1, 0);
        WorkerPool::parallel_for(n, [&](int64_t i) {
            const int64_t nx = T.dims[(size_t)i].nx, ny = T.dims[(size_t)i].ny, at = T.cells[(size_t)i];
            if (nx * ny == 0) return;
            std::vector<int32_t> parent((size_t)(nx * ny));
            region_field_host(grid + at, nx, ny, mask, value, connectivity, parent.data(), labels_counts ? labels_counts + at : nullptr,
                              labels_fill ? labels_fill + at : nullptr, per[(size_t)i]);
        });
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (int64_t i = 0; i < n; ++i) ro[(size_t)i + 1] = ro[(size_t)i] + (int64_t)per[(size_t)i].size();
    if (region_offsets) memcpy(region_offsets, ro.data(), ro.size() * sizeof(int64_t));
    if (records && ro[(size_t)n] <= region_cap)
        for (int64_t i = 0; i < n; ++i)
            if (!per[(size_t)i].empty())
                memcpy((RegionRecord *)records + ro[(size_t)i], per[(size_t)i].data(), per[(size_t)i].size() * sizeof(RegionRecord));
    return FCPP_OK;
}

}  // extern "C"

// ---- patch passes (fcpp_patch.hip; the rule: fcpp_patchfn.h) ------------------------------------------------------------------------------
namespace {
// what every patch entry checks of its scalars and its region offsets, before any kernel runs
int patch_call_args(fcpp_ctx *c, int64_t n, double res, double width, double margin, double join, const int64_t *region_offsets,
                    const int64_t *region_offsets_host, int64_t n_regions, std::vector<int64_t> &ro)
{
    if (!patch_args_ok(res, width, margin, join))
        return fail(FCPP_EINVAL, "res and width must be positive, 0 <= margin with width - 2 margin > 0, join >= 0, all finite");
    if (n < 0 || n > INT32_MAX || n_regions < 0) return fail(FCPP_ESIZE, "bad sizes");
    try { ro.assign((size_t)n + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (!c || region_offsets_host) memcpy(ro.data(), region_offsets_host ? region_offsets_host : region_offsets, ro.size() * sizeof(int64_t));
    else {
        HIPCHK(hipMemcpyAsync(ro.data(), region_offsets, ro.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return region_offsets_check(ro, n, n_regions);
}

// the field angles on the host, checked
int patch_angles(fcpp_ctx *c, int64_t n, const double *angle, std::vector<double> &th)
{
    try { th.assign((size_t)n, 0.0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (n > 0 && c) {
        HIPCHK(hipMemcpyAsync(th.data(), angle, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    } else if (n > 0) memcpy(th.data(), angle, (size_t)n * sizeof(double));
    for (int64_t i = 0; i < n; ++i)
        if (!patch_angle_ok(th[(size_t)i])) return fail(FCPP_EINVAL, "a field's angle is not finite or beyond 1e5 in magnitude");
    return FCPP_OK;
}

// the runs kernel's launch: workgroups per compute unit of the context's device (each wavefront strides over the lines)
int patch_runs_blocks(const fcpp_ctx *c) { return 4 * (c->n_cu > 0 ? c->n_cu : 64); }

PatchRule patch_rule(double res, double width, double margin, double join) { return { res, width - 2.0 * margin, margin, patch_join_bins(join, res) }; }
}  // namespace

extern "C" {

int fcpp_patch_sizes(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host, double res,
                     const int32_t *labels, const int64_t *region_offsets, const int64_t *region_offsets_host, int64_t n_regions, const double *angle,
                     double width, double margin, double join, double *frame, void *records, int64_t *totals_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && (!dims || !angle || !frame)) || !cell_offsets || !region_offsets || !totals_host) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> ro;
    int rc = patch_call_args(c, n, res, width, margin, join, region_offsets, region_offsets_host, n_regions, ro);
    if (rc) return rc;
    RegionTables T;
    rc = region_tables(c, n, dims, cell_offsets, cell_offsets_host, T);
    if (rc) return rc;
    if ((T.cells[(size_t)n] > 0 && !labels) || (n_regions > 0 && !records)) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<double> th;
    rc = patch_angles(c, n, angle, th);
    if (rc) return rc;
    hipStream_t st = c->stream;
    DevBuf<int64_t> block_first, line_first, word_first, err;
    HIPCHK(block_first.upload(T.block_first, st));
    HIPCHK(line_first.alloc((size_t)n_regions + 1));
    HIPCHK(word_first.alloc((size_t)n_regions + 1));
    HIPCHK(err.alloc(1));
    const PatchFields F = { (const RegionDims *)dims, cell_offsets, block_first.p, region_offsets, frame };
    const PatchRule rule = patch_rule(res, width, margin, join);
    if (n_regions > 0) HIPCHK(hipMemsetAsync(records, 0, (size_t)n_regions * sizeof(PatchRecord), st));
    LAUNCHCHK(launch_patch_frame(st, n, angle, frame));
    if (n_regions > 0) LAUNCHCHK(launch_patch_extent(st, n, T.block_first[(size_t)n], F, rule, labels, (PatchRecord *)records));
    LAUNCHCHK(launch_patch_layout(st, n_regions, rule, (PatchRecord *)records, line_first.p, word_first.p, err.p));
    HIPCHK(hipMemcpyAsync(totals_host, line_first.p + n_regions, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(totals_host + 1, word_first.p + n_regions, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

int fcpp_patch_counts(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host, double res,
                      const int32_t *labels, const int64_t *region_offsets, const int64_t *region_offsets_host, int64_t n_regions, const double *frame,
                      double width, double margin, double join, const void *records, int64_t n_lines, int64_t n_words, uint64_t *bitmap,
                      int64_t *line_counts, int64_t *line_offsets, int64_t *swath_offsets, int64_t *swath_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && (!dims || !frame)) || !cell_offsets || !region_offsets || !line_offsets || !swath_offsets) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> ro;
    int rc = patch_call_args(c, n, res, width, margin, join, region_offsets, region_offsets_host, n_regions, ro);
    if (rc) return rc;
    if (n_lines < 0 || n_words < 0) return fail(FCPP_ESIZE, "bad sizes");
    RegionTables T;
    rc = region_tables(c, n, dims, cell_offsets, cell_offsets_host, T);
    if (rc) return rc;
    if ((T.cells[(size_t)n] > 0 && !labels) || (n_regions > 0 && !records) || (n_words > 0 && !bitmap) || (n_lines > 0 && !line_counts))
        return fail(FCPP_EINVAL, "bad arguments");
    hipStream_t st = c->stream;
    DevBuf<int64_t> block_first, err;
    HIPCHK(block_first.upload(T.block_first, st));
    HIPCHK(err.alloc(1));
    const PatchFields F = { (const RegionDims *)dims, cell_offsets, block_first.p, region_offsets, frame };
    const PatchRule rule = patch_rule(res, width, margin, join);
    const PatchSwaths none = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
    if (n_words > 0) HIPCHK(hipMemsetAsync(bitmap, 0, (size_t)n_words * sizeof(uint64_t), st));
    if (n_lines > 0) HIPCHK(hipMemsetAsync(line_counts, 0, (size_t)n_lines * sizeof(int64_t), st));
    if (n_regions > 0)
        LAUNCHCHK(launch_patch_mark(st, n, T.block_first[(size_t)n], F, rule, labels, (const PatchRecord *)records, n_words, (unsigned long long *)bitmap));
    LAUNCHCHK(launch_patch_runs(st, 0, n, n_regions, n_lines, n_words, F, rule, (const PatchRecord *)records, (const unsigned long long *)bitmap,
                                line_counts, nullptr, none, patch_runs_blocks(c)));
    LAUNCHCHK(launch_patch_offsets(st, n, n_regions, n_lines, F, (const PatchRecord *)records, line_counts, line_offsets, err.p, swath_offsets));
    if (swath_offsets_host)
        HIPCHK(hipMemcpyAsync(swath_offsets_host, swath_offsets, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

int fcpp_patch_fill(fcpp_ctx *c, int64_t n, const void *dims, double res, const int64_t *region_offsets, const int64_t *region_offsets_host,
                    int64_t n_regions, const double *frame, double width, double margin, double join, const void *records, int64_t n_lines,
                    int64_t n_words, const uint64_t *bitmap, const int64_t *line_offsets, int64_t n_swaths, double *ax, double *ay, double *bx, double *by,
                    int32_t *line, double *length, int64_t *region)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && (!dims || !frame)) || !region_offsets || !line_offsets) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> ro;
    int rc = patch_call_args(c, n, res, width, margin, join, region_offsets, region_offsets_host, n_regions, ro);
    if (rc) return rc;
    if (n_lines < 0 || n_words < 0 || n_swaths < 0) return fail(FCPP_ESIZE, "bad sizes");
    if ((n_regions > 0 && !records) || (n_words > 0 && !bitmap) || (n_swaths > 0 && (!ax || !ay || !bx || !by || !line || !length || !region)))
        return fail(FCPP_EINVAL, "bad arguments");
    hipStream_t st = c->stream;
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, line_offsets + n_lines, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total != n_swaths) return fail(FCPP_ESIZE, "n_swaths is not the total of line_offsets");
    const PatchFields F = { (const RegionDims *)dims, nullptr, nullptr, region_offsets, frame };
    const PatchRule rule = patch_rule(res, width, margin, join);
    const PatchSwaths out = { ax, ay, bx, by, length, line, region, n_swaths };
    if (n_swaths > 0)
        LAUNCHCHK(launch_patch_runs(st, 1, n, n_regions, n_lines, n_words, F, rule, (const PatchRecord *)records, (const unsigned long long *)bitmap,
                                    nullptr, line_offsets, out, patch_runs_blocks(c)));
    HIPCHK(hipStreamSynchronize(st));
    return FCPP_OK;
}

int fcpp_debug_patch_swaths(int64_t n, const void *dims, const int64_t *cell_offsets, double res, const int32_t *labels, const int64_t *region_offsets,
                            int64_t n_regions, const double *angle, double width, double margin, double join, double *frame, void *records,
                            int64_t *totals, int64_t word_cap, uint64_t *bitmap, int64_t line_cap, int64_t *line_counts, int64_t *line_offsets,
                            int64_t *swath_offsets, int64_t swath_cap, double *ax, double *ay, double *bx, double *by, int32_t *line, double *length,
                            int64_t *region)
{
    if ((n > 0 && (!dims || !angle)) || !cell_offsets || !region_offsets) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<int64_t> ro;
    int rc = patch_call_args(nullptr, n, res, width, margin, join, region_offsets, nullptr, n_regions, ro);
    if (rc) return rc;
    if (word_cap < 0 || line_cap < 0 || swath_cap < 0) return fail(FCPP_ESIZE, "bad sizes");
    RegionTables T;
    rc = region_tables(nullptr, n, dims, cell_offsets, nullptr, T);
    if (rc) return rc;
    if (T.cells[(size_t)n] > 0 && !labels) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<double> th;
    rc = patch_angles(nullptr, n, angle, th);
    if (rc) return rc;
    PatchHost o;
    try {
        // fields to the library's host threads: every field writes only its own regions' keys, words, counts and swaths
        patch_host(n, T.dims.data(), T.cells.data(), res, labels, ro.data(), th.data(), width, margin, join,
                   [](int64_t cnt, auto fn) { WorkerPool::parallel_for(cnt, fn); }, o);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    auto put = [](void *dst, const void *src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
    put(frame, o.frame.data(), o.frame.size() * sizeof(double));
    put(records, o.records.data(), o.records.size() * sizeof(PatchRecord));
    if (totals) { totals[0] = o.n_lines; totals[1] = o.n_words; totals[2] = o.n_swaths; }
    put(swath_offsets, o.swath_offsets.data(), o.swath_offsets.size() * sizeof(int64_t));
    if (o.n_words <= word_cap) put(bitmap, o.bitmap.data(), o.bitmap.size() * sizeof(uint64_t));
    if (o.n_lines <= line_cap) {
        put(line_counts, o.line_counts.data(), o.line_counts.size() * sizeof(int64_t));
        put(line_offsets, o.line_offsets.data(), o.line_offsets.size() * sizeof(int64_t));
    }
    if (o.n_swaths <= swath_cap) {
        const size_t m8 = (size_t)o.n_swaths * sizeof(double);
        put(ax, o.ax.data(), m8); put(ay, o.ay.data(), m8); put(bx, o.bx.data(), m8); put(by, o.by.data(), m8); put(length, o.length.data(), m8);
        put(line, o.line.data(), (size_t)o.n_swaths * sizeof(int32_t));
        put(region, o.region.data(), (size_t)o.n_swaths * sizeof(int64_t));
    }
    return FCPP_OK;
}

}  // extern "C"
