// fcpp_glue_polygon.cpp -- C-ABI glue of the polygon swaths and the polygon inset (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_inset.h"
#include "fcpp_insetfn.h"
#include "fcpp_swath.h"

using namespace fcpp;

namespace {
// ---- polygon swaths: what fcpp_swath_scores / _counts / _fill and fcpp_debug_swaths check alike ------------------------------------
int swath_params(double W, double first, double min_length)
{
    if (const int bad = positive_finite(W, "width")) return bad;
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

// ---- polygon inset: what fcpp_inset_counts / _fill and fcpp_debug_inset check alike --------------------------------------------------
int inset_sizes(int64_t n, int64_t n_rings, int64_t n_verts, int64_t D)
{
    if (n < 0 || n_rings < 0 || n_verts < 0 || D < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    if (D > 0 && n > INSET_MAX_PAIRS / D) return fail(FCPP_ESIZE, "2^31 (field, distance) pairs or more");
    return FCPP_OK;
}

// arc_step in (0, pi/2]; the D distances, read to the host: positive and finite
int inset_params(fcpp_ctx *c, int64_t D, const double *ptr, const double *host, double arc_step)
{
    if (!(arc_step > 0.0) || !(arc_step <= INSET_MAX_ARC_STEP)) return fail(FCPP_EINVAL, "arc_step must lie in (0, pi/2]");
    std::vector<double> dist;
    const int rc = host_table(c, D, ptr, host, dist);
    if (rc) return rc;
    for (const double d : dist)
        if (const int bad = positive_finite(d, "distances")) return bad;
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
}  // namespace

extern "C" {

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
    rc = swath_fields(nullptr, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, per_field ? n : A, angles, nullptr);
    if (rc) return rc;
    std::vector<double> u, w;
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t nv = verts[(size_t)rings[(size_t)i + 1]] - verts[(size_t)rings[(size_t)i]];
        try { u.resize((size_t)nv); w.resize((size_t)nv); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
        store(out_offsets, i, at);
        for (int64_t j = 0; j < A; ++j) {
            const SwathTotals t = swath_field_host(verts.data(), rings[(size_t)i], rings[(size_t)i + 1], x, y, angles[per_field ? i : j], W, first, min_length,
                                                   u.data(), w.data(), [&](int64_t k, double ua, double ub, double wk, double c, double s, double len) {
                if (!out_offsets) return;
                if (at < cap) {
                    double px, py, qx, qy;
                    swath_point(ua, wk, c, s, px, py);
                    swath_point(ub, wk, c, s, qx, qy);
                    store(ax, at, px); store(ay, at, py); store(bx, at, qx); store(by, at, qy); store(line, at, (int32_t)k);
                    store(seg_length, at, len);
                }
                ++at;
            });
            store(n_swaths, i * A + j, t.n_swaths); store(n_lines, i * A + j, t.n_lines); store(length, i * A + j, t.length);
            store(status, i * A + j, t.status);
        }
    }
    store(out_offsets, n, at);
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
    if (rc == FCPP_OK) rc = inset_params(nullptr, D, dist, nullptr, arc_step);
    std::vector<int64_t> rings, verts;
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    int64_t ring_at = 0, vert_at = 0;
    try {
        InsetWork work;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < D; ++j) {
                const int64_t pair = i * D + j;
                store(pair_ring_offsets, pair, ring_at); store(pair_vert_offsets, pair, vert_at);
                const InsetTotals t = inset_field_host(verts.data(), rings[(size_t)i], rings[(size_t)i + 1], x, y, dist[j], arc_step, work,
                    [&](int32_t r, int32_t off) { if (out_vert_offsets && ring_at + r < ring_cap) out_vert_offsets[ring_at + r] = vert_at + off; },
                    [&](int32_t at, double vx, double vy, int32_t src) {
                        if (vert_at + at >= vert_cap) return;
                        store(out_x, vert_at + at, vx); store(out_y, vert_at + at, vy); store(out_src, vert_at + at, src);
                    });
                store(status, pair, t.status); store(gap, pair, t.gap);
                ring_at += t.n_rings;
                vert_at += t.n_verts;
            }
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    store(pair_ring_offsets, n * D, ring_at); store(pair_vert_offsets, n * D, vert_at);
    if (out_vert_offsets && ring_at <= ring_cap) out_vert_offsets[ring_at] = vert_at;
    return FCPP_OK;
}

}  // extern "C"
