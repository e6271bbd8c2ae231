// fcpp_glue_conn.cpp -- C-ABI glue of the connectors: Dubins / Reeds-Shepp solve, matrix and sampler, clearance, clear connectors (shared: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_clear.h"
#include "fcpp_clearfn.h"
#include "fcpp_conn.h"
#include "fcpp_parallel.h"
#include "fcpp_solveclear.h"

using namespace fcpp;

namespace {
// ---- connectors: what the Dubins (mode 0) and Reeds-Shepp (mode 1) entries share: the argument checks, the launch ---------------------------
int conn_solve(fcpp_ctx *c, int mode, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
               const double *th, double radius, int32_t *word, double *seg, double *len)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (const int bad = positive_finite(radius, "radius")) return bad;
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
    if (const int bad = positive_finite(radius, "radius")) return bad;
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
    if (const int bad = positive_finite(radius, "radius")) return bad;
    if (const int bad = positive_finite(spacing, "spacing")) return bad;
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
            store(ok, i * NW + w, have ? 1 : 0); store(total, i * NW + w, have ? all.total[w] : __builtin_nan(""));
            if (seg)
                for (int k = 0; k < NSEG; ++k) seg[(i * NW + w) * NSEG + k] = have ? all.seg[w][k] : __builtin_nan("");
        }
    });
}
}  // namespace

extern "C" {

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
    if (const int bad = positive_finite(spacing, "spacing")) return bad;
    if (n < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    if (!out_offsets || (n > 0 && !len)) return fail(FCPP_EINVAL, "bad arguments");
    return sample_counts(c, n, out_offsets, out_offsets_host, "a path's length is negative or infinite, or it has 2^31 samples or more",
                         [&](hipStream_t st, int64_t *err) { return launch_dubins_counts(st, n, len, spacing, out_offsets, err); });
}

int fcpp_rs_counts(fcpp_ctx *c, int64_t n, const int32_t *word, const double *seg, double spacing, int64_t *out_offsets, int64_t *out_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (const int bad = positive_finite(spacing, "spacing")) return bad;
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

int fcpp_debug_conn_clear(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, double radius, const int32_t *word,
                          const double *seg, const int64_t *pair_field, int64_t n_fields, const int64_t *ring_offsets, int64_t n_rings,
                          const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y, int32_t *crossings, int8_t *inside,
                          double *first_s, int32_t *field_status)
{
    int rc = clear_conn_args(mode, n, from_x, from_y, from_h, radius, word, seg, pair_field, n_fields, ring_offsets, n_rings, vert_offsets, n_verts, x, y);
    if (rc) return rc;
    std::vector<int64_t> rings, verts;
    rc = swath_fields(nullptr, n_fields, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    if (field_status) WorkerPool::parallel_for(n_fields, [&](int64_t f) { field_status[f] = clear_field_status(F, f); });
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const ClearResult r = mode == 0 ? clear_path<0>(F, pair_field[i], from_x[i], from_y[i], from_h[i], radius, word[i], seg + 3 * i)
                                        : clear_path<1>(F, pair_field[i], from_x[i], from_y[i], from_h[i], radius, word[i], seg + 5 * i);
        store(crossings, i, r.crossings); store(inside, i, r.inside); store(first_s, i, r.first_s);
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
    DevBuf<int64_t> list;
    DevBuf<unsigned long long> count;
    if (n > 0 && (word || seg || len || rank || crossings)) {
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
    }
    HIPCHK(hipStreamSynchronize(c->stream));          // (the list dies here)
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
    rc = swath_fields(nullptr, n_fields, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    if (field_status) WorkerPool::parallel_for(n_fields, [&](int64_t f) { field_status[f] = clear_field_status(F, f); });
    const int nseg = mode == 0 ? 3 : 5;
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const SolveClearResult r = mode == 0 ? solve_clear<0>(F, pair_field[i], from_x[i], from_y[i], from_h[i], to_x[i], to_y[i], to_h[i], radius)
                                             : solve_clear<1>(F, pair_field[i], from_x[i], from_y[i], from_h[i], to_x[i], to_y[i], to_h[i], radius);
        store(word, i, r.word);
        if (seg)
            for (int k = 0; k < nseg; ++k) seg[i * nseg + k] = r.seg[k];
        store(len, i, r.len); store(rank, i, r.rank); store(crossings, i, r.crossings);
    });
    return FCPP_OK;
}

}  // extern "C"
