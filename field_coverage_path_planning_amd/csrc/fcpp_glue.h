// fcpp_glue.h -- what the glue files of the standalone path operators (fcpp_paths.cpp, fcpp_glue_*.cpp) share: the host-table reader and
// the CSR checks layered on it, the small named rules, the *_counts / *_sample skeletons.  Like fcpp_api.cpp, a glue file is argument checking,
// device buffers and launches; every operator but the small stateless ones drains the context's stream before it returns.  Private to csrc/.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "fcpp_api_internal.h"
#include "fcpp_swathfn.h"

namespace fcpp {
namespace {      // (every glue file its own copy: nothing here is exported)
// ---- the host-table reader --------------------------------------------------------------------------------------------------------------
// m values of type T on the host, in `out`: the caller's host copy if given, else one asynchronous copy from the device plus one
// synchronisation on the context's stream (none for a host copy or an empty table).  With no context (the fcpp_debug_* twins) `ptr` is
// a host pointer.  host_copy_async is the copy alone, into the caller's storage: for a caller that reads two tables behind one synchronisation.
template <class T>
int host_copy_async(fcpp_ctx *c, int64_t m, const T *ptr, const T *host, T *out)
{
    if (m <= 0) return FCPP_OK;
    if (host || !c) memcpy((void *)out, host ? host : ptr, (size_t)m * sizeof(T));
    else HIPCHK(hipMemcpyAsync((void *)out, ptr, (size_t)m * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return FCPP_OK;
}

template <class T>
int host_table(fcpp_ctx *c, int64_t m, const T *ptr, const T *host, std::vector<T> &out)
{
    try { out.assign((size_t)std::max<int64_t>(m, 0), T()); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    const int rc = host_copy_async(c, m, ptr, host, out.data());
    if (rc) return rc;
    if (c && !host && m > 0) HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

// the ends of a device offsets table of n + 1 entries, on the host: a copy per end asked for (`first` may be NULL), one synchronisation
int table_ends(fcpp_ctx *c, const int64_t *dev, int64_t n, int64_t *first, int64_t *last)
{
    if (first) HIPCHK(hipMemcpyAsync(first, dev, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(last, dev + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

// ---- CSR checks of a table on the host (n + 1 entries), in the two wordings the entries use --------------------------------------------------
// `head` fails first with `head_text`, then the order: "<what> must be non-decreasing"
int csr_check(const std::vector<int64_t> &t, int64_t n, bool head, const char *what, const char *head_text)
{
    if (!head) return fail(FCPP_ESIZE, std::string(what) + head_text);
    for (int64_t p = 0; p < n; ++p)
        if (t[(size_t)p + 1] < t[(size_t)p]) return fail(FCPP_ESIZE, std::string(what) + " must be non-decreasing");
    return FCPP_OK;
}

// both ends at once, then the order ...
int csr_spans(const std::vector<int64_t> &t, int64_t n, int64_t total, const char *what)
{
    return csr_check(t, n, t[0] == 0 && t.back() == total, what, " do not span [0, total]");
}

// ... or the start, then the order; what the end must be is the caller's, in its words
int csr_ordered(const std::vector<int64_t> &t, int64_t n, const char *what) { return csr_check(t, n, t[0] == 0, what, " must start at 0"); }

// CSR offsets of n rows on the host, read and checked to span [0, total]
int host_offsets(fcpp_ctx *c, int64_t n, const int64_t *ptr, const int64_t *host, int64_t total, const char *what, std::vector<int64_t> &out)
{
    const int rc = host_table(c, n + 1, ptr, host, out);
    return rc ? rc : csr_spans(out, n, total, what);
}

// the two CSR levels of the fields (rings of a field, vertices of a ring), read and checked
int swath_fields(fcpp_ctx *c, int64_t n, const int64_t *ring_ptr, const int64_t *ring_host, int64_t n_rings, const int64_t *vert_ptr,
                 const int64_t *vert_host, int64_t n_verts, std::vector<int64_t> &rings, std::vector<int64_t> &verts)
{
    int rc = host_offsets(c, n, ring_ptr, ring_host, n_rings, "ring_offsets", rings);
    if (rc == FCPP_OK) rc = host_offsets(c, n_rings, vert_ptr, vert_host, n_verts, "vert_offsets", verts);
    return rc;
}

// the swath offsets and the router's block offsets on the host, checked against each other: block i holds (2 m_i)^2 entries, none beyond
// FCPP_ROUTE_MAX_SWATHS (route_block of fcpp_routefn.h); what the router's entries and the service trips check alike
int route_offsets(fcpp_ctx *c, int64_t n, const int64_t *soff_ptr, const int64_t *soff_host, int64_t n_total, const int64_t *toff_ptr,
                  const int64_t *toff_host, int64_t t_total, std::vector<int64_t> &soff, std::vector<int64_t> &toff)
{
    if (n < 0 || n_total < 0 || t_total < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    int rc = host_offsets(c, n, soff_ptr, soff_host, n_total, "swath_offsets", soff);
    if (rc == FCPP_OK) rc = host_offsets(c, n, toff_ptr, toff_host, t_total, "t_offsets", toff);
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t m = soff[(size_t)i + 1] - soff[(size_t)i];
        if (toff[(size_t)i + 1] - toff[(size_t)i] != (m > FCPP_ROUTE_MAX_SWATHS ? 0 : 4 * m * m))
            return fail(FCPP_ESIZE, "t_offsets do not match the swath counts: block i holds (2 m_i)^2 entries, none for m_i > 512");
    }
    return FCPP_OK;
}

// m angles on the host, read and checked: finite and within fc_sincos' range, or FCPP_EINVAL in the entry's words
int host_angles(fcpp_ctx *c, int64_t m, const double *ptr, const double *host, const char *text, std::vector<double> &th)
{
    const int rc = host_table(c, m, ptr, host, th);
    if (rc) return rc;
    for (int64_t j = 0; j < m; ++j)
        if (!(fabs(th[(size_t)j]) <= SWATH_MAX_ANGLE)) return fail(FCPP_EINVAL, text);
    return FCPP_OK;
}

int swath_angles(fcpp_ctx *c, int64_t m, const double *ptr, const double *host)
{
    std::vector<double> th;
    return host_angles(c, m, ptr, host, "angles must be finite, |angle| <= 1e5", th);
}

// ---- the small rules -------------------------------------------------------------------------------------------------------------------------
int positive_finite(double v, const char *name)
{
    if (!(v > 0.0) || !isfinite(v)) return fail(FCPP_EINVAL, std::string(name) + " must be positive and finite");
    return FCPP_OK;
}

int route_radius(double radius, int mode)
{
    const int rc = positive_finite(radius, "radius");
    if (rc) return rc;
    if (mode != 0 && mode != 1) return fail(FCPP_EINVAL, "mode must be 0 (Dubins) or 1 (Reeds-Shepp)");
    return FCPP_OK;
}

// what the clear connectors (fcpp_glue_conn.cpp) and the loop transits (fcpp_glue_legs.cpp) check alike of their pairs and their fields
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

// an optional output of a host twin: written where the caller asked for it
template <class T, class V>
void store(T *out, int64_t at, V v) { if (out) out[at] = (T)v; }

// a striding kernel's launch: workgroups per compute unit of the context's device
int blocks_per_cu(const fcpp_ctx *c) { return 4 * (c->n_cu > 0 ? c->n_cu : 64); }

// ---- the fixed-step samplers (fcpp_samplefn.h): what the *_counts / *_sample entries share (the count rule itself: fcpp_connfn.h) -----------------
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
}  // namespace
}  // namespace fcpp
