// fcpp_swath.hip -- gfx950 (MI355X) kernels of the polygon swaths: k_swath_count (n fields x A angles: swath count, line count and length
// sum of every pair -- the angle search, and with A = 1 the counting pass of the cut) and k_swath_fill (the swath records at the CSR offsets
// the project's workgroup scan made of the counts).  The rule is ONE set of host+device expressions, fcpp_swathfn.h; float64,
// -ffp-contract=off like every other translation unit, so the kernels give the bits fcpp_debug_swaths gives on the host.
//
// Mapping.  A workgroup is ONE wavefront and takes a (field, angle) pair; it walks the field's lines 64 at a time, a lane per line.  The
// field's vertices are rotated into the track frame 64 at a time, a lane per vertex, and stay in REGISTERS: the edge all lanes look at is two
// v_readlane broadcasts of (u, w) into scalar registers, so the edge stream needs neither LDS nor a barrier and the vertex count has no cap
// (a chunk is 63 edges: its last vertex is the next chunk's first, evaluated again by the same expression, hence the same bits).  A lane
// tests the edge against its own line (two compares) and, on a crossing, inserts u into ITS column of an LDS table -- slot-major,
// tab[slot * 64 + lane], so the lanes of a wavefront hit 64 consecutive doubles whatever slot each is at: conflict-free, and no per-lane array
// indexed at run time (which would be scratch).  64 slots x 64 lanes x 8 B = 32 KiB per wavefront: four wavefronts per CU, one per SIMD.
// That is the price of the cap of 64 crossings; what runs at that occupancy is the edge loop -- scalar broadcasts and two fp64 compares per
// edge and lane, LDS only on a crossing -- not an LDS read stream.  After a block of lines every lane pairs its column in order.
// length: a lane adds the swaths of its lines in order, then the fixed xor butterfly over the wavefront (fcpp_swathfn.h states the order).
// Before the lines one pass over the vertices gives w_min / w_max (exact in any order) and the field's validity.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_samplefn.h"
#include "fcpp_swath.h"
#include "fcpp_swathfn.h"

namespace fcpp {

static constexpr int SWAVE = 64;            // the workgroup: one wavefront
static constexpr int SCHUNK = SWAVE - 1;    // edges per vertex chunk
static constexpr int SBLOCK = 256;          // the offsets scan

// lane `from` (uniform) of v, in every lane
__device__ __forceinline__ double swath_bcast(double v, int from)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), from), hi = __builtin_amdgcn_readlane(__double2hiint(v), from);
    return __hiloint2double(hi, lo);
}

// One (field, angle) pair by one wavefront.  FILL: also the records, from offsets[i] on and never at or beyond offsets[i + 1].
template <bool FILL>
__device__ __forceinline__ SwathTotals swath_wave(double *tab, int64_t i, double theta, const int64_t *__restrict__ ring_offsets,
                                                  const int64_t *__restrict__ vert_offsets, const double *__restrict__ x,
                                                  const double *__restrict__ y, double W, double first, double min_length, int64_t out0,
                                                  int64_t out1, double *__restrict__ ax, double *__restrict__ ay, double *__restrict__ bx,
                                                  double *__restrict__ by, int32_t *__restrict__ line, double *__restrict__ length)
{
    const SwathTotals invalid = { SWATH_EINVAL, 0, 0, 0.0 }, unsupported = { SWATH_EUNSUPPORTED, 0, 0, 0.0 };
    const int lane = threadIdx.x;
    const int64_t r0 = ring_offsets[i], r1 = ring_offsets[i + 1];
    if (r1 <= r0) return invalid;
    const int64_t v0 = vert_offsets[r0], v1 = vert_offsets[r1];
    double s, c;
    fc_sincos(theta, s, c);
    // validity, w_min and w_max
    bool bad = false;
    for (int64_t r = r0 + lane; r < r1; r += SWAVE) bad |= vert_offsets[r + 1] - vert_offsets[r] < 3;
    double w_min = INFINITY, w_max = -INFINITY;
    for (int64_t v = v0 + lane; v < v1; v += SWAVE) {
        double u, w;
        swath_uw(x[v], y[v], c, s, u, w);
        bad |= !swath_finite(x[v]) || !swath_finite(y[v]) || !swath_finite(u) || !swath_finite(w);
        w_min = fmin(w_min, w);
        w_max = fmax(w_max, w);
    }
    if (__any(bad)) return invalid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        w_min = fmin(w_min, __shfl_xor(w_min, o));
        w_max = fmax(w_max, __shfl_xor(w_max, o));
    }
    const int64_t K = swath_n_lines(w_min, w_max, first, W);
    if (K > SWATH_MAX_LINES) return unsupported;
    const double base = w_min + first;
    double *col = tab + lane;
    double acc = 0.0;
    int n_sw = 0;
    int64_t done = 0;                 // FILL: records of the blocks before this one
    for (int64_t k0 = 0; k0 < K; k0 += SWAVE) {
        const int64_t k = k0 + lane;
        const double wk = k < K ? swath_line_w(base, W, k) : __builtin_nan("");      // (a NaN line crosses nothing)
        int cnt = 0;
        bool over = false;
        for (int64_t r = r0; r < r1; ++r) {
            const int64_t a = vert_offsets[r], b = vert_offsets[r + 1];
            for (int64_t c0 = a; c0 < b; c0 += SCHUNK) {
                const int m = (int)(b - c0 < SCHUNK ? b - c0 : SCHUNK);      // edges of this chunk: lanes 0 .. m hold their vertices
                int64_t vi = c0 + lane;
                if (vi >= b) vi = a;                                           // (the ring closes; idle lanes read a valid vertex)
                double ul, wl;
                swath_uw(x[vi], y[vi], c, s, ul, wl);
                double up = swath_bcast(ul, 0), wp = swath_bcast(wl, 0);
                for (int e = 0; e < m; ++e) {
                    const double uq = swath_bcast(ul, e + 1), wq = swath_bcast(wl, e + 1);
                    if (swath_crosses(wp, wq, wk)) {
                        if (cnt == SWATH_MAX_CROSSINGS) over = true;
                        else { swath_insert(col, SWAVE, cnt, swath_cross_u(up, wp, uq, wq, wk)); ++cnt; }
                    }
                    up = uq; wp = wq;
                }
            }
        }
        if (__any(over)) return unsupported;
        int kept = 0;
        for (int j = 0; j + 1 < cnt; j += 2) {
            const double len = col[(j + 1) * SWAVE] - col[j * SWAVE];
            if (!(len > min_length)) continue;
            acc += len;
            ++kept;
        }
        n_sw += kept;
        if (FILL) {
            int inc = kept;
#pragma unroll
            for (int o = 1; o < SWAVE; o <<= 1) {
                const int pv = __shfl_up(inc, o);
                if (lane >= o) inc += pv;
            }
            int64_t at = out0 + done + (inc - kept);
            done += __shfl(inc, SWAVE - 1);
            for (int j = 0; j + 1 < cnt; j += 2) {
                const double ua = col[j * SWAVE], ub = col[(j + 1) * SWAVE], len = ub - ua;
                if (!(len > min_length)) continue;
                if (at >= out0 && at < out1) {
                    double px, py, qx, qy;
                    swath_point(ua, wk, c, s, px, py);
                    swath_point(ub, wk, c, s, qx, qy);
                    if (ax) ax[at] = px;
                    if (ay) ay[at] = py;
                    if (bx) bx[at] = qx;
                    if (by) by[at] = qy;
                    if (line) line[at] = (int32_t)k;
                    if (length) length[at] = len;
                }
                ++at;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o);
        n_sw += __shfl_xor(n_sw, o);
    }
    return { SWATH_OK, (int32_t)K, n_sw, acc };
}

__global__ __launch_bounds__(SWAVE) void k_swath_count(int64_t A, int per_field, const int64_t *__restrict__ ring_offsets,
                                                       const int64_t *__restrict__ vert_offsets, const double *__restrict__ x,
                                                       const double *__restrict__ y, const double *__restrict__ angles, double W, double first,
                                                       double min_length, int32_t *__restrict__ n_swaths, int32_t *__restrict__ n_lines,
                                                       double *__restrict__ length, int32_t *__restrict__ status)
{
    __shared__ double tab[SWATH_MAX_CROSSINGS * SWAVE];
    const int64_t pair = blockIdx.x, i = pair / A, j = pair - i * A;
    const SwathTotals t = swath_wave<false>(tab, i, angles[per_field ? i : j], ring_offsets, vert_offsets, x, y, W, first, min_length, 0, 0,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (threadIdx.x != 0) return;
    if (n_swaths) n_swaths[pair] = t.n_swaths;
    if (n_lines) n_lines[pair] = t.n_lines;
    if (length) length[pair] = t.length;
    if (status) status[pair] = t.status;
}

__global__ __launch_bounds__(SWAVE) void k_swath_fill(const int64_t *__restrict__ ring_offsets, const int64_t *__restrict__ vert_offsets,
                                                      const double *__restrict__ x, const double *__restrict__ y,
                                                      const double *__restrict__ angles, double W, double first, double min_length,
                                                      const int64_t *__restrict__ offsets, double *__restrict__ ax, double *__restrict__ ay,
                                                      double *__restrict__ bx, double *__restrict__ by, int32_t *__restrict__ line,
                                                      double *__restrict__ length)
{
    __shared__ double tab[SWATH_MAX_CROSSINGS * SWAVE];
    const int64_t i = blockIdx.x, out0 = offsets[i], out1 = offsets[i + 1];
    if (out1 <= out0) return;                  // no swaths: an empty field, or one with a status
    (void)swath_wave<true>(tab, i, angles[i], ring_offsets, vert_offsets, x, y, W, first, min_length, out0, out1, ax, ay, bx, by, line, length);
}

// the count of field p for the workgroup scan of fcpp_samplefn.h
struct SwathCount {
    const int32_t *n_swaths;
    __device__ int64_t operator()(int64_t p, int64_t &) const { return n_swaths[p]; }
};

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_swath_count(hipStream_t st, int64_t n, int64_t A, int per_field, const int64_t *ring_offsets, const int64_t *vert_offsets,
                       const double *x, const double *y, const double *angles, double W, double first, double min_length, int32_t *n_swaths,
                       int32_t *n_lines, double *length, int32_t *status)
{
    if (n <= 0 || A <= 0) return 0;
    return launch(st, k_swath_count, (unsigned)(n * A), SWAVE, A, per_field, ring_offsets, vert_offsets, x, y, angles, W, first, min_length, n_swaths,
                  n_lines, length, status);
}

int launch_swath_offsets(hipStream_t st, int64_t n, const int32_t *n_swaths, int64_t *out_offsets, int64_t *err)
{
    return launch_path_counts<SBLOCK>(st, n, SwathCount{ n_swaths }, out_offsets, err);
}

int launch_swath_fill(hipStream_t st, int64_t n, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x, const double *y,
                      const double *angles, double W, double first, double min_length, const int64_t *offsets, double *ax, double *ay, double *bx,
                      double *by, int32_t *line, double *length)
{
    if (n <= 0) return 0;
    return launch(st, k_swath_fill, (unsigned)n, SWAVE, ring_offsets, vert_offsets, x, y, angles, W, first, min_length, offsets, ax, ay, bx, by, line,
                  length);
}

}  // namespace fcpp
