// fcpp_pcoverfn.h -- the coverage report of ANY polygon field: which cells of a field's grid lie inside the field, which the working passes of
// a sampled path set cover, which two different passes cover, and which are covered outside the field.  ONE set of expressions for the host
// (fcpp_debug_polygon_cover, the tests' checker) and the device (fcpp_pcover.hip), written like fcpp_swathfn.h / fcpp_hpathfn.h in plain
// IEEE-754 double operations and compiled with -ffp-contract=off on both sides, so that both give the same bits.  Build-defined: the
// reference's coverage rate reads four corners.
//
// THE RULE (include/fcpp.h states it for callers).
//   fields    the two-level CSR of the swath operators (ring_offsets, vert_offsets, x, y), even-odd interior: the SURVEYED boundaries.
//             FCPP_EINVAL as there: no ring, a ring with fewer than 3 vertices, a vertex that is not finite.
//   grid      r = W / 2, m = ceil(r / res) margin cells; gx = x_min - m res, gy = y_min - m res; nx = ceil((x_max - x_min) / res) + 2 m, ny
//             likewise; cell (a, b) is sampled at (gx + ((double)a + 0.5) res, gy + ((double)b + 0.5) res) (pcover_cell: fcpp_cover_grid's
//             expression with shift 0.5).  More than 2^28 cells: FCPP_EUNSUPPORTED.  A failed field has an empty grid and zero counts.
//   inside    a cell is inside iff an odd number of edges cross its row at u < X: swath_crosses / swath_cross_u of fcpp_swathfn.h in the frame
//             theta = 0 (u = x, w = y through swath_uw with c = 1, s = 0) -- half-open, so a row through a vertex counts consistently.
//   working   segment (k, k + 1) of a path works iff both samples work (work[k] != 0; no mask: all do) and both are finite; its pass is
//             pass[k] (no array: the path's index).  An end of a working segment is a JOINT iff the neighbouring segment of the same path on
//             that side works too.
//   covered   with a -> b the segment, p the cell, dot = (p - a).(b - a), len2 = |b - a|^2, cross = (b - a) x (p - a):
//                 0 < dot < len2 : cross^2 < r^2 len2
//                 dot <= 0       : a joint (or caps = 1): |p - a|^2 < r^2;  a flat end: dot == 0 and cross^2 < r^2 len2
//                 dot >= len2    : b joint (or caps = 1): |p - b|^2 < r^2;  a flat end: dot == len2 and cross^2 < r^2 len2
//             -- the three-way partition of fcpp_cover_grid with the strict comparison; with every end round it IS that predicate.  A run of
//             working segments sweeps a rectangle with rounded interior joints.
//   overlap   a cell is overlapped iff working segments of at least two different pass ids cover it (the first covering id and a flag:
//             independent of the order of the segments).
//   outputs   counts (4 per field): cells inside; inside and covered; inside and overlapped; covered and not inside.  grid (optional): one
//             byte per cell, row-major, bit 0 inside, bit 1 covered, bit 2 overlapped.
// Every culling step (a segment's box against a row of cells, a chunk's box against a tile) is CONSERVATIVE: it may keep what cannot cover and
// never drops what can, so host and device, which cull differently, agree in every bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_math.h"
#include "fcpp_swathfn.h"

namespace fcpp {

constexpr int PCOVER_OK = 0, PCOVER_EINVAL = -1, PCOVER_EUNSUPPORTED = -3;      // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED
constexpr int64_t PCOVER_MAX_CELLS = (int64_t)1 << 28;
constexpr int PCOVER_CHUNK = 256;          // segments per chunk of a path (one bounding box each)
constexpr int PCOVER_TILE = 64;            // tile edge in cells

struct PcoverDims {        // fcpp_polygon_cover_sizes' record per field: 32 bytes
    double gx, gy;
    int64_t nx, ny;
};

FCPP_HD double pcover_cell(double g, int64_t a, double res) { return g + ((double)a + 0.5) * res; }

// the culling distance of a segment: k_cover's (culling must never drop a covering segment)
FCPP_HD double pcover_reach(double r) { return r * (1.0 + 1e-9) + 1e-9; }

// the grid of a field with the finite bounding box [x_min, x_max] x [y_min, y_max]: PCOVER_OK or PCOVER_EUNSUPPORTED (then d is empty)
FCPP_HD int pcover_dims(double x_min, double x_max, double y_min, double y_max, double W, double res, PcoverDims &d)
{
    const double r = W / 2.0, m = ceil(r / res);
    const double fx = ceil((x_max - x_min) / res) + 2.0 * m, fy = ceil((y_max - y_min) / res) + 2.0 * m;
    d.gx = 0.0; d.gy = 0.0; d.nx = 0; d.ny = 0;
    if (!(fx <= (double)PCOVER_MAX_CELLS) || !(fy <= (double)PCOVER_MAX_CELLS) || !(fx * fy <= (double)PCOVER_MAX_CELLS)) return PCOVER_EUNSUPPORTED;
    d.gx = x_min - m * res;
    d.gy = y_min - m * res;
    d.nx = (int64_t)fx;
    d.ny = (int64_t)fy;
    return PCOVER_OK;
}

// does the edge (px, py) -> (qx, qy) cross the row Y left of X?  (the half-open rule of the swaths at theta = 0)
FCPP_HD bool pcover_edge_left(double px, double py, double qx, double qy, double X, double Y)
{
    double up, wp, uq, wq;
    swath_uw(px, py, 1.0, 0.0, up, wp);
    swath_uw(qx, qy, 1.0, 0.0, uq, wq);
    if (!swath_crosses(wp, wq, Y)) return false;
    return swath_cross_u(up, wp, uq, wq, Y) < X;
}

// the same on an edge already in the frame (the kernels stage (u, w) pairs)
FCPP_HD bool pcover_edge_left_uw(double up, double wp, double uq, double wq, double X, double Y)
{
    if (!swath_crosses(wp, wq, Y)) return false;
    return swath_cross_u(up, wp, uq, wq, Y) < X;
}

// ja / jb: the end at a / b is round (a joint, or caps = 1)
FCPP_HD bool pcover_covers(double ax, double ay, double bx, double by, double X, double Y, double r2, bool ja, bool jb)
{
    const double abx = bx - ax, aby = by - ay, apx = X - ax, apy = Y - ay;
    const double len2 = abx * abx + aby * aby, dot = apx * abx + apy * aby;
    if (dot <= 0.0) {
        if (ja) return apx * apx + apy * apy < r2;
        if (dot != 0.0) return false;
    } else if (dot >= len2) {
        if (jb) { const double bpx = X - bx, bpy = Y - by; return bpx * bpx + bpy * bpy < r2; }
        if (dot != len2) return false;
    }
    const double cr = abx * apy - aby * apx;
    return cr * cr < r2 * len2;
}

// the paths of a call (host or device pointers): work and pass may be NULL
struct PcoverPaths {
    const double *x, *y;
    const uint8_t *work;
    const int32_t *pass;
};

// does sample k take part in working segments?
FCPP_HD bool pcover_sample_ok(const PcoverPaths &P, int64_t k)
{
    return (!P.work || P.work[k] != 0) && swath_finite(P.x[k]) && swath_finite(P.y[k]);
}

// segment (k, k + 1) of the path [p0, p1) (p0 <= k, k + 1 < p1): false if it does not work; else its ends, its pass and the two round flags
FCPP_HD bool pcover_segment(const PcoverPaths &P, int64_t path, int64_t p0, int64_t p1, int64_t k, int caps, double &ax, double &ay, double &bx,
                            double &by, int32_t &pass, bool &ja, bool &jb)
{
    if (!pcover_sample_ok(P, k) || !pcover_sample_ok(P, k + 1)) return false;
    ax = P.x[k]; ay = P.y[k]; bx = P.x[k + 1]; by = P.y[k + 1];
    pass = P.pass ? P.pass[k] : (int32_t)path;
    ja = caps != 0 || (k - 1 >= p0 && pcover_sample_ok(P, k - 1));
    jb = caps != 0 || (k + 2 < p1 && pcover_sample_ok(P, k + 2));
    return true;
}

// one cell's state under one covering segment: bit 1 covered, bit 2 overlapped (the grid's bits); `first` the first covering pass
FCPP_HD void pcover_mark(uint8_t &bits, int32_t &first, int32_t pass)
{
    if (!(bits & 2)) { bits |= 2; first = pass; }
    else if (first != pass) bits |= 4;
}

// ---- the rule on the host, field by field ------------------------------------------------------------------------------------------------
// a field's status and grid (rings r0 .. r1 of vert_offsets)
inline int pcover_field_dims_host(const int64_t *vert_offsets, int64_t r0, int64_t r1, const double *x, const double *y, double W, double res,
                                  PcoverDims &d)
{
    d.gx = 0.0; d.gy = 0.0; d.nx = 0; d.ny = 0;
    if (r1 <= r0) return PCOVER_EINVAL;
    for (int64_t r = r0; r < r1; ++r)
        if (vert_offsets[r + 1] - vert_offsets[r] < 3) return PCOVER_EINVAL;
    double x_min = INFINITY, x_max = -INFINITY, y_min = INFINITY, y_max = -INFINITY;
    for (int64_t v = vert_offsets[r0]; v < vert_offsets[r1]; ++v) {
        if (!swath_finite(x[v]) || !swath_finite(y[v])) return PCOVER_EINVAL;
        if (x[v] < x_min) x_min = x[v];
        if (x[v] > x_max) x_max = x[v];
        if (y[v] < y_min) y_min = y[v];
        if (y[v] > y_max) y_max = y[v];
    }
    return pcover_dims(x_min, x_max, y_min, y_max, W, res, d);
}

// index range [lo, hi] of the cells of one axis whose sample may lie within `reach` of [v0, v1]: two cells wider than the arithmetic asks for
inline void pcover_cell_range(double g, double res, int64_t n, double v0, double v1, double reach, int64_t &lo, int64_t &hi)
{
    const double a = floor((v0 - reach - g) / res - 0.5) - 2.0, b = ceil((v1 + reach - g) / res - 0.5) + 2.0;
    lo = a > 0.0 ? (a < (double)n ? (int64_t)a : n) : 0;
    hi = b < (double)(n - 1) ? (b >= 0.0 ? (int64_t)b : -1) : n - 1;
}

// One good field (d from pcover_field_dims_host, d.nx d.ny cells): bits (one byte per cell) and first (one int32 per cell) are the caller's
// scratch, bits ends as the grid's bytes; the field's paths are path_ids[s0 .. s1) (path_ids NULL: s itself) of path_offsets; counts[4].
inline void pcover_field_host(const int64_t *vert_offsets, int64_t r0, int64_t r1, const double *x, const double *y, const PcoverDims &d, double W,
                              double res, int caps, const int64_t *path_offsets, const PcoverPaths &P, const int64_t *path_ids, int64_t s0,
                              int64_t s1, uint8_t *bits, int32_t *first, double *cross, int64_t counts[4])
{
    const int64_t nx = d.nx, ny = d.ny;
    const double r = W / 2.0, r2 = r * r, reach = pcover_reach(r);
    // inside: per row the crossings' u, then every cell counts those left of it
    for (int64_t b = 0; b < ny; ++b) {
        const double Y = pcover_cell(d.gy, b, res);
        int64_t nc = 0;
        for (int64_t rg = r0; rg < r1; ++rg) {
            const int64_t v0 = vert_offsets[rg], m = vert_offsets[rg + 1] - v0;
            for (int64_t e = 0; e < m; ++e) {
                const int64_t p = v0 + e, q = v0 + (e + 1 == m ? 0 : e + 1);
                double up, wp, uq, wq;
                swath_uw(x[p], y[p], 1.0, 0.0, up, wp);
                swath_uw(x[q], y[q], 1.0, 0.0, uq, wq);
                if (swath_crosses(wp, wq, Y)) cross[nc++] = swath_cross_u(up, wp, uq, wq, Y);
            }
        }
        for (int64_t a = 0; a < nx; ++a) {
            const double X = pcover_cell(d.gx, a, res);
            int odd = 0;
            for (int64_t k = 0; k < nc; ++k) odd ^= cross[k] < X ? 1 : 0;
            bits[b * nx + a] = (uint8_t)odd;
            first[b * nx + a] = 0;
        }
    }
    // covered, overlapped: every working segment over the cells its box may reach
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t path = path_ids ? path_ids[s] : s, p0 = path_offsets[path], p1 = path_offsets[path + 1];
        for (int64_t k = p0; k + 1 < p1; ++k) {
            double ax, ay, bx, by;
            int32_t pass;
            bool ja, jb;
            if (!pcover_segment(P, path, p0, p1, k, caps, ax, ay, bx, by, pass, ja, jb)) continue;
            int64_t a0, a1, b0, b1;
            pcover_cell_range(d.gx, res, nx, fmin(ax, bx), fmax(ax, bx), reach, a0, a1);
            pcover_cell_range(d.gy, res, ny, fmin(ay, by), fmax(ay, by), reach, b0, b1);
            for (int64_t b = b0; b <= b1; ++b) {
                const double Y = pcover_cell(d.gy, b, res);
                for (int64_t a = a0; a <= a1; ++a)
                    if (pcover_covers(ax, ay, bx, by, pcover_cell(d.gx, a, res), Y, r2, ja, jb)) pcover_mark(bits[b * nx + a], first[b * nx + a], pass);
            }
        }
    }
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int64_t c = 0; c < nx * ny; ++c) {
        const uint8_t v = bits[c];
        counts[0] += v & 1;
        counts[1] += (v & 3) == 3;
        counts[2] += (v & 5) == 5;
        counts[3] += (v & 3) == 2;
    }
}

}  // namespace fcpp
