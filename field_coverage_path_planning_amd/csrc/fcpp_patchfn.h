// fcpp_patchfn.h -- patch passes: straight working passes over the member cells of coverage regions (the missed patches
// fcpp_cover_regions_fill labels), parallel to the field's tracks.  ONE set of expressions for the host (fcpp_debug_patch_swaths, the
// tests' checker) and the device (fcpp_patch.hip).  The extents are exact min / max, everything behind the two `floor`s of a member is
// integer work: the result is a function of the input alone, whatever the order of work.  Plain C++: g++ compiles it as it is.
//
// THE RULE (include/fcpp.h states it for callers).
//   input     the grids as fcpp_polygon_cover writes them (dims, cell_offsets, res); labels, int32 per cell: a value >= 0 is the cell's
//             region index within its field, any negative value is no member; region_offsets (n + 1); one track angle theta per field;
//             width W, margin m (0 <= m, We = W - 2 m > 0), join j >= 0.
//   frame     (s, c) = fc_sincos(theta).  Cell (a, b) has the GRID-LOCAL centre x = ((double)a + 0.5) res, y = ((double)b + 0.5) res
//             (patch_cell_uw; the grid origin is added only at the output), (u, w) = swath_uw(x, y, c, s).
//   extent    per region u_min, u_max, w_min, w_max over its members (patch_key: an order-preserving integer key of a double, so the
//             device's integer atomic max of the keys of -u, u, -w, w is the exact extent, -0 below +0).
//   lines     K = floor((w_max - w_min) / We) + 1,  w_lo = w_min - (fl(K We) - (w_max - w_min)) / 2,  line k at
//             w_k = w_lo + ((double)k + 0.5) We (patch_line_w); a member belongs to line clamp(floor((w - w_lo) / We), 0, K - 1).
//   bins      h = res, B = floor((u_max - u_min) / h) + 1, a member falls in bin clamp(floor((u - u_min) / h), 0, B - 1); bit
//             (region, k, q) is set iff some member falls there: line k of a region is ceil(B / 64) words of 64 bins.
//   runs      J = floor(j / h); a set bin q starts a run iff none of the bins q - J - 1 .. q - 1 is set; a run ends at the last set bin
//             before the next start, or at the line's last set bin (patch_line_runs).
//   swath     of a run q0 .. q1 on line k: u_a = u_min + (double)q0 h - m, u_b = u_min + (double)(q1 + 1) h + m, the end points
//             swath_point(u, w_k, c, s) + (gx, gy), length u_b - u_a.  Order within a field: by region, then k, then u.
//   status    per region FCPP_EUNSUPPORTED for K > 2^22 or K ceil(B / 64) >= 2^31: no lines, no swaths.  A region without members
//             (its label never occurs) has no lines and status 0.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "fcpp_geom.h"
#include "fcpp_math.h"
#include "fcpp_regionfn.h"
#include "fcpp_swathfn.h"

namespace fcpp {

constexpr int64_t PATCH_MAX_LINES = (int64_t)1 << 22;           // per region (SWATH_MAX_LINES)
constexpr int64_t PATCH_MAX_WORDS = (int64_t)1 << 31;           // per region: K ceil(B / 64) stays below
constexpr int64_t PATCH_MAX_JOIN_BINS = (int64_t)1 << 40;       // J is clamped here: above every supported B (a larger B is unsupported unseen)
constexpr int PATCH_OK = 0, PATCH_EUNSUPPORTED = -3;            // FCPP_OK / FCPP_EUNSUPPORTED

struct PatchRecord {        // 64 bytes per region; between the extent and the layout its first four words hold the keys of -u, u, -w, w
    double u_min, w_lo;
    int64_t K, B;
    int64_t first_line, first_word;     // the lines / bitmap words of all earlier regions of the call
    int32_t status, zero;
    double u_max;
};
static_assert(sizeof(PatchRecord) == 64, "the patch record is 64 bytes");

FCPP_HD bool patch_args_ok(double res, double W, double m, double join)
{
    return swath_finite(res) && res > 0.0 && swath_finite(W) && swath_finite(m) && swath_finite(join) && m >= 0.0 && W - 2.0 * m > 0.0 && join >= 0.0;
}

FCPP_HD bool patch_angle_ok(double theta) { return fabs(theta) <= SWATH_MAX_ANGLE; }          // false for NaN

// an integer key that orders as the doubles do (-0 below +0); no double has key 0, which stands for "no member yet"
FCPP_HD uint64_t patch_key(double v)
{
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

FCPP_HD double patch_unkey(uint64_t k)
{
    const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

FCPP_HD void patch_cell_uw(int64_t a, int64_t b, double res, double c, double s, double &u, double &w)
{
    const double x = ((double)a + 0.5) * res, y = ((double)b + 0.5) * res;
    swath_uw(x, y, c, s, u, w);
}

// the layout of a region from the keys of its extent (max of -u, u, -w, w; 0: no member): everything of the record but its place in the call
FCPP_HD PatchRecord patch_layout(uint64_t key_nu, uint64_t key_u, uint64_t key_nw, uint64_t key_w, double We, double h)
{
    PatchRecord r = { 0.0, 0.0, 0, 0, 0, 0, PATCH_OK, 0, 0.0 };
    if (key_u == 0) return r;
    const double u_min = -patch_unkey(key_nu), u_max = patch_unkey(key_u), w_min = -patch_unkey(key_nw), w_max = patch_unkey(key_w);
    r.u_min = u_min; r.u_max = u_max;
    const double span = w_max - w_min;
    const double Kd = floor(span / We) + 1.0, Bd = floor((u_max - u_min) / h) + 1.0;
    if (!(Kd <= (double)PATCH_MAX_LINES) || !(Bd <= (double)PATCH_MAX_JOIN_BINS)) { r.status = PATCH_EUNSUPPORTED; return r; }
    const int64_t K = (int64_t)Kd, B = (int64_t)Bd;
    if (K * ((B + 63) / 64) >= PATCH_MAX_WORDS) { r.status = PATCH_EUNSUPPORTED; return r; }
    r.K = K; r.B = B;
    r.w_lo = w_min - ((double)K * We - span) / 2.0;
    return r;
}

FCPP_HD int64_t patch_words_per_line(int64_t B) { return (B + 63) >> 6; }

// clamp(floor(t), 0, n - 1) for n >= 1; the comparison is made on the double, so no conversion overflows
FCPP_HD int64_t patch_floor_clamp(double t, int64_t n)
{
    const double f = floor(t);
    if (!(f >= 0.0)) return 0;
    if (f >= (double)(n - 1)) return n - 1;
    return (int64_t)f;
}

FCPP_HD int64_t patch_line(double w, double w_lo, double We, int64_t K) { return patch_floor_clamp((w - w_lo) / We, K); }
FCPP_HD int64_t patch_bin(double u, double u_min, double h, int64_t B) { return patch_floor_clamp((u - u_min) / h, B); }
FCPP_HD double patch_line_w(double w_lo, double We, int64_t k) { return w_lo + ((double)k + 0.5) * We; }

FCPP_HD int64_t patch_join_bins(double join, double h)
{
    const double f = floor(join / h);
    if (!(f >= 0.0)) return 0;
    return f >= (double)PATCH_MAX_JOIN_BINS ? PATCH_MAX_JOIN_BINS : (int64_t)f;
}

// a set bin q whose previous set bin on the line is prev (< 0: none) starts a run iff none of the bins q - J - 1 .. q - 1 is set
FCPP_HD bool patch_starts(int64_t q, int64_t prev, int64_t J) { return prev < 0 || q - prev > J + 1; }

FCPP_HD double patch_u_a(double u_min, double h, double m, int64_t q0) { return u_min + (double)q0 * h - m; }
FCPP_HD double patch_u_b(double u_min, double h, double m, int64_t q1) { return u_min + (double)(q1 + 1) * h + m; }

// one end of a swath: the point at u on line w_k, in world metres
FCPP_HD void patch_end_point(double u, double wk, double c, double s, double gx, double gy, double &x, double &y)
{
    double px, py;
    swath_point(u, wk, c, s, px, py);
    x = px + gx; y = py + gy;
}

// ---- the host's order of work (fcpp_debug_patch_swaths; the tests' native driver) ------------------------------------------------------
// one field's members join the extent keys of its regions: keys = 4 words per region of the field, zeroed; a label outside 0 .. n_reg - 1
// is no member
inline void patch_field_extent_host(int64_t nx, int64_t ny, double res, const int32_t *labels, int64_t n_reg, double c, double s, uint64_t *keys)
{
    for (int64_t b = 0; b < ny; ++b)
        for (int64_t a = 0; a < nx; ++a) {
            const int32_t lab = labels[b * nx + a];
            if (lab < 0 || (int64_t)lab >= n_reg) continue;
            double u, w;
            patch_cell_uw(a, b, res, c, s, u, w);
            const uint64_t v[4] = { patch_key(-u), patch_key(u), patch_key(-w), patch_key(w) };
            for (int j = 0; j < 4; ++j)
                if (v[j] > keys[4 * lab + j]) keys[4 * lab + j] = v[j];
        }
}

// one field's members set their bits: rec = the field's records (placed), bitmap = the call's words (n_words of them)
inline void patch_field_mark_host(int64_t nx, int64_t ny, double res, const int32_t *labels, int64_t n_reg, double c, double s, double We, double h,
                                  const PatchRecord *rec, uint64_t *bitmap, int64_t n_words)
{
    for (int64_t b = 0; b < ny; ++b)
        for (int64_t a = 0; a < nx; ++a) {
            const int32_t lab = labels[b * nx + a];
            if (lab < 0 || (int64_t)lab >= n_reg) continue;
            const PatchRecord &r = rec[lab];
            if (r.K <= 0) continue;
            double u, w;
            patch_cell_uw(a, b, res, c, s, u, w);
            const int64_t k = patch_line(w, r.w_lo, We, r.K), q = patch_bin(u, r.u_min, h, r.B);
            const int64_t word = r.first_word + k * patch_words_per_line(r.B) + (q >> 6);
            if (word >= 0 && word < n_words) bitmap[word] |= 1ull << (q & 63);
        }
}

// the runs of one line of `words` 64-bin words, in ascending u: emit(t, q0, q1) for run t; returns their number
template <class Emit>
inline int64_t patch_line_runs(const uint64_t *line, int64_t words, int64_t J, Emit emit)
{
    int64_t t = 0, prev = -1, q0 = -1;
    for (int64_t wi = 0; wi < words; ++wi) {
        uint64_t bits = line[wi];
        while (bits) {
            const int j = __builtin_ctzll(bits);
            bits &= bits - 1;
            const int64_t q = wi * 64 + j;
            if (patch_starts(q, prev, J)) {
                if (q0 >= 0) emit(t++, q0, prev);
                q0 = q;
            }
            prev = q;
        }
    }
    if (q0 >= 0) emit(t++, q0, prev);
    return t;
}

struct PatchHost {          // everything the three device entries write
    std::vector<double> frame;                  // n x 2: s, c
    std::vector<PatchRecord> records;           // per region
    int64_t n_lines = 0, n_words = 0, n_swaths = 0;
    std::vector<uint64_t> bitmap;
    std::vector<int64_t> line_counts, line_offsets, swath_offsets;
    std::vector<double> ax, ay, bx, by, length;
    std::vector<int32_t> line;
    std::vector<int64_t> region;
};

// The whole rule on the host, arguments checked by the caller.  for_fields(n, fn) calls fn(i) for every field i, in any order and on any
// threads: a field writes only its own regions' keys, words, counts and swaths.
template <class ForFields>
inline void patch_host(int64_t n, const RegionDims *dims, const int64_t *cell_offsets, double res, const int32_t *labels, const int64_t *region_offsets,
                       const double *angle, double W, double m, double join, ForFields for_fields, PatchHost &o)
{
    const int64_t n_regions = region_offsets[n];
    const double We = W - 2.0 * m, h = res;
    const int64_t J = patch_join_bins(join, h);
    o.frame.assign((size_t)(2 * n), 0.0);
    for (int64_t i = 0; i < n; ++i) fc_sincos(angle[i], o.frame[(size_t)(2 * i)], o.frame[(size_t)(2 * i + 1)]);
    std::vector<uint64_t> keys((size_t)(4 * n_regions), 0);
    for_fields(n, [&](int64_t i) {
        patch_field_extent_host(dims[i].nx, dims[i].ny, res, labels + cell_offsets[i], region_offsets[i + 1] - region_offsets[i],
                                o.frame[(size_t)(2 * i + 1)], o.frame[(size_t)(2 * i)], keys.data() + 4 * region_offsets[i]);
    });
    o.records.resize((size_t)n_regions);
    o.n_lines = o.n_words = 0;
    for (int64_t r = 0; r < n_regions; ++r) {
        PatchRecord &R = o.records[(size_t)r];
        R = patch_layout(keys[(size_t)(4 * r)], keys[(size_t)(4 * r + 1)], keys[(size_t)(4 * r + 2)], keys[(size_t)(4 * r + 3)], We, h);
        R.first_line = o.n_lines; R.first_word = o.n_words;
        o.n_lines += R.K; o.n_words += R.K * patch_words_per_line(R.B);
    }
    o.bitmap.assign((size_t)o.n_words, 0);
    o.line_counts.assign((size_t)o.n_lines, 0);
    auto each_line = [&](int64_t i, auto fn) {          // fn(region, k, global line, the line's words, how many)
        for (int64_t r = region_offsets[i]; r < region_offsets[i + 1]; ++r) {
            const PatchRecord &R = o.records[(size_t)r];
            const int64_t wpl = patch_words_per_line(R.B);
            for (int64_t k = 0; k < R.K; ++k) fn(r, k, R.first_line + k, o.bitmap.data() + R.first_word + k * wpl, wpl);
        }
    };
    for_fields(n, [&](int64_t i) {
        patch_field_mark_host(dims[i].nx, dims[i].ny, res, labels + cell_offsets[i], region_offsets[i + 1] - region_offsets[i],
                              o.frame[(size_t)(2 * i + 1)], o.frame[(size_t)(2 * i)], We, h, o.records.data() + region_offsets[i], o.bitmap.data(),
                              o.n_words);
        each_line(i, [&](int64_t, int64_t, int64_t line, const uint64_t *words, int64_t wpl) {
            o.line_counts[(size_t)line] = patch_line_runs(words, wpl, J, [](int64_t, int64_t, int64_t) {});
        });
    });
    o.line_offsets.assign((size_t)o.n_lines + 1, 0);
    for (int64_t l = 0; l < o.n_lines; ++l) o.line_offsets[(size_t)l + 1] = o.line_offsets[(size_t)l] + o.line_counts[(size_t)l];
    o.n_swaths = o.line_offsets[(size_t)o.n_lines];
    o.swath_offsets.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i <= n; ++i) {
        const int64_t r = region_offsets[i];
        o.swath_offsets[(size_t)i] = o.line_offsets[(size_t)(r < n_regions ? o.records[(size_t)r].first_line : o.n_lines)];
    }
    const size_t ms = (size_t)o.n_swaths;
    o.ax.assign(ms, 0.0); o.ay.assign(ms, 0.0); o.bx.assign(ms, 0.0); o.by.assign(ms, 0.0); o.length.assign(ms, 0.0);
    o.line.assign(ms, 0); o.region.assign(ms, 0);
    for_fields(n, [&](int64_t i) {
        const double s = o.frame[(size_t)(2 * i)], c = o.frame[(size_t)(2 * i + 1)], gx = dims[i].gx, gy = dims[i].gy;
        const int64_t field_line = region_offsets[i] < n_regions ? o.records[(size_t)region_offsets[i]].first_line : o.n_lines;
        each_line(i, [&](int64_t r, int64_t k, int64_t line, const uint64_t *words, int64_t wpl) {
            const PatchRecord &R = o.records[(size_t)r];
            const double wk = patch_line_w(R.w_lo, We, k);
            const int64_t base = o.line_offsets[(size_t)line];
            patch_line_runs(words, wpl, J, [&](int64_t t, int64_t q0, int64_t q1) {
                const size_t at = (size_t)(base + t);
                const double ua = patch_u_a(R.u_min, h, m, q0), ub = patch_u_b(R.u_min, h, m, q1);
                patch_end_point(ua, wk, c, s, gx, gy, o.ax[at], o.ay[at]);
                patch_end_point(ub, wk, c, s, gx, gy, o.bx[at], o.by[at]);
                o.length[at] = ub - ua;
                o.line[at] = (int32_t)(line - field_line);
                o.region[at] = r;
            });
        });
    });
}

}  // namespace fcpp
