// polygon_cover_sanitize_driver.cpp -- csrc/fcpp_pcoverfn.h (the rule behind fcpp_debug_polygon_cover and the polygon-coverage kernels) under
// ASan + UBSan on the CPU.  The fields: the 40 x 20 rectangle, the L with its hole, a 300-vertex star, fields of exactly 64 and 65 columns, a
// field with a NaN vertex, a ring of two vertices, no ring, a field of more than 2^28 cells, and random rectangles and stars.  The paths:
// swaths, a run of more than 256 samples, a fine arc, runs with connectors masked out, NaN and infinite samples, paths of no and of one
// sample, paths that leave the grid, random zigzags; both caps, with and without the work and pass arrays, the path table grouped and
// permuted.  Every array is allocated at its exact size, so a read or write past a field's cells, vertices or samples is a report.  Any
// sanitizer report aborts; the driver itself checks what every field must give: the counts are the grid's, overlapped implies covered,
// round ends only add, a permuted table changes nothing, the known counts of the rectangle.
// usage: polygon_cover_sanitize_driver SEED N
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../field_coverage_path_planning_amd/csrc/fcpp_pcoverfn.h"

using namespace fcpp;

struct Field {
    std::vector<int64_t> vo{ 0 };
    std::vector<double> x, y;
    void ring(const std::vector<double> &px, const std::vector<double> &py)
    {
        x.insert(x.end(), px.begin(), px.end());
        y.insert(y.end(), py.begin(), py.end());
        vo.push_back((int64_t)x.size());
    }
};

struct Path {
    std::vector<double> x, y;
    std::vector<uint8_t> work;
    std::vector<int32_t> pass;
    void add(double px, double py, int w, int ps) { x.push_back(px); y.push_back(py); work.push_back((uint8_t)w); pass.push_back(ps); }
};

static Field rect(double ox, double oy, double w, double h)
{
    Field f;
    f.ring({ ox, ox + w, ox + w, ox }, { oy, oy, oy + h, oy + h });
    return f;
}

static Field star(std::mt19937_64 &rng, int m)
{
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    std::vector<double> a((size_t)m), px((size_t)m), py((size_t)m);
    for (double &v : a) v = 6.283185307179586 * unit(rng);
    std::sort(a.begin(), a.end());
    for (int k = 0; k < m; ++k) { const double r = 10.0 + 20.0 * unit(rng); px[(size_t)k] = 300.0 + r * cos(a[(size_t)k]); py[(size_t)k] = -120.0 + r * sin(a[(size_t)k]); }
    Field f;
    f.ring(px, py);
    return f;
}

static Path run(double x0, double y0, double x1, double y1, int m, int pass)
{
    Path p;
    for (int k = 0; k < m; ++k) {
        const double t = m > 1 ? (double)k / (m - 1) : 0.0;
        p.add(x0 + t * (x1 - x0), y0 + t * (y1 - y0), 1, pass);
    }
    return p;
}

struct Totals {
    long ok = 0, invalid = 0, unsupported = 0, fields_without_paths = 0, cells = 0, inside = 0, covered = 0, overlapped = 0, spill = 0, flat_ends = 0,
         joints = 0, masked = 0, nonfinite = 0, empty_paths = 0, single_paths = 0, permuted = 0, round_runs = 0, long_runs = 0;
};

struct Result {
    int status;
    PcoverDims d;
    int64_t counts[4];
    std::vector<uint8_t> grid;
};

// one field under its paths, every scratch array at its exact size; the paths are stored in `order` and named by path_ids (or in place)
static Result cover(const Field &f, const std::vector<Path> &paths, const std::vector<int> &order, bool with_ids, bool with_work, bool with_pass,
                    double W, double res, int caps, Totals &t)
{
    Result out;
    out.counts[0] = out.counts[1] = out.counts[2] = out.counts[3] = 0;
    const int64_t n_rings = (int64_t)f.vo.size() - 1;
    out.status = pcover_field_dims_host(f.vo.data(), 0, n_rings, f.x.data(), f.y.data(), W, res, out.d);
    if (out.status != PCOVER_OK) {
        if (out.d.nx != 0 || out.d.ny != 0) { fprintf(stderr, "a failed field has cells\n"); exit(2); }
        return out;
    }
    std::vector<int64_t> poff{ 0 };
    std::vector<double> px, py;
    std::vector<uint8_t> work;
    std::vector<int32_t> pass;
    for (int k : order) {
        const Path &p = paths[(size_t)k];
        px.insert(px.end(), p.x.begin(), p.x.end());
        py.insert(py.end(), p.y.begin(), p.y.end());
        work.insert(work.end(), p.work.begin(), p.work.end());
        pass.insert(pass.end(), p.pass.begin(), p.pass.end());
        poff.push_back((int64_t)px.size());
    }
    std::vector<int64_t> ids(order.size());
    for (size_t s = 0; s < order.size(); ++s) ids[s] = (int64_t)s;
    if (with_ids) std::reverse(ids.begin(), ids.end());
    const int64_t nc = out.d.nx * out.d.ny;
    out.grid.assign((size_t)nc, 0xEE);
    std::vector<int32_t> first((size_t)nc);
    std::vector<double> cross(f.x.size());
    const PcoverPaths P = { px.data(), py.data(), with_work ? work.data() : nullptr, with_pass ? pass.data() : nullptr };
    pcover_field_host(f.vo.data(), 0, n_rings, f.x.data(), f.y.data(), out.d, W, res, caps, poff.data(), P, with_ids ? ids.data() : nullptr, 0,
                      (int64_t)order.size(), out.grid.data(), first.data(), cross.data(), out.counts);
    int64_t c[4] = { 0, 0, 0, 0 };
    for (uint8_t v : out.grid) {
        if (v & 0xF8) { fprintf(stderr, "a grid byte has other bits\n"); exit(2); }
        if ((v & 4) && !(v & 2)) { fprintf(stderr, "overlapped but not covered\n"); exit(2); }
        c[0] += v & 1; c[1] += (v & 3) == 3; c[2] += (v & 5) == 5; c[3] += (v & 3) == 2;
    }
    for (int k = 0; k < 4; ++k)
        if (c[k] != out.counts[k]) { fprintf(stderr, "the counts are not the grid's\n"); exit(2); }
    // what the segments were
    for (size_t s = 0; s < order.size(); ++s) {
        const int64_t p0 = poff[s], p1 = poff[s + 1];
        if (p1 - p0 == 0) ++t.empty_paths;
        if (p1 - p0 == 1) ++t.single_paths;
        if (p1 - p0 > PCOVER_CHUNK) ++t.long_runs;
        for (int64_t k = p0; k + 1 < p1; ++k) {
            double ax, ay, bx, by;
            int32_t ps;
            bool ja, jb;
            if (!pcover_segment(P, (int64_t)s, p0, p1, k, 0, ax, ay, bx, by, ps, ja, jb)) {
                if (!swath_finite(px[(size_t)k]) || !swath_finite(py[(size_t)k]) || !swath_finite(px[(size_t)k + 1]) || !swath_finite(py[(size_t)k + 1])) ++t.nonfinite;
                else ++t.masked;
                continue;
            }
            t.joints += (ja ? 1 : 0) + (jb ? 1 : 0);
            t.flat_ends += (ja ? 0 : 1) + (jb ? 0 : 1);
        }
    }
    return out;
}

static void tally(const Result &r, bool no_paths, Totals &t)
{
    if (r.status == PCOVER_EINVAL) { ++t.invalid; return; }
    if (r.status == PCOVER_EUNSUPPORTED) { ++t.unsupported; return; }
    ++t.ok;
    if (no_paths) ++t.fields_without_paths;
    t.cells += (long)r.grid.size(); t.inside += (long)r.counts[0]; t.covered += (long)r.counts[1]; t.overlapped += (long)r.counts[2]; t.spill += (long)r.counts[3];
}

// every variant of one (field, paths) pair
static void drive(const Field &f, const std::vector<Path> &paths, double W, double res, Totals &t)
{
    std::vector<int> order(paths.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
    const Result flat = cover(f, paths, order, false, true, true, W, res, 0, t);
    tally(flat, paths.empty(), t);
    const Result round = cover(f, paths, order, false, true, true, W, res, 1, t);
    tally(round, paths.empty(), t);
    if (flat.status == PCOVER_OK) {
        ++t.round_runs;
        for (size_t c = 0; c < flat.grid.size(); ++c)
            if ((flat.grid[c] & ~round.grid[c]) & 7) { fprintf(stderr, "round ends took a bit away\n"); exit(2); }
    }
    std::vector<int> rev(order.rbegin(), order.rend());
    const Result perm = cover(f, paths, rev, true, true, true, W, res, 0, t);       // stored backwards, named forwards
    tally(perm, paths.empty(), t);
    if (perm.status == PCOVER_OK) {
        ++t.permuted;
        if (perm.grid != flat.grid) { fprintf(stderr, "a permuted path table changed the grid\n"); exit(2); }
    }
    tally(cover(f, paths, order, false, false, true, W, res, 0, t), paths.empty(), t);
    tally(cover(f, paths, order, false, true, false, W, res, 1, t), paths.empty(), t);
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int n_random = argc > 2 ? atoi(argv[2]) : 40;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    Totals t;

    // the rectangle's known answers (tests/test_polygon_cover_host.py)
    {
        const Field r40 = rect(0, 0, 40, 20);
        std::vector<Path> five, shorter;
        int id = 0;
        for (double y : { 2.0, 6.0, 10.0, 14.0, 18.0 }) { five.push_back(run(0, y, 40, y, 3, id)); shorter.push_back(run(2, y, 38, y, 3, id)); ++id; }
        std::vector<int> order{ 0, 1, 2, 3, 4 };
        const int64_t want[4][3] = { { 12800, 0, 0 }, { 12800, 0, 1040 }, { 11520, 0, 0 }, { 12560, 0, 0 } };
        for (int v = 0; v < 4; ++v) {
            const Result r = cover(r40, v < 2 ? five : shorter, order, false, true, true, 4.0, 0.25, v & 1, t);
            if (r.status != 0 || r.d.nx != 176 || r.d.ny != 96 || r.counts[0] != 12800 || r.counts[1] != want[v][0] || r.counts[2] != want[v][1] || r.counts[3] != want[v][2]) {
                fprintf(stderr, "known answer %d: %ld %ld %ld %ld\n", v, (long)r.counts[0], (long)r.counts[1], (long)r.counts[2], (long)r.counts[3]);
                return 2;
            }
        }
        std::vector<Path> two{ run(0, 2, 40, 2, 3, 0), run(0, 5, 40, 5, 3, 1) };
        const Result r = cover(r40, two, { 0, 1 }, false, true, true, 4.0, 0.25, 0, t);
        if (r.counts[1] != 4480 || r.counts[2] != 640 || r.counts[3] != 0) { fprintf(stderr, "known answer: two swaths\n"); return 2; }
    }

    // the fixed shapes
    std::vector<Field> shapes;
    shapes.push_back(rect(0, 0, 40, 20));
    { Field f; f.ring({ 0, 60, 60, 25, 25, 0 }, { 0, 0, 20, 20, 50, 50 }); f.ring({ 10, 20, 20, 10 }, { 5, 5, 15, 15 }); shapes.push_back(f); }
    shapes.push_back(star(rng, 300));
    shapes.push_back(rect(100, 0, 12, 9));
    shapes.push_back(rect(100, 0, 12.25, 9));
    { Field f = rect(0, 0, 10, 10); f.y[2] = NAN; shapes.push_back(f); }
    { Field f; f.ring({ 0, 10 }, { 0, 0 }); shapes.push_back(f); }
    shapes.push_back(Field());
    shapes.push_back(rect(0, 0, 5000, 4000));
    { Field f = rect(0, 0, 10, 10); f.x[1] = INFINITY; shapes.push_back(f); }
    for (const Field &f : shapes) {
        double x0 = 0, x1 = 40, y0 = 0, y1 = 20;
        if (!f.x.empty() && swath_finite(f.x[0]) && swath_finite(f.y[0])) { x0 = f.x[0] - 30; x1 = f.x[0] + 60; y0 = f.y[0] - 30; y1 = f.y[0] + 60; }
        std::vector<Path> paths;
        paths.push_back(run(x0 + 30, y0 + 32, x0 + 70, y0 + 32, 401, 0));                  // more than 256 samples
        paths.push_back(run(x0 + 30, y0 + 35, x0 + 70, y0 + 35, 3, 1));                    // overlaps the first
        { Path a; for (int k = 0; k < 40; ++k) a.add(x0 + 40 + 6 * cos(k * M_PI / 78), y0 + 40 + 6 * sin(k * M_PI / 78), 1, 2); paths.push_back(a); }
        {   // two runs and the connector between them, masked; a NaN and an infinite sample inside a run
            Path p = run(x0 + 32, y0 + 44, x0 + 60, y0 + 44, 9, 3);
            for (int k = 1; k < 8; ++k) p.add(x0 + 60 + 3 * sin(k * M_PI / 8), y0 + 47 - 3 * cos(k * M_PI / 8), 0, 3);
            const Path back = run(x0 + 60, y0 + 50, x0 + 32, y0 + 50, 9, 4);
            p.x.insert(p.x.end(), back.x.begin(), back.x.end()); p.y.insert(p.y.end(), back.y.begin(), back.y.end());
            p.work.insert(p.work.end(), back.work.begin(), back.work.end()); p.pass.insert(p.pass.end(), back.pass.begin(), back.pass.end());
            p.x[3] = NAN; p.y[20] = INFINITY;
            paths.push_back(p);
        }
        paths.push_back(Path());                                                           // no sample
        paths.push_back(run(x0 + 35, y0 + 35, x0 + 35, y0 + 35, 1, 5));                    // one sample
        paths.push_back(run(x0 - 500, y0 - 500, x1 + 500, y1 + 500, 7, 6));                // leaves the grid on both sides
        paths.push_back(run(x0 + 33, y0 + 33, x0 + 33, y0 + 33, 4, 7));                    // four samples at one point: segments of length 0
        drive(f, paths, 4.0, 0.25, t);
        drive(f, {}, 4.0, 0.25, t);
    }
    // random fields and zigzags
    for (int it = 0; it < n_random; ++it) {
        const bool is_star = unit(rng) < 0.3;
        const Field f = is_star ? star(rng, 3 + (int)(unit(rng) * 40)) : rect(-500 + 1000 * unit(rng), -500 + 1000 * unit(rng), 3 + 40 * unit(rng), 3 + 40 * unit(rng));
        const double W = 0.5 + 5.5 * unit(rng), res = 0.2 + 0.8 * unit(rng);
        const double cx = f.x[0], cy = f.y[0];
        std::vector<Path> paths;
        const int np = (int)(unit(rng) * 5);
        for (int k = 0; k < np; ++k) {
            Path p;
            const int m = (int)(unit(rng) * 30);
            for (int j = 0; j < m; ++j) {
                double px = cx - 30 + 80 * unit(rng), py = cy - 30 + 80 * unit(rng);
                if (unit(rng) < 0.03) px = NAN;
                p.add(px, py, unit(rng) < 0.85, (int)(unit(rng) * 3));
            }
            paths.push_back(p);
        }
        drive(f, paths, W, res, t);
    }
    printf("ok %ld invalid %ld unsupported %ld no_paths %ld cells %ld inside %ld covered %ld overlapped %ld spill %ld flat_ends %ld joints %ld masked %ld "
           "nonfinite %ld empty_paths %ld single_paths %ld permuted %ld round_runs %ld long_runs %ld\n",
           t.ok, t.invalid, t.unsupported, t.fields_without_paths, t.cells, t.inside, t.covered, t.overlapped, t.spill, t.flat_ends, t.joints, t.masked,
           t.nonfinite, t.empty_paths, t.single_paths, t.permuted, t.round_runs, t.long_runs);
    return 0;
}
