// fcpp_connfn.h -- the connectors behind ONE interface, host+device: Conn<0> Dubins (fcpp_dubinsfn.h), Conn<1> Reeds-Shepp (fcpp_rsfn.h).
// The mathematics stays in those two headers; what is written HERE, once, is what every user of a solved connector shares: the count
// rule of the fixed-step samplers and where sample k of a solved path lies.  The kernels (fcpp_conn.hip), the router (fcpp_routefn.h) and
// the field paths (fcpp_fpathfn.h) all go through it, on the host and on the device, in plain IEEE-754 double operations.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_dubinsfn.h"
#include "fcpp_rsfn.h"

namespace fcpp {

// The count rule: K = floor(T / step) + 1 samples at k * step, and one more AT T when with_end is set and the last of them lies before
// it.  A total that is negative or not finite, or 2^31 samples or more, counts as bad (K = 0); nan_one: a NaN total is one sample instead.
FCPP_HD int64_t sample_count(double T, double step, bool with_end, bool nan_one, int64_t &bad)
{
    const double q = floor(T / step);
    if (nan_one && T != T) return 1;
    if (!(T >= 0.0) || !(q < 2147483646.0)) { ++bad; return 0; }
    const int64_t K = (int64_t)q + 1;
    return K + (with_end && (double)(K - 1) * step < T ? 1 : 0);
}

// A path sampled PER RUN (a Reeds-Shepp path, run by run of one gear): every run of length len[r] by the count rule with its end, so that
// a junction of two runs is a sample of both.  2^31 samples or more in all count as bad, like one run of that many.
FCPP_HD int64_t sample_count_runs(const double *len, int n_runs, double step, int64_t &bad)
{
    int64_t K = 0, b = 0;
    for (int r = 0; r < n_runs; ++r) K += sample_count(len[r], step, true, false, b);
    if (b || K > 2147483646) { ++bad; return 0; }
    return K;
}

// Conn<MODE>: NSEG segments per solved path; Pose / prep: what depends on one pose only; idle(): the pose of a lane without a column;
// solve_prepped / solve: the shortest word, its NSEG segment lengths and their total (word -1: a non-finite input);
// count(word, seg, spacing, bad): the samples of a solved path (0 and ++bad for a bad one);
// eval(start pose, R, word, seg, spacing, k, K, ...): sample k of its K -- s = k * spacing (one multiplication, never accumulated), the
// last sample AT the end.
template <int MODE> struct Conn;

template <> struct Conn<0> {
    static constexpr int NSEG = 3;
    using Pose = DubinsPose;
    static FCPP_HD Pose prep(double x, double y, double h, double R) { return dubins_prep(x, y, h, R); }
    static FCPP_HD Pose idle() { return { 0.0, 0.0, 0.0, 0.0, 0.0 }; }
    static FCPP_HD void solve_prepped(const Pose &f, const Pose &t, double R, int &word, double *seg, double &total)
    {
        dubins_solve_prepped(f, t, R, word, seg[0], seg[1], seg[2], total);
    }
    static FCPP_HD void solve(double x0, double y0, double h0, double x1, double y1, double h1, double R, int &word, double *seg, double &total)
    {
        dubins_solve(x0, y0, h0, x1, y1, h1, R, word, seg[0], seg[1], seg[2], total);
    }
    static FCPP_HD int64_t count(int, const double *seg, double spacing, int64_t &bad)
    {
        return sample_count((seg[0] + seg[1]) + seg[2], spacing, true, false, bad);
    }
    static FCPP_HD void eval(double x0, double y0, double h0, double R, int word, const double *seg, double spacing, int64_t k, int64_t K, double &x,
                             double &y, double &h, double &kappa, int &gear)
    {
        const double total = (seg[0] + seg[1]) + seg[2];
        double s = (double)k * spacing;
        if (k >= K - 1 || s > total) s = total;             // (K - 1) * spacing <= total: the last sample is the path's end either way
        dubins_pose_at(x0, y0, h0, R, word, seg[0], seg[1], seg[2], s, x, y, h, kappa);
        gear = 1;
    }
};

// Reeds-Shepp is counted and sampled per gear run (rs_runs): the last sample of a run lies AT its end, which is the first sample of the
// next run -- a cusp is two samples with one pose and opposite gears.  A path without a word or with a NaN segment is one NaN sample.
template <> struct Conn<1> {
    static constexpr int NSEG = 5;
    using Pose = RsPose;
    static FCPP_HD Pose prep(double x, double y, double h, double) { return rs_prep(x, y, h); }
    static FCPP_HD Pose idle() { return { 0.0, 0.0, 0.0, 0.0, 1.0 }; }
    static FCPP_HD void solve_prepped(const Pose &f, const Pose &t, double R, int &word, double *seg, double &total)
    {
        rs_solve_prepped(f, t, R, word, seg, total);
    }
    static FCPP_HD void solve(double x0, double y0, double h0, double x1, double y1, double h1, double R, int &word, double *seg, double &total)
    {
        rs_solve(x0, y0, h0, x1, y1, h1, R, word, seg, total);
    }
    static FCPP_HD bool solved(int w, const double *s)
    {
        return w >= 0 && w < RS_WORDS && s[0] == s[0] && s[1] == s[1] && s[2] == s[2] && s[3] == s[3] && s[4] == s[4];
    }
    static FCPP_HD int64_t count(int word, const double *seg, double spacing, int64_t &bad)
    {
        if (!solved(word, seg)) return 1;
        const RsRuns runs = rs_runs(word, seg);
        return sample_count_runs(runs.len, runs.n, spacing, bad);
    }
    static FCPP_HD void eval(double x0, double y0, double h0, double R, int word, const double *seg, double spacing, int64_t k, int64_t, double &x,
                             double &y, double &h, double &kappa, int &gear)
    {
        x = y = h = kappa = __builtin_nan("");
        gear = 0;
        if (!solved(word, seg)) return;
        const RsRuns runs = rs_runs(word, seg);
        int r = 0;
        int64_t Kr = 0, bad = 0;
        for (; r < runs.n; ++r) {
            Kr = sample_count(runs.len[r], spacing, true, false, bad);
            if (k < Kr || r == runs.n - 1) break;
            k -= Kr;
        }
        double e = (double)k * spacing;
        if (k >= Kr - 1 || e > runs.len[r]) e = runs.len[r];        // (Kr - 1) * spacing <= the run's length: its last sample is its end
        rs_pose_in_run(x0, y0, h0, R, word, seg, runs, r, e, x, y, h, kappa, gear);
    }
};

}  // namespace fcpp
