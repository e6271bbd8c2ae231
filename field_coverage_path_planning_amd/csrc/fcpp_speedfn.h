// fcpp_speedfn.h -- path speeds: the speed profile of the polygon chain's sampled paths (field paths, headland paths, loop transits,
// mission paths) from what their samples carry: the exact kappa, the part and the gear.  ONE set of expressions for the host
// (fcpp_debug_path_speeds, the tests' driver) and the device (fcpp_speed.hip), in plain IEEE-754 double operations and compiled with
// -ffp-contract=off on both sides.  Build-defined: the reference has the curvature clamp and the two sweeps of MLP:467-600 only, on chord
// curvature, with one acceleration, a 1e-6 m skip and no stop (fcpp_speed_plan mirrors those and stays what it is).
//
// THE RULE (include/fcpp.h states it for callers).  Per path of n samples, speeds in m/s, u = v^2:
//   cap    c_i = the smallest of  (nominal_kmh[part_i] / 3.6)^2;  (reverse_kmh / 3.6)^2 where gear_i = -1;  and where |kappa_i| > kappa_eps
//          (turn_kmh / 3.6)^2 and (sqrt(a_lat / |kappa_i|) * safety_factor)^2 -- the reference's formula (MLP:496-499) on the STORED kappa.
//   stops  c_i = 0 at sample 0 with REST_START, at sample n - 1 with REST_END, and with STOP_AT_CUSPS at every sample whose gear differs
//          from its predecessor's or its successor's within the path: both samples of a doubled cusp.
//   steps  d_i = sqrt((x_i - x_(i-1))^2 + (y_i - y_(i-1))^2), fcpp_trajectory's expression.  No threshold: a zero step passes the value on.
//   sweeps u_i = min(c_i, u_(i-1) + 2 a_acc d_i) forwards, then u_i = min(u_i, u_(i+1) + 2 a_dec d_(i+1)) backwards: the greatest
//          profile under the caps and both limits,  u_i = min over j of  c_j + 2 a_acc (d_(j+1) + .. + d_i)  for j <= i  and
//          c_j + 2 a_dec (d_(i+1) + .. + d_j)  for j >= i.  The host walks the two sweeps; the device composes the maps u -> min(c, u + w)
//          in a scan.  Both add the same non-negative terms in different groupings: |v - v'| <= (n + 4) 2^-52 v, stops exactly 0.
//   out    v_i = sqrt(u_i) * 3.6 and cap_i = sqrt(c_i) * 3.6 [km/h]; cap is pointwise, hence the same bits on both sides.
//   status SPEED_EINVAL for a path with a non-finite x, y or kappa, a part outside 0 .. 7 or a gear other than +-1: NaN in both outputs
//          over the whole path.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/fcpp.h"
#include "fcpp_geom.h"

namespace fcpp {

constexpr int SPEED_OK = 0, SPEED_EINVAL = -1;          // FCPP_OK / FCPP_EINVAL

// fcpp_speed_params in the units of the sweeps
struct SpeedRule {
    double nom_u[8];            // (nominal_kmh[part] / 3.6)^2
    double rev_u, turn_u;       // likewise of reverse_kmh and turn_kmh
    double a_lat, sf, kappa_eps;
    double two_acc, two_dec;    // 2 a_acc, 2 a_dec
    uint32_t flags;
};

FCPP_HD double speed_kmh_u(double kmh) { const double ms = kmh / 3.6; return ms * ms; }

// false: a parameter that is not finite and positive (turn_kmh and the nominals may be +inf, a nominal may be 0: a stop)
inline bool speed_rule(const fcpp_speed_params &p, SpeedRule &r)
{
    auto pos = [](double v) { return v > 0.0 && isfinite(v); };
    for (int k = 0; k < 8; ++k) {
        if (!(p.nominal_kmh[k] >= 0.0)) return false;
        r.nom_u[k] = speed_kmh_u(p.nominal_kmh[k]);
    }
    if (!pos(p.reverse_kmh) || !(p.turn_kmh > 0.0) || !pos(p.a_lat) || !pos(p.a_acc) || !pos(p.a_dec) || !pos(p.safety_factor) || !pos(p.kappa_eps))
        return false;
    if (p.flags & ~(uint32_t)(FCPP_SPEED_REST_START | FCPP_SPEED_REST_END | FCPP_SPEED_STOP_AT_CUSPS)) return false;
    r.rev_u = speed_kmh_u(p.reverse_kmh); r.turn_u = speed_kmh_u(p.turn_kmh);
    r.a_lat = p.a_lat; r.sf = p.safety_factor; r.kappa_eps = p.kappa_eps;
    r.two_acc = 2.0 * p.a_acc; r.two_dec = 2.0 * p.a_dec;
    r.flags = p.flags;
    return true;
}

FCPP_HD bool speed_sample_ok(double x, double y, double kappa, int part, int gear)
{
    return isfinite(x) && isfinite(y) && isfinite(kappa) && part >= 0 && part <= 7 && (gear == 1 || gear == -1);
}

// the cap of a valid sample that is no stop
FCPP_HD double speed_cap_u(const SpeedRule &r, double kappa, int part, int gear)
{
    double c = r.nom_u[part & 7];
    if (gear < 0) c = fmin(c, r.rev_u);
    const double ak = fabs(kappa);
    if (ak > r.kappa_eps) {
        const double vm = sqrt(r.a_lat / ak) * r.sf;          // MLP:496-499
        c = fmin(fmin(c, r.turn_u), vm * vm);
    }
    return c;
}

// sample i of n stands: g_prev / g_next are read only where the sample has that neighbour
FCPP_HD bool speed_stop(uint32_t flags, int64_t i, int64_t n, int g_prev, int g, int g_next)
{
    return ((flags & FCPP_SPEED_REST_START) && i == 0) || ((flags & FCPP_SPEED_REST_END) && i == n - 1)
           || ((flags & FCPP_SPEED_STOP_AT_CUSPS) && ((i > 0 && g_prev != g) || (i < n - 1 && g_next != g)));
}

FCPP_HD double speed_step(double x0, double y0, double x1, double y1)
{
    const double dx = x1 - x0, dy = y1 - y0;
    return sqrt(dx * dx + dy * dy);
}

FCPP_HD double speed_out(double u) { return sqrt(u) * 3.6; }

// One path on the host, the plain sequential form: caps, the forward sweep, the backward sweep.  The columns are the path's own (sample 0
// first); v and cap may each be NULL; u: n values of scratch.  -> the path's status.
inline int speed_path_host(const SpeedRule &r, int64_t n, const double *x, const double *y, const double *kappa, const int8_t *part,
                           const int8_t *gear, double *u, double *v, double *cap)
{
    bool ok = true;
    for (int64_t i = 0; i < n && ok; ++i) ok = speed_sample_ok(x[i], y[i], kappa[i], part[i], gear[i]);
    if (!ok) {
        const double nan = __builtin_nan("");
        for (int64_t i = 0; i < n; ++i) {
            if (v) v[i] = nan;
            if (cap) cap[i] = nan;
        }
        return SPEED_EINVAL;
    }
    for (int64_t i = 0; i < n; ++i) {
        const bool stop = speed_stop(r.flags, i, n, i > 0 ? gear[i - 1] : 0, gear[i], i < n - 1 ? gear[i + 1] : 0);
        u[i] = stop ? 0.0 : speed_cap_u(r, kappa[i], part[i], gear[i]);
        if (cap) cap[i] = speed_out(u[i]);
    }
    for (int64_t i = 1; i < n; ++i) u[i] = fmin(u[i], u[i - 1] + r.two_acc * speed_step(x[i - 1], y[i - 1], x[i], y[i]));
    for (int64_t i = n - 2; i >= 0; --i) u[i] = fmin(u[i], u[i + 1] + r.two_dec * speed_step(x[i], y[i], x[i + 1], y[i + 1]));
    for (int64_t i = 0; v && i < n; ++i) v[i] = speed_out(u[i]);
    return SPEED_OK;
}

}  // namespace fcpp
