"""Shared builders of the path-speed tests (a helper, not a test file): synthetic path sets in numpy, the numpy oracle of the rule of
csrc/fcpp_speedfn.h, the bound and the property checks, and the ctypes calls of the host twin and the device entry.

Paths are made of PIECES, each (n_samples, kappa, part, gear): a straight or an arc sampled at `spacing` with a SHORT LAST STEP, every
piece starting on the last sample of the piece before it -- a doubled junction, or a doubled cusp where the gear flips -- exactly what the
samplers of the polygon chain write.

The oracle does the work in another order than both the twin and the kernels: caps pointwise, the running step sums S by np.cumsum, then
    forwards  u_i = 2 a_acc S_i + min over j <= i of (c_j - 2 a_acc S_j)        (np.minimum.accumulate)
    backwards u_i = min over j >= i of (c_j + 2 a_dec S_j) - 2 a_dec S_i        (the same, mirrored)
The differences c_j - 2 a S_j + 2 a S_i cancel: in float64 they would lose (S_i / step) ulps, far more than the sums they stand for.  The
scans therefore run in numpy's extended type (64-bit mantissa on x86-64: the cancellation then costs 2^-63 S, nothing against the bound)
on the float64 steps, and the result is rounded to float64 once.
The bound.  Every candidate is c_j plus a sum of at most n_p non-negative terms, added in different groupings by the oracle, the twin and
the kernels, so |v - v_oracle| <= (n_p + 4) 2^-52 v_oracle with n_p the path's sample count (the 4: product, square root and the two unit
conversions); a stop is exactly 0 in all three.  cap is pointwise: the same bits everywhere.
"""
import ctypes as C

import numpy as np

from field_coverage_path_planning_amd import _lib as L
from tests.support import p as _p

EPS = 2.0 ** -52
WIDE = np.longdouble
assert np.finfo(WIDE).nmant >= 63, 'the oracle needs an extended floating-point type'
ALL_FLAGS = L.SPEED_REST_START | L.SPEED_REST_END | L.SPEED_STOP_AT_CUSPS


def params(nominal=None, reverse_kmh=2.5, turn_kmh=4.0, a_lat=2.0, a_acc=1.5, a_dec=1.5, safety_factor=0.85, kappa_eps=1e-6, flags=ALL_FLAGS):
    p = L.SpeedParams()
    nominal = [9.0, 15.0, 15.0, 15.0, 9.0, 15.0, 15.0, 15.0] if nominal is None else nominal
    for k in range(8):
        p.nominal_kmh[k] = nominal[k]
    p.reverse_kmh, p.turn_kmh, p.a_lat, p.a_acc, p.a_dec, p.safety_factor, p.kappa_eps, p.flags = (reverse_kmh, turn_kmh, a_lat, a_acc, a_dec,
                                                                                                    safety_factor, kappa_eps, flags)
    return p


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def path(pieces, spacing=0.1, x0=0.0, y0=0.0, h0=0.3):
    """pieces: (n, kappa, part, gear) each -> dict of the path's five columns.  Piece k + 1 starts on the last sample of piece k."""
    xs, ys, ks, ps, gs = [], [], [], [], []
    x, y, h = x0, y0, h0
    for n, kappa, part, gear in pieces:
        if n <= 0:
            continue
        s = spacing * np.arange(n, dtype=np.float64)
        if n >= 2:
            s[-1] = s[-2] + 0.37 * spacing          # the short last step
        ds = s * gear
        if kappa == 0.0:
            px, py = x + ds * np.cos(h), y + ds * np.sin(h)
        else:
            px, py = x + (np.sin(h + kappa * ds) - np.sin(h)) / kappa, y - (np.cos(h + kappa * ds) - np.cos(h)) / kappa
        xs.append(px); ys.append(py); ks.append(np.full(n, kappa)); ps.append(np.full(n, part, np.int8)); gs.append(np.full(n, gear, np.int8))
        x, y, h = px[-1], py[-1], h + kappa * ds[-1]
    if not xs:
        return dict(x=np.zeros(0), y=np.zeros(0), kappa=np.zeros(0), part=np.zeros(0, np.int8), gear=np.zeros(0, np.int8))
    return dict(x=np.concatenate(xs), y=np.concatenate(ys), kappa=np.concatenate(ks), part=np.concatenate(ps), gear=np.concatenate(gs))


def pack(paths):
    """a list of paths -> the path set: offsets + the five columns"""
    out = {k: np.ascontiguousarray(np.concatenate([p[k] for p in paths]) if paths else np.zeros(0), dtype=dt)
           for k, dt in (('x', np.float64), ('y', np.float64), ('kappa', np.float64), ('part', np.int8), ('gear', np.int8))}
    out['offsets'] = np.concatenate([[0], np.cumsum([len(p['x']) for p in paths])]).astype(np.int64)
    return out


def straight_arc_straight(n1, n2, n3, radius=6.0, spacing=0.1, **kw):
    return path([(n1, 0.0, 0, 1), (n2, 1.0 / radius, 1, 1), (n3, 0.0, 0, 1)], spacing, **kw)


def reeds_shepp_like(n1, n2, n3, radius=5.0, spacing=0.1, **kw):
    """forwards on an arc, a cusp, backwards on the mirrored arc, a cusp, forwards straight"""
    return path([(n1, 1.0 / radius, 1, 1), (n2, -1.0 / radius, 1, -1), (n3, 0.0, 0, 1)], spacing, **kw)


def seam_path(length, at, cusp, spacing=0.1):
    """`length` samples with ONE doubled pair at samples at - 1, at: a cusp (the gear flips) or a junction with a curvature step"""
    if cusp:
        return path([(at, 0.0, 0, 1), (length - at, 0.0, 0, -1)], spacing)
    return path([(at, 0.0, 0, 1), (length - at, 0.25, 1, 1)], spacing)


def fixed_set():
    """the fixed shapes of the host tests: every kind of piece, empty, one-sample and two-equal-sample paths"""
    two = path([(1, 0.0, 0, 1), (1, 0.0, 0, 1)])
    two_cusp = path([(1, 0.0, 0, 1), (1, 0.0, 0, -1)])
    return pack([straight_arc_straight(300, 90, 211), reeds_shepp_like(57, 33, 140), path([]), path([(1, 0.2, 4, 1)]), two, two_cusp,
                 path([(40, 0.0, 0, 1), (25, -0.125, 4, 1), (12, 0.5, 2, 1), (3, 0.0, 3, -1), (30, 0.0, 5, 1), (20, 1e-7, 6, 1)], 0.25),
                 straight_arc_straight(700, 0, 423, spacing=0.05), path([(2, 0.0, 0, 1)]), path([(3, 2.0, 1, -1)])])


def random_set(rng, n_paths=12, max_pieces=6, max_n=80):
    paths = []
    for _ in range(n_paths):
        pieces = [(int(rng.integers(0, max_n)), float(rng.choice([0.0, 0.0, 0.1, -0.3, 1.5, 1e-7])), int(rng.integers(0, 7)), int(rng.choice([1, 1, -1])))
                  for _ in range(int(rng.integers(0, max_pieces)))]
        paths.append(path(pieces, float(rng.choice([0.05, 0.1, 0.5]))))
    return pack(paths)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def oracle(ps, prm):
    """-> v, cap [km/h], status: the rule in numpy, scans instead of sweeps"""
    off = ps['offsets']
    n_paths = len(off) - 1
    v, cap = np.zeros(len(ps['x'])), np.zeros(len(ps['x']))
    status = np.zeros(n_paths, np.int32)
    nom = np.array(list(prm.nominal_kmh))
    with np.errstate(all='ignore'):
        for p in range(n_paths):
            sl = slice(off[p], off[p + 1])
            x, y, kap, part, gear = (ps[k][sl] for k in ('x', 'y', 'kappa', 'part', 'gear'))
            n = len(x)
            if n == 0:
                continue
            if not (np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(kap).all() and ((part >= 0) & (part <= 7)).all()
                    and (np.abs(gear) == 1).all()):
                v[sl] = cap[sl] = np.nan
                status[p] = L.EINVAL
                continue
            ms = nom[part] / 3.6
            c = ms * ms
            rev = prm.reverse_kmh / 3.6
            c = np.where(gear < 0, np.minimum(c, rev * rev), c)
            ak = np.abs(kap)
            turn = prm.turn_kmh / 3.6
            vm = np.sqrt(prm.a_lat / np.where(ak > prm.kappa_eps, ak, 1.0)) * prm.safety_factor
            c = np.where(ak > prm.kappa_eps, np.minimum(np.minimum(c, turn * turn), vm * vm), c)
            c[stops(gear, prm.flags)] = 0.0
            cap[sl] = np.sqrt(c) * 3.6
            S = np.concatenate([[0.0], np.cumsum(steps(x, y).astype(WIDE))])
            fa, fd = WIDE(2.0 * prm.a_acc) * S, WIDE(2.0 * prm.a_dec) * S
            fwd = np.minimum.accumulate(c - fa) + fa
            bwd = np.minimum.accumulate((c + fd)[::-1])[::-1] - fd
            v[sl] = np.sqrt(np.minimum(fwd, bwd).astype(np.float64)) * 3.6
    return v, cap, status


def steps(x, y):
    dx, dy = np.diff(x), np.diff(y)
    return np.sqrt(dx * dx + dy * dy)


def stops(gear, flags):
    n = len(gear)
    s = np.zeros(n, bool)
    if n and flags & L.SPEED_REST_START:
        s[0] = True
    if n and flags & L.SPEED_REST_END:
        s[-1] = True
    if flags & L.SPEED_STOP_AT_CUSPS:
        flip = gear[1:] != gear[:-1]
        s[1:] |= flip
        s[:-1] |= flip
    return s


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------
def assert_within_bound(ps, v, ref, what):
    """|v - ref| <= (n_p + 4) 2^-52 ref per path; NaN where ref is NaN, +inf where it is +inf, 0 exactly where it is 0"""
    off = ps['offsets']
    for p in range(len(off) - 1):
        a, r = v[off[p]:off[p + 1]], ref[off[p]:off[p + 1]]
        n = len(a)
        assert np.array_equal(np.isnan(a), np.isnan(r)), (what, p)
        fin = np.isfinite(r)
        assert np.array_equal(a[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), (what, p)
        assert np.array_equal(a[fin] == 0.0, r[fin] == 0.0), (what, p)
        err = np.abs(a[fin] - r[fin])
        bad = err > (n + 4) * EPS * r[fin]
        assert not bad.any(), (what, p, n, float((err / np.maximum(r[fin], 1e-300)).max() / EPS))


def check_properties(ps, prm, v, cap, status, slack=0):
    """The properties of the rule on every path of status 0.  The step checks recompute u = (v / 3.6)^2: four roundings on the way out and
    back, under 4 * 2^-52 relative per u; the sweep's own sum and product add one each.  So a tight step misses
    (u_i - u_(i-1)) / (2 d) = a by at most a * tau_i, tau_i = 2^-52 ((5 + 4 slack) (u_i + u_(i-1)) / (2 a d) + 4), where slack = 0 for the
    host twin, whose sweeps ARE those sums, and slack = n_p + 4 for the device, whose v lies within (n_p + 4) 2^-52 of such a profile (u
    within twice that, on both ends of the step).  Across a zero step the twin's two values are one value; the device's agree to its bound."""
    off = ps['offsets']
    for p in range(len(off) - 1):
        if status[p] != 0:
            continue
        sl = slice(off[p], off[p + 1])
        vv, cc, gear = v[sl], cap[sl], ps['gear'][sl]
        n = len(vv)
        if n == 0:
            continue
        k = slack(n) if callable(slack) else slack
        assert (vv <= cc).all(), p
        st = stops(gear, prm.flags)
        assert (vv[st] == 0.0).all() and (cc[st] == 0.0).all(), p
        if n == 1 or not np.isfinite(vv).all():
            continue
        u = (vv / 3.6) ** 2
        d = steps(ps['x'][sl], ps['y'][sl])
        pos = d > 0
        with np.errstate(all='ignore'):
            slope = (u[1:] - u[:-1]) / (2.0 * d)
            tau_acc = EPS * ((5 + 4 * k) * (u[1:] + u[:-1]) / (2.0 * prm.a_acc * d) + 4)
            tau_dec = EPS * ((5 + 4 * k) * (u[1:] + u[:-1]) / (2.0 * prm.a_dec * d) + 4)
        assert (slope[pos] <= prm.a_acc * (1 + tau_acc[pos])).all(), p
        assert (slope[pos] >= -prm.a_dec * (1 + tau_dec[pos])).all(), p
        same = np.abs(vv[1:][~pos] - vv[:-1][~pos]) <= 2 * k * EPS * vv[1:][~pos]
        assert same.all(), p
        # maximality, per group of samples joined by zero steps (one value): a member at its cap, or the step into the group tight
        # against a_acc, or the step out of it tight against a_dec
        acc_tight = np.zeros(n, bool)
        dec_tight = np.zeros(n, bool)
        acc_tight[1:][pos] = slope[pos] >= prm.a_acc * (1 - tau_acc[pos])
        dec_tight[:-1][pos] = slope[pos] <= -prm.a_dec * (1 - tau_dec[pos])
        at_cap = np.abs(vv - cc) <= 2 * k * EPS * cc
        group = np.concatenate([[0], np.cumsum(pos)])
        held = np.zeros(group[-1] + 1, bool)
        np.logical_or.at(held, group, at_cap | acc_tight | dec_tight)
        assert held.all(), (p, np.flatnonzero(~held)[:5])


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------


def host_speeds(ps, prm, expect=L.OK, want_v=True, want_cap=True, **override):
    """fcpp_debug_path_speeds -> v, cap, status (None where not asked for); override: a column or 'offsets' replaced (None: NULL)"""
    lib = L.load()
    a = dict(ps)
    a.update(override)
    total = len(ps['x'])
    n = len(ps['offsets']) - 1
    v = np.full(total, 7.0) if want_v else None
    cap = np.full(total, 7.0) if want_cap else None
    status = np.full(n, 99, np.int32)
    rc = lib.fcpp_debug_path_speeds(C.byref(prm) if prm is not None else None, override.get('n_paths', n), _p(a['offsets']),
                                    override.get('total', total), _p(a['x']), _p(a['y']), _p(a['kappa']), _p(a['part']), _p(a['gear']),
                                    _p(v), _p(cap), _p(status) if override.get('status', True) is not None else None)
    assert rc == expect, (rc, lib.fcpp_last_error())
    return v, cap, status


def device_speeds(ps, prm, device=None):
    """fcpp_path_speeds on ordinary device tensors -> v, cap, status as numpy"""
    import torch
    from field_coverage_path_planning_amd import engine as E
    ctx = E.get_context(device)
    dev = torch.device('cuda', ctx.device)
    t = {k: torch.as_tensor(ps[k], device=dev) for k in ('offsets', 'x', 'y', 'kappa', 'part', 'gear')}
    total, n = len(ps['x']), len(ps['offsets']) - 1
    v, cap = torch.full((total,), 7.0, dtype=torch.float64, device=dev), torch.full((total,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((n,), 99, dtype=torch.int32, device=dev)
    ctx.bind_stream()
    rc = ctx.lib.fcpp_path_speeds(ctx.handle, C.byref(prm), n, E._ptr(t['offsets']), total, E._ptr(t['x']), E._ptr(t['y']), E._ptr(t['kappa']),
                                  E._ptr(t['part']), E._ptr(t['gear']), E._ptr(v), E._ptr(cap), E._ptr(status), _p(ps['offsets']))
    assert rc == L.OK, ctx.lib.fcpp_last_error()
    return v.cpu().numpy(), cap.cpu().numpy(), status.cpu().numpy()
