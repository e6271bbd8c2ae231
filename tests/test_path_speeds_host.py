"""CPU-side tests of the path speeds: the entries exist (header, ctypes binding, libfcpp.so; ABI version still 5), argument errors need no
device -- and the RULE, through fcpp_debug_path_speeds (csrc/fcpp_speedfn.h on the host: the plain sequential two-sweep form).

The checker shares no code with the rule (tests/path_speed_cases.py): the caps pointwise in numpy (the same IEEE operations, so cap is
compared bit for bit), the profile by cumulative sums and running minima -- another order of work than the sweeps, compared to the derived
bound (n_p + 4) 2^-52 -- and the properties that define the result: under the caps, standing at every cusp and rested end, within both
acceleration limits on every step, one value across a zero step, and maximal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from tests import path_speed_cases as S
from tests.support import REPO, check_entries

ENTRIES = {'fcpp_path_speeds': 14, 'fcpp_debug_path_speeds': 12}


def test_entries_in_header_binding_and_library():
    text = check_entries(ENTRIES)
    for name, val in (('REST_START', L.SPEED_REST_START), ('REST_END', L.SPEED_REST_END), ('STOP_AT_CUSPS', L.SPEED_STOP_AT_CUSPS)):
        assert re.search(r'#define FCPP_SPEED_%s %du\b' % (name, val), text)
    assert C.sizeof(L.SpeedParams) == 8 * 15 + 8
    for src in ('fcpp_glue_speed.cpp', 'fcpp_speed.hip'):
        assert src in open(os.path.join(REPO, 'field_coverage_path_planning_amd', 'csrc', 'Makefile')).read()


SETS = [('fixed', lambda: S.fixed_set())] + [('random%d' % k, (lambda k=k: S.random_set(np.random.default_rng(100 + k)))) for k in range(6)]
PARAMS = [('default', dict()), ('asym', dict(a_acc=0.3, a_dec=0.9)), ('no_stops', dict(flags=0)), ('cusps_only', dict(flags=L.SPEED_STOP_AT_CUSPS)),
          ('slow', dict(a_acc=0.05, a_dec=0.08, turn_kmh=np.inf)), ('zero_nominal', dict(nominal=[9.0, 0.0, 15.0, 15.0, 9.0, 15.0, 15.0, 15.0]))]


@pytest.mark.parametrize('pname,pkw', PARAMS, ids=[p[0] for p in PARAMS])
@pytest.mark.parametrize('sname,make', SETS, ids=[s[0] for s in SETS])
def test_twin_against_oracle_and_properties(sname, make, pname, pkw):
    ps, prm = make(), S.params(**pkw)
    v, cap, status = S.host_speeds(ps, prm)
    ov, ocap, ostatus = S.oracle(ps, prm)
    assert np.array_equal(status, ostatus) and (status == 0).all()
    assert np.array_equal(cap.view(np.int64), ocap.view(np.int64))          # pointwise: bit for bit
    S.assert_within_bound(ps, v, ov, (sname, pname))
    S.check_properties(ps, prm, v, cap, status)
    # every output may be NULL; what is written does not depend on it
    v2, none, _ = S.host_speeds(ps, prm, want_cap=False)
    none2, cap2, _ = S.host_speeds(ps, prm, want_v=False)
    assert none is None and none2 is None and np.array_equal(v2, v) and np.array_equal(cap2, cap)


def test_what_the_reference_sweeps_get_wrong():
    """a swath at 9 km/h into a tight connector: the braking ramp crosses the doubled junction, both twins of it have one speed, and
    the vehicle stands on both samples of the cusp"""
    ps = S.pack([S.path([(200, 0.0, 0, 1), (40, 0.4, 1, 1), (30, -0.4, 1, -1), (100, 0.0, 0, 1)])])
    prm = S.params()
    v, cap, _ = S.host_speeds(ps, prm)
    assert v[199] == v[200] and v[199] <= cap[200] < 9.0 and v[150] > v[199]          # the junction: one speed, the connector's cap, reached by braking
    assert v[239] == v[240] == 0.0 and cap[239] == cap[240] == 0.0                    # the cusp
    assert v[0] == v[-1] == 0.0
    assert (v[240:270] <= 2.5 * (1 + 4 * S.EPS)).all() and v[255] > 0.0                                 # the reverse run


def test_status_cases():
    prm = S.params()
    base = S.fixed_set()
    off = base['offsets']
    target = 1          # the Reeds-Shepp-like path
    at = int(off[target]) + 5
    for col, val in (('x', np.nan), ('y', np.inf), ('kappa', np.nan), ('kappa', -np.inf), ('part', 8), ('part', -1), ('gear', 0), ('gear', 2)):
        ps = {k: a.copy() for k, a in base.items()}
        ps[col][at] = val
        v, cap, status = S.host_speeds(ps, prm)
        want = np.zeros(len(off) - 1, np.int32)
        want[target] = L.EINVAL
        assert np.array_equal(status, want), (col, val)
        sl = slice(off[target], off[target + 1])
        assert np.isnan(v[sl]).all() and np.isnan(cap[sl]).all()
        gv, gcap, _ = S.host_speeds(base, prm)
        keep = np.ones(len(v), bool)
        keep[sl] = False
        assert np.array_equal(v[keep], gv[keep]) and np.array_equal(cap[keep], gcap[keep])          # the other paths are unaffected
        ov, ocap, ostatus = S.oracle(ps, prm)
        assert np.array_equal(ostatus, status)
    # the empty path, the one-sample path, the two paths of two equal samples (fixed_set paths 2 .. 5)
    v, cap, status = S.host_speeds(base, prm)
    assert (status == 0).all() and off[3] == off[2]
    assert v[off[3]] == 0.0 and cap[off[3]] == 0.0                               # one sample, rested
    assert (v[off[4]:off[6]] == 0.0).all()
    free = S.params(flags=0)
    v, cap, status = S.host_speeds(base, free)
    assert v[off[3]] == cap[off[3]] > 0.0                                       # one sample, not rested: its cap
    assert v[off[4]] == v[off[4] + 1] == cap[off[4]] and abs(v[off[4]] - 9.0) < 1e-14                    # two equal samples: one value
    assert v[off[5]] == v[off[5] + 1] == cap[off[5] + 1] and abs(v[off[5]] - 2.5) < 1e-14                                  # ... of different gears, no stop asked for: the lower cap on both


def test_parameter_rejections():
    ps = S.fixed_set()
    for kw in (dict(reverse_kmh=0.0), dict(reverse_kmh=np.inf), dict(reverse_kmh=np.nan), dict(turn_kmh=0.0), dict(turn_kmh=np.nan), dict(a_lat=0.0),
               dict(a_lat=np.inf), dict(a_acc=0.0), dict(a_acc=-1.0), dict(a_acc=np.nan), dict(a_dec=0.0), dict(a_dec=np.inf), dict(safety_factor=0.0),
               dict(safety_factor=np.nan), dict(kappa_eps=0.0), dict(kappa_eps=np.inf), dict(flags=8),
               dict(nominal=[9.0, -1.0] + [15.0] * 6), dict(nominal=[np.nan] + [15.0] * 7)):
        S.host_speeds(ps, S.params(**kw), expect=L.EINVAL)
    S.host_speeds(ps, S.params(turn_kmh=np.inf, nominal=[np.inf] * 8))          # allowed
    prm = S.params()
    S.host_speeds(ps, None, expect=L.EINVAL)
    for col in ('offsets', 'x', 'y', 'kappa', 'part', 'gear'):
        S.host_speeds(ps, prm, expect=L.EINVAL, **{col: None})
    S.host_speeds(ps, prm, expect=L.EINVAL, status=None)
    off = ps['offsets']
    for bad in (off + 1, np.concatenate([off[:-1], [off[-1] - 1]]), np.concatenate([off[:1], [off[2] + 1], off[2:]])):
        S.host_speeds(ps, prm, expect=L.ESIZE, offsets=np.ascontiguousarray(bad))
    S.host_speeds(ps, prm, expect=L.ESIZE, n_paths=-1)
    S.host_speeds(ps, prm, expect=L.ESIZE, total=-1)
