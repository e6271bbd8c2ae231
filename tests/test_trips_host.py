"""CPU-side tests of the service trips: the two entries exist (header, ctypes binding, libfcpp.so; ABI version still 5), the call's errors
need no device -- and the RULE, through fcpp_debug_trip_solve (csrc/fcpp_tripfn.h on the host: the very expressions the kernel runs).

The checker shares no code with the library (tests/trip_cases.py): the tables of a tour restated in Python floats from include/fcpp.h -- a
sum of two doubles rounds like the library's (-ffp-contract=off), so "to the bit" is meant literally -- and the least cost over EVERY stop
set of every variant, 2^(m - 1) of them for m <= 10."""
import dataclasses

import numpy as np
import pytest

from tests import trip_cases as TC
from tests.support import bits, check_entries, lib, p          # noqa: F401 (lib: a fixture)
from tests.trip_cases import EINVAL, INF, KINDS, poisoned

ENTRIES = {'fcpp_trip_solve': 30, 'fcpp_debug_trip_solve': 27}
ESIZE = -6


def test_header_binding_and_abi(lib):
    header = check_entries(ENTRIES, lib)
    assert 'service trips' in header and 'csrc/fcpp_tripfn.h' in header


# ---- what every split field must give ---------------------------------------------------------------------------------------------------
def check_field(b, r, f, oracle_row=None):
    """field f of the twin's results r against the rule, restated: the cost row (where the oracle's is given), the winner, the tour, the
    trips and that the returned stops are feasible and cost what `cost` says"""
    T, length, E, X, In, Out, tours = b.field(f)
    s0, m = int(b.soff[f]), b.m(f)
    Q, Q0 = float(b.Q[f]), float(b.Q[f] if b.Q0 is None else b.Q0[f])
    row = r['costs'][f]
    assert r['status'][f] == 0
    if oracle_row is not None:
        assert bits(row).tolist() == bits(oracle_row).tolist(), (f, row, oracle_row)
    exists = [v for v in range(2 * b.C) if b.both_ways or v % 2 == 0]
    assert all(np.isnan(row[v]) for v in range(2 * b.C) if v not in exists)
    win = int(r['winner'][f])
    assert win == min(exists, key=lambda v: (row[v], v))          # the least total, ties to the lowest v
    assert bits(r['cost'][f]) == bits(row[win])
    t = TC.variant(tours[win >> 1], win & 1)
    assert r['tour'][s0:s0 + m].tolist() == t.tolist()
    trip = r['trip'][s0:s0 + m]
    n_trips = int(r['n_trips'][f])
    if m == 0:
        assert n_trips == 0 and r['overfull'][f] == 0 and r['cost'][f] == 0.0 and r['base'][f] == 0.0 and r['extra'][f] == 0.0
        return
    assert trip[0] == 0 and trip[-1] == n_trips - 1 and set(np.diff(trip).tolist()) <= {0, 1}
    starts = [0] + [j for j in range(1, m) if trip[j] != trip[j - 1]]
    P, d, base = TC.tables(t, T, length, E, X, In, Out, b.stop)
    extra = TC.cost_of(starts, P, d, Q, Q0)
    assert extra is not None, 'the returned stops are infeasible'
    assert bits(base) == bits(r['base'][f]) and bits(extra) == bits(r['extra'][f]) and bits(TC.plus(base, extra)) == bits(r['cost'][f])
    over = sum(P[j] - P[i] > (Q0 if i == 0 else Q) for i, j in zip(starts, starts[1:] + [m]))
    assert over == r['overfull'][f]


# ---- random fields against every stop set -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stop', [0.0, 7.5])
@pytest.mark.parametrize('both_ways', [1, 0])
def test_random_fields_against_all_stop_sets(lib, stop, both_ways):
    rng = np.random.default_rng(11 + int(stop) + both_ways)
    ms = np.concatenate([np.arange(11), rng.integers(1, 11, 25)])
    C = 3 if both_ways else 2
    b = TC.batch(rng, ms, C, rng.uniform(1.0, 4.0, len(ms)), first=rng.uniform(0.3, 1.0, len(ms)), stop=stop, both_ways=both_ways)
    r = TC.twin(lib, b)
    split = 0
    for f in range(b.n):
        check_field(b, r, f, TC.field_costs(b, f))
        split += r['n_trips'][f] > 1
    print('fields', b.n, 'with more than one trip', split, 'overfull trips', int(r['overfull'].sum()))
    assert split > b.n // 2 and r['overfull'].sum() > 0


def test_without_ends_and_first_capacity(lib):
    rng = np.random.default_rng(5)
    b = TC.batch(rng, rng.integers(0, 10, 20), 2, rng.uniform(1.0, 4.0, 20), ends=False)
    r = TC.twin(lib, b)
    for f in range(b.n):
        check_field(b, r, f, TC.field_costs(b, f))


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------
def even_field(m, C=1):
    """m swaths of 10 m in stored order, every transit 4, every way to and from the service point 5: every stop costs 6"""
    rng = np.random.default_rng(0)
    b = TC.batch(rng, [m], C, 2.0, ends=False, swath=10.0)
    b.T[np.isfinite(b.T)] = 4.0
    b.In[:] = 5.0
    b.Out[:] = 5.0
    b.tours[:] = 2 * np.arange(m)
    return b


def test_equal_g_goes_to_the_lowest_start(lib):
    # capacity 20 = two swaths; five swaths need two stops, every stop 6.  g = [0, 6, 6, 12, 12]: the last trip may start at 3 or 4, both
    # 12 -> 3; pred[3] is 1 or 2, both 6 -> 1; pred[1] = 0: trips {0}, {1, 2}, {3, 4}
    b = even_field(5)
    r = TC.twin(lib, b)
    assert r['trip'].tolist() == [0, 1, 1, 2, 2] and r['n_trips'][0] == 3 and r['extra'][0] == 12.0 and r['overfull'][0] == 0
    check_field(b, r, 0, TC.field_costs(b, 0))
    # three swaths: one stop, behind the first swath or the second, both 6 -> the last trip starts at 1
    b = even_field(3)
    r = TC.twin(lib, b)
    assert r['trip'].tolist() == [0, 1, 1] and r['extra'][0] == 6.0


def test_equal_variants_go_to_the_lowest(lib):
    # two candidates that are one tour; every table is symmetric, so backwards costs the same too: four equal totals -> variant 0
    b = even_field(5, C=2)
    r = TC.twin(lib, b)
    assert len(set(bits(r['costs'][0]).tolist())) == 1 and r['winner'][0] == 0
    assert r['tour'].tolist() == b.tours[0].tolist()
    # the second candidate made cheaper by one transit of its own: it wins, as given
    b.tours[1] = b.tours[0][::-1] ^ 1
    T = b.T.reshape(10, 10)
    T[b.tours[1][0], b.tours[1][1]] = 3.0
    r = TC.twin(lib, b)
    assert r['winner'][0] == 1          # (candidate 0 backwards is candidate 1's tour: v = 1 ties with v = 2 and is the lower)
    check_field(b, r, 0, TC.field_costs(b, 0))


# ---- the capacity's ends ----------------------------------------------------------------------------------------------------------------
def test_infinite_capacity_is_one_trip(lib):
    rng = np.random.default_rng(3)
    b = TC.batch(rng, [1, 4, 9, 10], 3, INF, metric=True)          # (no stop pays: none is made)
    r = TC.twin(lib, b)
    assert r['n_trips'].tolist() == [1, 1, 1, 1] and not r['trip'].any() and not r['overfull'].any() and not r['extra'].any()
    for f in range(b.n):
        T, length, E, X, In, Out, tours = b.field(f)
        for c in range(b.C):
            base = TC.tables(TC.variant(tours[c], 0), T, length, E, X, In, Out, b.stop)[2]
            assert bits(r['costs'][f, 2 * c]) == bits(base)
        check_field(b, r, f)


def test_capacity_below_every_swath(lib):
    rng = np.random.default_rng(4)
    b = TC.batch(rng, [1, 2, 7, 10], 2, 1.0)
    b.Q[:] = 4.0          # (the shortest swath is 5 m)
    r = TC.twin(lib, b)
    assert r['n_trips'].tolist() == [1, 2, 7, 10] and r['overfull'].tolist() == [1, 2, 7, 10]
    for f in range(b.n):
        assert r['trip'][int(b.soff[f]):int(b.soff[f + 1])].tolist() == list(range(b.m(f)))
        check_field(b, r, f, TC.field_costs(b, f))


def test_no_swath_and_one_swath(lib):
    rng = np.random.default_rng(6)
    b = TC.batch(rng, [0, 1, 0], 2, 2.0)
    r = TC.twin(lib, b)
    assert r['status'].tolist() == [0, 0, 0] and r['n_trips'].tolist() == [0, 1, 0] and r['winner'][0] == 0 and r['winner'][2] == 0
    assert bits(r['costs'][0]).tolist() == [0] * 4 and r['cost'][0] == 0.0
    p0 = int(b.tours[0, 0])
    assert r['costs'][1, 0] == b.E[p0] + b.X[p0] and r['costs'][1, 1] == b.E[p0 ^ 1] + b.X[p0 ^ 1]
    assert r['trip'].tolist() == [0] and r['extra'][1] == 0.0
    for f in range(3):
        check_field(b, r, f, TC.field_costs(b, f))


# ---- the statuses -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_status_of_one_field_among_good_ones(lib, kind):
    b, status = poisoned(kind)
    r = TC.twin(lib, b)
    s0, s1 = int(b.soff[1]), int(b.soff[2])
    assert r['status'].tolist() == [0, status, 0]
    assert r['tour'][s0:s1].tolist() == b.tours[0, s0:s1].tolist() and not r['trip'][s0:s1].any()
    assert r['n_trips'][1] == 1 and r['overfull'][1] == 0 and r['winner'][1] == 0
    assert np.isnan(r['costs'][1]).all() and np.isnan([r['cost'][1], r['base'][1], r['extra'][1]]).all()
    for f in (0, 2):
        check_field(b, r, f, TC.field_costs(b, f))


def test_a_later_candidate_without_a_finite_base_only_loses(lib):
    b, _ = poisoned('none')
    s0 = int(b.soff[1])
    b.tours[0, s0:s0 + 7] = 2 * np.arange(7)
    b.tours[1, s0:s0 + 7] = [0, 4, 8, 12, 2, 6, 10]
    # a NaN transit from swath 4 to swath 6, both forwards: candidate 1 drives it, neither direction of candidate 0 does, nor candidate 1 backwards
    b.T[int(b.toff[1]):int(b.toff[2])].reshape(14, 14)[8, 12] = np.nan
    r = TC.twin(lib, b)
    assert r['status'][1] == 0 and r['costs'][1, 2] == INF and np.isfinite(r['costs'][1, [0, 1, 3]]).all() and r['winner'][1] != 2


# ---- the call's errors ------------------------------------------------------------------------------------------------------------------
def call(lib, b, **kw):
    """fcpp_debug_trip_solve with arguments replaced by name"""
    a = dict(n=b.n, soff=p(b.soff), n_total=b.n_total, toff=p(b.toff), t_total=int(b.toff[-1]), T=p(b.T), length=p(b.length), E=p(b.E), X=p(b.X),
             In=p(b.In), Out=p(b.Out), C=b.C, tours=p(b.tours), both_ways=b.both_ways, Q=p(b.Q), Q0=p(b.Q0), stop=b.stop)
    a.update(kw)
    return lib.fcpp_debug_trip_solve(*a.values(), *[None] * 10)


def test_call_errors(lib):
    rng = np.random.default_rng(9)
    b = TC.batch(rng, [3, 4], 2, 2.0, first=0.5)
    assert call(lib, b) == 0
    for name in ('soff', 'toff', 'T', 'length', 'In', 'Out', 'tours', 'Q'):
        assert call(lib, b, **{name: None}) == EINVAL, name
    assert call(lib, b, E=None, X=None, Q0=None) == 0
    for C in (0, -1, 65):
        assert call(lib, b, C=C) == EINVAL
    for stop in (-1.0, np.nan, INF):
        assert call(lib, b, stop=stop) == EINVAL
    for ways in (-1, 2):
        assert call(lib, b, both_ways=ways) == EINVAL
    assert call(lib, b, n_total=-1) == ESIZE and call(lib, b, n=-1) == ESIZE and call(lib, b, t_total=-1) == ESIZE
    assert call(lib, b, n_total=b.n_total + 1) == ESIZE and call(lib, b, t_total=int(b.toff[-1]) + 4) == ESIZE
    for bad in (b.soff + 1, [0, 5, 7], [0, 4, 3]):          # not from 0; other counts than the blocks'; decreasing
        bad = np.ascontiguousarray(bad, dtype=np.int64)
        assert call(lib, b, soff=p(bad)) == ESIZE
    assert call(lib, b, toff=p(np.array([0, 36, 99], dtype=np.int64))) == ESIZE
    # the device entry refuses the same before it touches a device: no handle
    assert lib.fcpp_trip_solve(None, b.n, p(b.soff), p(b.soff), b.n_total, p(b.toff), p(b.toff), int(b.toff[-1]), p(b.T), p(b.length), None, None, p(b.In),
                               p(b.Out), b.C, p(b.tours), 1, p(b.Q), None, 0.0, *[None] * 10) == EINVAL


def test_every_output_may_be_null(lib):
    rng = np.random.default_rng(10)
    b = TC.batch(rng, [5, 0, 8], 2, 2.0)
    full = TC.twin(lib, b)
    sizes = TC.out_sizes(b)
    for left_out in TC.OUTPUTS:
        outs = {k: np.full(sizes[k], -7, dtype=TC.out_dtype(k)) for k in TC.OUTPUTS if k != left_out}
        assert TC.twin_call(lib, b, outs) == 0
        for k, a in outs.items():
            assert a.tobytes() == np.ascontiguousarray(full[k]).tobytes(), (left_out, k)


def test_results_do_not_depend_on_the_batch(lib):
    """a field solved alone gives what it gives among others (offsets that do not start at 0 in the tables)"""
    rng = np.random.default_rng(12)
    b = TC.batch(rng, [4, 9, 6], 3, 2.0, first=0.7, stop=2.0)
    r = TC.twin(lib, b)
    s0, s1 = int(b.soff[1]), int(b.soff[2])
    one = dataclasses.replace(b, soff=np.array([0, 9], dtype=np.int64), toff=np.array([0, 324], dtype=np.int64), T=b.T[int(b.toff[1]):int(b.toff[2])].copy(),
                              length=b.length[s0:s1].copy(), E=b.E[2 * s0:2 * s1].copy(), X=b.X[2 * s0:2 * s1].copy(), In=b.In[2 * s0:2 * s1].copy(),
                              Out=b.Out[2 * s0:2 * s1].copy(), tours=np.ascontiguousarray(b.tours[:, s0:s1]), Q=b.Q[1:2].copy(), Q0=b.Q0[1:2].copy())
    q = TC.twin(lib, one)
    assert q['tour'].tolist() == r['tour'][s0:s1].tolist() and q['trip'].tolist() == r['trip'][s0:s1].tolist()
    assert bits(q['costs'][0]).tolist() == bits(r['costs'][1]).tolist() and q['winner'][0] == r['winner'][1]
