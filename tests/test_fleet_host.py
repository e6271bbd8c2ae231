"""CPU-side tests of the vehicle shares: the two entries exist (header, ctypes binding, libfcpp.so; ABI version still 5), the call's errors
need no device -- and the RULE, through fcpp_debug_fleet_solve (csrc/fcpp_fleetfn.h on the host: the very expressions the kernel runs).

The checker shares no code with the library (tests/fleet_cases.py): the tables of a tour restated in Python floats from include/fcpp.h -- a
sum of two doubles rounds like the library's (-ffp-contract=off), so "to the bit" is meant literally -- and EVERY composition of every
variant's tour into at most K shares, for m <= 10: the least largest share cost, then the least rounded sum among those within it."""
import dataclasses

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests.fleet_cases import EINVAL, INF, KINDS, poisoned
from tests.support import bits, check_entries, lib, p          # noqa: F401 (lib: a fixture)

ENTRIES = {'fcpp_fleet_solve': 29, 'fcpp_debug_fleet_solve': 26}
ESIZE = -6


def test_header_binding_and_abi(lib):
    header = check_entries(ENTRIES, lib)
    assert 'vehicle shares' in header and 'csrc/fcpp_fleetfn.h' in header and '#define FCPP_FLEET_MAX_VEHICLES 16' in header


# ---- what every divided field must give -------------------------------------------------------------------------------------------------
def check_field(b, r, f, rows=None):
    """field f of the twin's results r against the rule, restated: the value rows (where the oracle's are given), the winner, the tour, and
    that the returned shares partition the tour and cost what share_cost, makespan and total say"""
    T, length, In, Out, tours = b.field(f)
    s0, m, K = int(b.soff[f]), b.m(f), int(b.K[f])
    Ms, sums = r['makespans'][f], r['totals'][f]
    assert r['status'][f] == 0
    if rows is not None:
        assert bits(Ms).tolist() == bits(rows[0]).tolist(), (f, Ms, rows[0])
        assert bits(sums).tolist() == bits(rows[1]).tolist(), (f, sums, rows[1])
    exists = [v for v in range(2 * b.C) if b.both_ways or v % 2 == 0]
    assert all(np.isnan(Ms[v]) and np.isnan(sums[v]) for v in range(2 * b.C) if v not in exists)
    win = int(r['winner'][f])
    assert win == min(exists, key=lambda v: (Ms[v], sums[v], v))          # the least (M, sum, v)
    assert bits(r['makespan'][f]) == bits(Ms[win]) and bits(r['total'][f]) == bits(sums[win])
    t = FC.variant(tours[win >> 1], win & 1)
    assert r['tour'][s0:s0 + m].tolist() == t.tolist()
    share = r['share'][s0:s0 + m]
    used = int(r['n_used'][f])
    first, cost = r['share_first'][f], r['share_cost'][f]
    assert used <= min(K, m)
    assert (first[used:] == -1).all() and np.isnan(cost[used:]).all()
    if m == 0:
        assert used == 0 and r['makespan'][f] == 0.0 and r['total'][f] == 0.0
        return
    # the shares partition the tour: indices from 0, never decreasing, none skipped; share_first names where each begins
    assert share[0] == 0 and share[-1] == used - 1 and set(np.diff(share).tolist()) <= {0, 1}
    firsts = [0] + [j for j in range(1, m) if share[j] != share[j - 1]]
    assert first[:used].tolist() == firsts
    P, S = FC.tables(t, T, length)
    costs = FC.split_costs(t, P, S, In, Out, b.omega, firsts)
    assert bits(cost[:used]).tolist() == bits(costs).tolist()
    assert bits(max(costs)) == bits(r['makespan'][f]) and bits(FC.rounded_sum(costs)) == bits(r['total'][f])


# ---- random fields against every composition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('omega', [0.0, 1.0, 2.5])
@pytest.mark.parametrize('both_ways', [1, 0])
@pytest.mark.parametrize('tables', ['random', 'integer', 'blocked'])
def test_random_fields_against_all_compositions(lib, omega, both_ways, tables):
    rng = np.random.default_rng(11 + int(2 * omega) + both_ways + 7 * len(tables))
    ms = np.concatenate([np.arange(11), rng.integers(1, 11, 19)])
    K = np.concatenate([np.arange(11) % 6 + 1, rng.integers(1, 7, 19)])
    C = int(rng.integers(1, 5)) if tables != 'blocked' else 2
    b = FC.batch(rng, ms, C, K, omega=omega, both_ways=both_ways, integer=tables != 'random', blocked=tables == 'blocked')
    r = FC.twin(lib, b)
    fewer = beyond = infinite = 0
    for f in range(b.n):
        check_field(b, r, f, FC.field_rows(b, f))
        fewer += r['n_used'][f] < min(b.K[f], b.m(f))
        beyond += b.K[f] > b.m(f)
        infinite += np.isinf(r['makespans'][f]).any()
    print('fields', b.n, 'C', C, 'with fewer shares than vehicles', fewer, 'with more vehicles than swaths', beyond, 'with an infinite variant', infinite)
    assert beyond > 0 and (tables != 'blocked' or infinite > 0)


def test_a_further_vehicle_never_hurts_and_may_stay_home(lib):
    rng = np.random.default_rng(2)
    ms = rng.integers(1, 11, 24)
    b = FC.batch(rng, ms, 2, 1)
    last, home = None, 0
    for K in range(1, 8):
        b.K[:] = K
        r = FC.twin(lib, b)
        for f in range(b.n):
            check_field(b, r, f, FC.field_rows(b, f) if K in (1, 4) else None)
        if last is not None:
            assert (r['makespan'] <= last).all()
        last = r['makespan'].copy()
        home += int((r['n_used'] < np.minimum(K, ms)).sum())
    print('fields that left a vehicle at home, summed over K', home)
    assert home > 0          # (a further vehicle adds its own ways in and out: "at most K" matters)


def test_one_vehicle_is_one_share_over_the_tour(lib):
    rng = np.random.default_rng(3)
    b = FC.batch(rng, [1, 4, 9, 10], 3, 1, omega=2.5)
    r = FC.twin(lib, b)
    assert r['n_used'].tolist() == [1, 1, 1, 1] and not r['share'].any() and r['share_first'][:, 0].tolist() == [0] * 4
    for f in range(b.n):
        T, length, In, Out, tours = b.field(f)
        for v in range(2 * b.C):
            t = FC.variant(tours[v >> 1], v & 1)
            P, S = FC.tables(t, T, length)
            c = FC.share_cost(t, P, S, In, Out, b.omega, 0, b.m(f))
            assert bits(r['makespans'][f, v]) == bits(c) and bits(r['totals'][f, v]) == bits(c)
        check_field(b, r, f)
        assert bits(r['share_cost'][f, 0]) == bits(r['makespan'][f])


def test_no_swath_and_one_swath(lib):
    rng = np.random.default_rng(6)
    b = FC.batch(rng, [0, 1, 0], 2, [3, 3, 1], k_stride=3)
    r = FC.twin(lib, b)
    assert r['status'].tolist() == [0, 0, 0] and r['n_used'].tolist() == [0, 1, 0] and r['winner'][0] == 0 and r['winner'][2] == 0
    assert bits(r['makespans'][0]).tolist() == [0] * 4 and bits(r['totals'][2]).tolist() == [0] * 4
    assert r['share_first'].tolist() == [[-1] * 3, [0, -1, -1], [-1] * 3] and r['share_cost'].shape == (3, 3)
    for f in range(3):
        check_field(b, r, f, FC.field_rows(b, f))


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------
def even_field(m, K, C=1):
    """m swaths of 10 m in stored order, every transit 4, every way to and from the depot 5"""
    rng = np.random.default_rng(0)
    b = FC.batch(rng, [m], C, K)
    b.T[np.isfinite(b.T)] = 4.0
    b.length[:] = 10.0
    b.In[:] = 5.0
    b.Out[:] = 5.0
    b.tours[:] = 2 * np.arange(m)
    return b


def test_equal_sums_go_to_the_lowest_start(lib):
    # a share of q swaths costs 10 + 4 (q - 1) + 10 q.  Five swaths, two vehicles: 3 + 2 or 2 + 3, M = 48 either way and both sums 82.  The
    # last share's start is picked ascending with a strict "less than": 2, so the shares are {0, 1}, {2, 3, 4}
    b = even_field(5, 2)
    r = FC.twin(lib, b)
    assert r['makespan'][0] == 48.0 and r['total'][0] == 82.0 and r['share'].tolist() == [0, 0, 1, 1, 1]
    check_field(b, r, 0, FC.field_rows(b, 0))
    # three vehicles: 2 + 2 + 1, 2 + 1 + 2 or 1 + 2 + 2, all M = 34 and sum 88: the last start is 3 (of 3, 4), then 1 (of 1, 2)
    b = even_field(5, 3)
    r = FC.twin(lib, b)
    assert r['makespan'][0] == 34.0 and r['total'][0] == 88.0 and r['share'].tolist() == [0, 1, 1, 2, 2]
    check_field(b, r, 0, FC.field_rows(b, 0))


def test_equal_variants_go_to_the_lowest(lib):
    # two candidates that are one tour; every table is symmetric, so backwards costs the same too: four equal pairs -> variant 0
    b = even_field(5, 2, C=2)
    r = FC.twin(lib, b)
    assert len(set(bits(r['makespans'][0]).tolist())) == 1 and len(set(bits(r['totals'][0]).tolist())) == 1 and r['winner'][0] == 0
    # the second candidate is the first one backwards, and the first transit of that tour is made cheaper: 3 + 2 swaths now cost 47 and 34.
    # Candidate 0 backwards (v = 1) is candidate 1 as given (v = 2): they tie in M and in the sum, and the lower v wins
    b.tours[1] = b.tours[0][::-1] ^ 1
    b.T.reshape(10, 10)[9, 7] = 3.0
    r = FC.twin(lib, b)
    assert r['makespans'][0].tolist() == [48.0, 47.0, 47.0, 48.0] and r['totals'][0].tolist() == [82.0, 81.0, 81.0, 82.0] and r['winner'][0] == 1
    assert r['tour'].tolist() == [9, 7, 5, 3, 1] and r['share'].tolist() == [0, 0, 0, 1, 1]
    check_field(b, r, 0, FC.field_rows(b, 0))


# ---- the statuses -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_status_of_one_field_among_good_ones(lib, kind):
    b, status = poisoned(kind)
    r = FC.twin(lib, b)
    s0, s1 = int(b.soff[1]), int(b.soff[2])
    assert r['status'].tolist() == [0, status, 0]
    assert r['tour'][s0:s1].tolist() == b.tours[0, s0:s1].tolist() and not r['share'][s0:s1].any()
    assert r['n_used'][1] == 1 and r['winner'][1] == 0
    assert np.isnan(r['makespans'][1]).all() and np.isnan(r['totals'][1]).all() and np.isnan([r['makespan'][1], r['total'][1]]).all()
    assert r['share_first'][1].tolist() == [0] + [-1] * (b.k_stride - 1) and np.isnan(r['share_cost'][1]).all()
    for f in (0, 2):
        check_field(b, r, f, FC.field_rows(b, f))


def test_a_later_candidate_with_an_infinite_transit_only_loses(lib):
    b, _ = poisoned('none')
    s0 = int(b.soff[1])
    b.tours[0, s0:s0 + 7] = 2 * np.arange(7)
    b.tours[1, s0:s0 + 7] = [0, 4, 8, 12, 2, 6, 10]
    # a NaN transit from swath 4 to swath 6, both forwards: candidate 1 drives it, neither direction of candidate 0 does, nor candidate 1 backwards
    b.T[int(b.toff[1]):int(b.toff[2])].reshape(14, 14)[8, 12] = np.nan
    r = FC.twin(lib, b)
    assert r['status'][1] == 0 and r['makespans'][1, 2] == INF and np.isfinite(r['makespans'][1, [0, 1, 3]]).all() and r['winner'][1] != 2
    check_field(b, r, 1, FC.field_rows(b, 1))


# ---- the call's errors ------------------------------------------------------------------------------------------------------------------
def call(lib, b, **kw):
    """fcpp_debug_fleet_solve with arguments replaced by name"""
    a = dict(n=b.n, soff=p(b.soff), n_total=b.n_total, toff=p(b.toff), t_total=int(b.toff[-1]), T=p(b.T), length=p(b.length), In=p(b.In), Out=p(b.Out),
             C=b.C, tours=p(b.tours), both_ways=b.both_ways, K=p(b.K), k_stride=b.k_stride, omega=b.omega)
    a.update(kw)
    return lib.fcpp_debug_fleet_solve(*a.values(), *[None] * 11)


def test_call_errors(lib):
    rng = np.random.default_rng(9)
    b = FC.batch(rng, [3, 4], 2, 2)
    assert call(lib, b) == 0
    for name in ('soff', 'toff', 'T', 'length', 'In', 'Out', 'tours', 'K'):
        assert call(lib, b, **{name: None}) == EINVAL, name
    for C in (0, -1, 65):
        assert call(lib, b, C=C) == EINVAL
    for omega in (-1.0, np.nan, INF, -INF):
        assert call(lib, b, omega=omega) == EINVAL
    assert call(lib, b, omega=0.0) == 0
    for stride in (0, -1, 17):
        assert call(lib, b, k_stride=stride) == EINVAL
    for ways in (-1, 2):
        assert call(lib, b, both_ways=ways) == EINVAL
    assert call(lib, b, n_total=-1) == ESIZE and call(lib, b, n=-1) == ESIZE and call(lib, b, t_total=-1) == ESIZE
    assert call(lib, b, n_total=b.n_total + 1) == ESIZE and call(lib, b, t_total=int(b.toff[-1]) + 4) == ESIZE
    for bad in (b.soff + 1, [0, 5, 7], [0, 4, 3]):          # not from 0; other counts than the blocks'; decreasing
        bad = np.ascontiguousarray(bad, dtype=np.int64)
        assert call(lib, b, soff=p(bad)) == ESIZE
    assert call(lib, b, toff=p(np.array([0, 36, 99], dtype=np.int64))) == ESIZE
    # the device entry refuses the same before it touches a device: no handle
    assert lib.fcpp_fleet_solve(None, b.n, p(b.soff), p(b.soff), b.n_total, p(b.toff), p(b.toff), int(b.toff[-1]), p(b.T), p(b.length), p(b.In), p(b.Out),
                                b.C, p(b.tours), 1, p(b.K), 16, 1.0, *[None] * 11) == EINVAL


def test_every_output_may_be_null(lib):
    rng = np.random.default_rng(10)
    b = FC.batch(rng, [5, 0, 8], 2, [2, 1, 3], k_stride=3)
    full = FC.twin(lib, b)
    sizes = FC.out_sizes(b)
    for left_out in FC.OUTPUTS:
        outs = {k: np.full(sizes[k], -7, dtype=FC.out_dtype(k)) for k in FC.OUTPUTS if k != left_out}
        assert FC.twin_call(lib, b, outs) == 0
        for k, a in outs.items():
            assert a.tobytes() == np.ascontiguousarray(full[k]).tobytes(), (left_out, k)


def test_results_do_not_depend_on_the_batch(lib):
    """a field solved alone gives what it gives among others (offsets that do not start at 0 in the tables)"""
    rng = np.random.default_rng(12)
    b = FC.batch(rng, [4, 9, 6], 3, [2, 3, 4], omega=0.5)
    r = FC.twin(lib, b)
    s0, s1 = int(b.soff[1]), int(b.soff[2])
    one = dataclasses.replace(b, soff=np.array([0, 9], dtype=np.int64), toff=np.array([0, 324], dtype=np.int64), T=b.T[int(b.toff[1]):int(b.toff[2])].copy(),
                              length=b.length[s0:s1].copy(), In=b.In[2 * s0:2 * s1].copy(), Out=b.Out[2 * s0:2 * s1].copy(),
                              tours=np.ascontiguousarray(b.tours[:, s0:s1]), K=b.K[1:2].copy())
    q = FC.twin(lib, one)
    assert q['tour'].tolist() == r['tour'][s0:s1].tolist() and q['share'].tolist() == r['share'][s0:s1].tolist()
    assert bits(q['makespans'][0]).tolist() == bits(r['makespans'][1]).tolist() and bits(q['totals'][0]).tolist() == bits(r['totals'][1]).tolist()
    assert q['winner'][0] == r['winner'][1] and bits(q['share_cost'][0]).tolist() == bits(r['share_cost'][1]).tolist()
