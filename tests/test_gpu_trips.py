"""GPU tests of the service trips (run with -m gpu on an MI355X): fcpp_trip_solve against its host twin (fcpp_debug_trip_solve) BYTE FOR BYTE
on synthetic tables -- tour, trip, n_trips, overfull, winner, status, cost, base, extra and the whole cost row -- over one batch of fields of
0, 1, 2, 3, 17, 63, 64, 65, 66, 130, 512 and 513 swaths.  The twin itself is held to every stop set in tests/test_trips_host.py.

The kernel's strided loops and what drives each into a second round (DESIGN.md section 4 lists them):
  a wavefront's lane loops over positions (tables, marks, ballots)   m >= 65
  the workgroup's loops over positions (lengths, the tour)           m = 512; the failed field's: m = 513
  candidates over the four wavefronts (validation)                   C = 8
  variants over the four wavefronts                                  C = 3 (6 variants), C = 8 (16)
  the window's lanes                                                 m >= 66 at a capacity of 65.5 equal swaths (a window of 65 or 66
                                                                     starts), m >= 66 at +inf (up to 8 rounds)
"""
import dataclasses

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import trip_cases as TC
from tests.support import lib          # noqa: F401 (a fixture)
from tests.trip_cases import INF, KINDS, OUTPUTS, poisoned

pytestmark = pytest.mark.gpu

MS = [0, 1, 2, 3, 17, 63, 64, 65, 66, 130, 512, 513]
CAPACITIES = {'inf': INF, '65.5 swaths': 65.5, '2.5 swaths': 2.5, 'below every swath': 1.0}          # in mean swaths (the last: set in metres)


def device_trips(b, host_tables=True, left_out=()):
    """fcpp_trip_solve on torch tensors -> {output: numpy array} like trip_cases.twin (an output in left_out is passed as NULL)"""
    import torch
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    P, HP = E._ptr, E._host_ptr
    soff, toff = up(b.soff), up(b.toff)
    ins = [up(a) for a in (b.T, b.length, b.E, b.X, b.In, b.Out)]
    tours, Q, Q0 = up(b.tours), up(b.Q), up(b.Q0)
    sizes = TC.out_sizes(b)
    out = {k: torch.full((sizes[k],), -7, dtype=torch.int32 if k in TC.OUT_I32 else torch.float64, device=dev) for k in OUTPUTS if k not in left_out}
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_trip_solve(ctx.handle, b.n, P(soff), HP(b.soff if host_tables else None), b.n_total, P(toff), HP(b.toff if host_tables else None),
                                    int(b.toff[-1]), *[P(t) for t in ins], b.C, P(tours), b.both_ways, P(Q), P(Q0), b.stop,
                                    *[P(out.get(k)) for k in OUTPUTS]))
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if 'costs' in res:
        res['costs'] = res['costs'].reshape(b.n, 2 * b.C)
    return res


def assert_same(dev, host):
    for k in dev:
        assert dev[k].tobytes() == np.ascontiguousarray(host[k]).tobytes(), k


def size_batch(C, capacity, case):
    """the batch of every size; the other axes turn with the case's number"""
    rng = np.random.default_rng(100 + case)
    equal = capacity in ('65.5 swaths', 'inf')          # swaths of 10 m each and no stop that pays: the trips' number is known
    smaller_first = (case + case // 4) % 2 == 0 and not equal
    b = TC.batch(rng, MS, C, CAPACITIES[capacity], first=0.6 if smaller_first else None, ends=case % 3 != 0, stop=7.5 if case % 2 else 0.0,
                 both_ways=0 if case % 5 == 1 else 1, swath=10.0 if equal else None, metric=equal)
    if capacity == 'below every swath':          # (the shortest swath is 5 m)
        b.Q[:] = 4.0
        if b.Q0 is not None:
            b.Q0[:] = 2.0
    return b


CASES = [(C, cap) for C in (1, 3, 8) for cap in CAPACITIES]


@pytest.mark.parametrize('case', range(len(CASES)), ids=['C%d-%s' % c for c in CASES])
def test_every_size_matches_the_twin(lib, case):
    C, capacity = CASES[case]
    b = size_batch(C, capacity, case)
    host = TC.twin(lib, b)
    dev = device_trips(b, host_tables=case % 2 == 0)
    assert_same(dev, host)
    # what the case is there for did happen
    ok = host['status'] == 0
    assert host['status'].tolist() == [0] * 11 + [TC.EUNSUPPORTED]
    m = np.asarray(MS)
    if capacity == 'inf':
        assert (host['n_trips'][ok] == np.minimum(m[ok], 1)).all()
    elif capacity == '65.5 swaths':
        # 65 swaths fit a trip; the cheapest split may make more stops than it must where the forced ones are dear
        assert host['n_trips'][ok][:9].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 2] and host['n_trips'][9] >= 2 and host['n_trips'][10] >= 8
        assert not host['overfull'].any()
    elif capacity == '2.5 swaths':
        assert (host['n_trips'][ok & (m >= 17)] > m[ok & (m >= 17)] // 4).all()          # (a trip holds 2.5 mean swaths)
    else:
        assert (host['n_trips'][ok] == m[ok]).all() and (host['overfull'][ok] == m[ok]).all()


@pytest.mark.parametrize('kind', KINDS)
def test_one_bad_field_among_good_ones(lib, kind):
    b, status = poisoned(kind)
    for ways in (1, 0):
        b = dataclasses.replace(b, both_ways=ways)
        host = TC.twin(lib, b)
        assert host['status'].tolist() == [0, status, 0]
        assert_same(device_trips(b), host)


def test_results_when_outputs_are_left_out(lib):
    rng = np.random.default_rng(7)
    b = TC.batch(rng, [5, 0, 70, 600, 9], 3, 2.5, first=0.5)
    host = TC.twin(lib, b)
    for left_out in OUTPUTS:
        dev = device_trips(b, left_out=(left_out,))
        assert left_out not in dev and len(dev) == len(OUTPUTS) - 1
        assert_same(dev, host)
