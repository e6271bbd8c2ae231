"""GPU tests of the vehicle shares (run with -m gpu on an MI355X): fcpp_fleet_solve against its host twin (fcpp_debug_fleet_solve) BYTE FOR BYTE
on synthetic tables -- tour, share, n_used, winner, status, makespan, total, both value rows, share_first and share_cost -- over one batch of
fields of 0, 1, 2, 3, 17, 63, 64, 65, 66, 130, 257, 512 and 513 swaths.  The twin itself is held to every composition in
tests/test_fleet_host.py.

The kernel's strided loops and what drives each into a second round (DESIGN.md section 4 lists them):
  a wavefront's lane loops over positions (tables, validation)       m >= 65
  a layer's rounds of 64 end positions j                             m >= 65 (two rounds), m = 512 (eight)
  the workgroup's loops over positions (lengths, tour, share)        m = 257, 512; the failed field's: m = 513
  candidates over the four wavefronts (validation)                   C = 8
  variants over the four wavefronts                                  C = 3 (6 variants), C = 8 (16; 8 with both_ways = 0)
  the layers                                                         K in {1, 2, 3, 16, 17 (unsupported)}, K > m (m = 1, 2, 3 at K = 2, 16, 16)
The rows of the per-share outputs: k_stride = max K (3) and 16.  both_ways 0 and 1, omega 0, 1 and 2.5, whole-number tables (ties).
The two instances of the kernel (a batch's largest field up to 192 swaths, or beyond): batches that end at 192 and at 193 swaths.
The 512-swath field keeps K C small -- K = 16 at C = 3, K = 3 at C = 8 -- so that the twin finishes within a few seconds.
"""
import dataclasses

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import fleet_cases as FC
from tests.fleet_cases import KINDS, OUTPUTS, poisoned
from tests.support import lib          # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

MS = [0, 1, 2, 3, 17, 63, 64, 65, 66, 130, 257, 512, 513]
K_WIDE = [3, 2, 16, 16, 17, 16, 2, 3, 16, 1, 3, 16, 4]          # per field of MS: K > m at m = 1, 2, 3; 17 is one too many
K_NARROW = [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2]              # max K = 3: the rows' length


def device_fleet(b, host_tables=True, left_out=()):
    """fcpp_fleet_solve on torch tensors -> {output: numpy array} like fleet_cases.twin (an output in left_out is passed as NULL)"""
    import torch
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    P, HP = E._ptr, E._host_ptr
    soff, toff = up(b.soff), up(b.toff)
    ins = [up(a) for a in (b.T, b.length, b.In, b.Out)]
    tours, K = up(b.tours), up(b.K)
    sizes = FC.out_sizes(b)
    out = {k: torch.full((sizes[k],), -7, dtype=torch.int32 if k in FC.OUT_I32 else torch.float64, device=dev) for k in OUTPUTS if k not in left_out}
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_fleet_solve(ctx.handle, b.n, P(soff), HP(b.soff if host_tables else None), b.n_total, P(toff), HP(b.toff if host_tables else None),
                                     int(b.toff[-1]), *[P(t) for t in ins], b.C, P(tours), b.both_ways, P(K), b.k_stride, b.omega,
                                     *[P(out.get(k)) for k in OUTPUTS]))
    return FC.shaped(b, {k: v.cpu().numpy() for k, v in out.items()})


def assert_same(dev, host):
    for k in dev:
        assert dev[k].tobytes() == np.ascontiguousarray(host[k]).tobytes(), k


#        C  K         k_stride  both  omega  whole numbers
CASES = [(3, K_WIDE, 16, 1, 1.0, False),
         (8, K_NARROW, 3, 1, 0.0, False),
         (8, K_NARROW, 16, 0, 2.5, False),
         (3, K_WIDE, 16, 0, 0.0, True),
         (1, K_NARROW, 3, 1, 2.5, True)]


@pytest.mark.parametrize('case', range(len(CASES)), ids=['C%d-K%d-rows%d-ways%d-w%g-whole%d' % (c[0], max(c[1]), c[2], c[3], c[4], c[5]) for c in CASES])
def test_every_size_matches_the_twin(lib, case):
    C, K, k_stride, both, omega, whole = CASES[case]
    rng = np.random.default_rng(100 + case)
    b = FC.batch(rng, MS, C, K, omega=omega, both_ways=both, k_stride=k_stride, integer=whole, blocked=case == 2)
    host = FC.twin(lib, b)
    dev = device_fleet(b, host_tables=case % 2 == 0)
    assert_same(dev, host)
    # what the case is there for did happen
    want = [0] * 12 + [FC.EUNSUPPORTED]
    if K is K_WIDE:
        want[4] = FC.EUNSUPPORTED
    assert host['status'].tolist() == want
    ok = host['status'] == 0
    m, Kf = np.asarray(MS), np.asarray(K)
    assert (host['n_used'][ok] <= np.minimum(m, Kf)[ok]).all() and (host['n_used'][ok & (m >= 17)] >= np.minimum(2, Kf[ok & (m >= 17)])).all()
    if K is K_WIDE:
        assert host['n_used'][11] >= 8          # (512 swaths among 16 vehicles: most of them drive)


@pytest.mark.parametrize('last', [192, 193])
def test_both_instances_of_the_kernel(lib, last):
    """a batch whose largest field has 192 swaths runs the small instance, at its cap; one swath more, the large one"""
    rng = np.random.default_rng(last)
    b = FC.batch(rng, [0, 1, 5, 64, 65, 130, 600, last], 3, [2, 3, 7, 3, 16, 2, 2, 5], omega=1.5)
    host = FC.twin(lib, b)
    assert host['status'].tolist() == [0] * 6 + [FC.EUNSUPPORTED, 0] and host['n_used'][7] == 5
    assert_same(device_fleet(b, host_tables=last == 192), host)


@pytest.mark.parametrize('kind', KINDS)
def test_one_bad_field_among_good_ones(lib, kind):
    b, status = poisoned(kind)
    for ways in (1, 0):
        b = dataclasses.replace(b, both_ways=ways)
        host = FC.twin(lib, b)
        assert host['status'].tolist() == [0, status, 0]
        assert_same(device_fleet(b, host_tables=ways == 1), host)          # (one direction: the library reads the device offsets back)


def test_results_when_outputs_are_left_out(lib):
    rng = np.random.default_rng(7)
    b = FC.batch(rng, [5, 0, 70, 600, 9], 3, [2, 4, 5, 3, 12], k_stride=12)
    host = FC.twin(lib, b)
    for left_out in OUTPUTS:
        dev = device_fleet(b, left_out=(left_out,))
        assert left_out not in dev and len(dev) == len(OUTPUTS) - 1
        assert_same(dev, host)
