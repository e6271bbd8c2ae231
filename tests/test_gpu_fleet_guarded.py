"""GPU tests of fcpp_fleet_solve through the guarded arena of tests/guarded.py (run with -m gpu on an MI355X): every buffer a slot of ONE uint8
CUDA tensor with 256 bytes of 0xA5 around it, outputs pre-filled with 0x5A, every pointer only naturally aligned and never 16-byte aligned.
After each call the guards are intact, the inputs have the bits that were put in, and every output element has the bits the host twin
(fcpp_debug_fleet_solve) gives -- none of which is the pre-fill pattern, so an element that was never written cannot pass: every element of
every field's outputs is written (the rows of the per-share outputs to their whole length, a failed field with candidate 0, zeros and NaN
costs), and nothing beside them.  Then every output is passed as NULL in turn: the others equal the full call's, and nothing else is
written.  Odd sizes: 0, 1, 67, 131, 513 and 7 swaths; the rows are 5 long, the most vehicles of a field."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import fleet_cases as FC
from tests.fleet_cases import OUTPUTS
from tests.guarded import Arena
from tests.support import lib          # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

INPUTS = ('soff', 'toff', 'T', 'length', 'In', 'Out', 'tours', 'K')


@pytest.fixture(scope='module')
def reference(lib):
    """per direction mode the batch and the twin's results: computed once and left unchanged"""
    out = {}
    for ways in (1, 0):
        rng = np.random.default_rng(21 + ways)
        b = FC.batch(rng, [0, 1, 67, 131, 513, 7], 3, [2, 3, 5, 4, 2, 3], omega=1.5, both_ways=ways, k_stride=5)
        b.length[int(b.soff[5]) + 2] = np.nan          # the last field: FCPP_EINVAL
        out[ways] = (b, FC.twin(lib, b))
    return out


@pytest.mark.parametrize('ways', [1, 0])
def test_fleet_solve_on_watched_buffers(reference, ways):
    import torch
    b, host = reference[ways]
    assert host['status'].tolist() == [0, 0, 0, 0, FC.EUNSUPPORTED, FC.EINVAL]
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    ctx.bind_stream()
    HP = E._host_ptr
    # (one direction mode has the library read the two offset tables back from the arena)
    hosts = (HP(b.soff), HP(b.toff)) if ways else (HP(None), HP(None))
    want = {k: np.ascontiguousarray(host[k], dtype=FC.out_dtype(k)).reshape(-1) for k in OUTPUTS}
    for left_out in (None,) + OUTPUTS:
        outs = [k for k in OUTPUTS if k != left_out]
        A = Arena()
        for name in INPUTS:
            A.input(name, getattr(b, name))
        for k in outs:
            A.output(k, FC.out_dtype(k), want[k].size)
        A.build(dev)
        L.check(ctx.lib.fcpp_fleet_solve(ctx.handle, b.n, A.ptr('soff'), hosts[0], b.n_total, A.ptr('toff'), hosts[1], int(b.toff[-1]), A.ptr('T'),
                                         A.ptr('length'), A.ptr('In'), A.ptr('Out'), b.C, A.ptr('tours'), b.both_ways, A.ptr('K'), b.k_stride, b.omega,
                                         *[A.ptr(k) for k in OUTPUTS]))
        A.check({k: want[k] for k in outs})
