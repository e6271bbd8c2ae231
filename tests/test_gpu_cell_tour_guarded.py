"""GPU tests of the cell tour's entries through the guarded arena of tests/guarded.py (run with -m gpu on an MI355X): every buffer a slot
of ONE uint8 CUDA tensor with 256 bytes of 0xA5 around it, outputs pre-filled with 0x5A, every pointer only naturally aligned and never
16-byte aligned.  After each call the guards are intact, the inputs have the bits that were put in, and every output element has the bits
the host twin (fcpp_debug_cell_tour) gives -- none of which is the pre-fill pattern, so an element that was never written cannot pass:
every element of every field's outputs is written (a field beyond a cap writes its stored order and NaN costs), and nothing beside them.
Then every output is passed as NULL in turn: the others equal the full call's, and nothing else is written."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import tour_cases as TC
from tests.guarded import Arena
from tests.test_gpu_cell_tour import R, mixed_scene, poses_for, stored_nodes
from tests.tour_cases import OUTPUTS

pytestmark = pytest.mark.gpu

S = 4
DTYPES = {k: np.int32 for k in TC.OUT_I32}
DTYPES.update({k: np.float64 for k in TC.OUT_F64})


@pytest.fixture(scope='module')
def reference():
    """the mixed batch, per mode its gate costs and the twin's results: computed once and left unchanged"""
    sc = mixed_scene()
    entry, exit = poses_for(sc)
    sn = stored_nodes(sc, 41)
    out = {}
    for mode in (0, 1):
        En, Xn = TC.gate_costs(sc, entry, exit, R, mode)
        out[mode] = (En, Xn, TC.twin(sc, R, mode, E=En, X=Xn, stored_node=sn, S=S, max_sweeps=3))
    return sc, sn, out


def _inputs(A, sc):
    A.input('coff', sc.coff).input('voff', sc.voff).input('doff', sc.doff)
    return A


@pytest.mark.parametrize('mode', [0, 1])
def test_cell_tour_on_watched_buffers(reference, mode):
    import torch
    sc, sn, per_mode = reference
    En, Xn, host = per_mode[mode]
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    ctx.bind_stream()
    HP = E._host_ptr
    # (mode 1 has the library read the three offset tables back from the arena)
    hosts = (HP(sc.coff), HP(sc.voff), HP(sc.doff)) if mode == 0 else (HP(None), HP(None), HP(None))
    d_total = int(sc.doff[-1])
    A = _inputs(Arena(), sc)
    for name, a in zip(('ix', 'iy', 'ih', 'ox', 'oy', 'oh'), sc.poses()):
        A.input(name, a)
    A.output('D', np.float64, d_total).build(dev)
    head = lambda A: (sc.n, A.ptr('coff'), hosts[0], sc.n_cells, A.ptr('voff'), hosts[1], sc.n_vars)
    L.check(ctx.lib.fcpp_cell_tour_transit(ctx.handle, *head(A), *[A.ptr(k) for k in ('ix', 'iy', 'ih', 'ox', 'oy', 'oh')], R, mode, A.ptr('doff'), hosts[2],
                                           d_total, A.ptr('D')))
    A.check({'D': host['D']})
    want = {k: np.ascontiguousarray(host[k], dtype=DTYPES[k]).reshape(-1) for k in OUTPUTS}
    for left_out in (None,) + OUTPUTS:
        outs = [k for k in OUTPUTS if k != left_out]
        A = _inputs(Arena(), sc)
        A.input('w', sc.w).input('sn', sn).input('D', host['D']).input('E', En).input('X', Xn)
        for k in outs:
            A.output(k, DTYPES[k], want[k].size)
        A.build(dev)
        L.check(ctx.lib.fcpp_cell_tour_solve(ctx.handle, *head(A), A.ptr('w'), A.ptr('sn'), A.ptr('doff'), hosts[2], d_total, A.ptr('D'), A.ptr('E'),
                                             A.ptr('X'), S, TC.MIN_GAIN, 3, *[A.ptr(k) for k in OUTPUTS]))
        A.check({k: want[k] for k in outs})
