"""GPU tests of the cell tour (run with -m gpu on an MI355X): the kernels of csrc/fcpp_tour.hip against the same rule on the host
(fcpp_debug_cell_tour) BIT FOR BIT -- the joint blocks, order, node, cost, stored cost, joint length, winner, sweeps, skipped, status and
every candidate's order and cost -- in both modes.  The layers are summed a ascending with a strict "less than" on both sides and the
minimum over (cost, code) pairs does not depend on how the device hands the moves to its wavefronts, so nothing is compared to a bound.

The shapes, the smallest at which a loop can go wrong: k = 0, 1, 2, 3 kept cells; k = 5 (more moves than the four wavefronts take in one
round); k = 32 at one variant per cell (the cell cap) and k = 33 (over it); a cell of 32 variants -- 64 nodes, every lane a target --
beside cells of 1, and one of 33 (over the cap); 16 cells x 32 variants, N_f = 1024, the block cap, with one candidate and one sweep so
that the twin stays within a few seconds, and 27 x 19, N_f = 1026, over it; a batch that mixes every status with an empty field first and
last; 1, 2 and 8 candidates; max_sweeps 0; and cells.cell_tour on a batch that a small budget splits into chunks."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import cells as CL
from field_coverage_path_planning_amd import engine as E
from tests import tour_cases as TC
from tests.support import np_of as _np
from tests.tour_cases import OUTPUTS, Scene, bits

pytestmark = pytest.mark.gpu

R = 6.0


def mixed_scene():
    rng = np.random.default_rng(31)
    nan_field = TC.grid_field(rng, [2, 1, 2])
    nan_field[1][0] = ((float('nan'), 3.0, 0.1), nan_field[1][0][1], 5.0)
    return Scene([[],                                          # an empty field first
                  TC.grid_field(rng, [2]),                     # k = 1
                  TC.grid_field(rng, [2, 3]),                  # k = 2
                  TC.grid_field(rng, [1, 0, 2, 3]),            # k = 3 and a skipped cell
                  TC.grid_field(rng, [1] * 33),                # over the cell cap
                  TC.grid_field(rng, [3, 2, 1, 2, 3]),         # k = 5
                  nan_field,                                   # FCPP_EINVAL
                  TC.grid_field(rng, [1, 33, 1]),              # a cell over its cap
                  TC.grid_field(rng, [0, 0]),                  # k = 0 of two cells
                  TC.grid_field(rng, [1, 32, 1, 2]),           # every lane a target
                  TC.grid_field(rng, [19] * 27),               # over the block cap
                  TC.grid_field(rng, [2, 2, 2, 2, 2, 2, 2]),   # k = 7
                  []])                                         # and an empty field last


def cap_cells_scene():
    rng = np.random.default_rng(32)
    return Scene([TC.grid_field(rng, [1] * 32)])


def cap_block_scene():
    rng = np.random.default_rng(33)
    return Scene([TC.grid_field(rng, [32] * 16)])


def poses_for(sc):
    k = np.arange(sc.n, dtype=np.float64)
    return np.column_stack([-15.0 - k, -10.0 + 0.5 * k, 0.3 + 0.01 * k]), np.column_stack([230.0 + k, 210.0 - 0.5 * k, 1.2 - 0.01 * k])


def stored_nodes(sc, seed):
    rng = np.random.default_rng(seed)
    return np.asarray([rng.integers(0, max(1, 2 * v)) for v in np.diff(sc.voff)], dtype=np.int32)


def device_tour(sc, mode, En=None, Xn=None, sn=None, S=8, min_gain=TC.MIN_GAIN, max_sweeps=None, host_tables=True):
    """fcpp_cell_tour_transit + fcpp_cell_tour_solve on torch tensors -> dict of numpy arrays like tour_cases.twin"""
    import torch
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    HP = E._host_ptr
    co, vo, do = up(sc.coff), up(sc.voff), up(sc.doff)
    hosts = (sc.coff, sc.voff, sc.doff) if host_tables else (None, None, None)
    poses = [up(a) for a in sc.poses()]
    w, sn_d, E_d, X_d = up(sc.w), up(sn), up(En), up(Xn)
    if max_sweeps is None:
        max_sweeps = TC.default_sweeps(sc)
    host = TC.outputs(sc, S)
    out = {k: up(v) for k, v in host.items()}
    D = torch.full((int(sc.doff[-1]),), -7.0, dtype=torch.float64, device=dev)
    ctx.bind_stream()
    P = E._ptr
    head = (sc.n, P(co), HP(hosts[0]), sc.n_cells, P(vo), HP(hosts[1]), sc.n_vars)
    L.check(ctx.lib.fcpp_cell_tour_transit(ctx.handle, *head, *[P(p) for p in poses], R, mode, P(do), HP(hosts[2]), int(sc.doff[-1]), P(D)))
    L.check(ctx.lib.fcpp_cell_tour_solve(ctx.handle, *head, P(w), P(sn_d), P(do), HP(hosts[2]), int(sc.doff[-1]), P(D), P(E_d), P(X_d), S, float(min_gain),
                                         int(max_sweeps), *[P(out[k]) for k in OUTPUTS]))
    res = {k: _np(v) for k, v in out.items()}
    res['D'] = _np(D)
    return res


def assert_same(dev, host):
    for k in ('D',) + TC.OUT_F64:
        assert np.array_equal(bits(dev[k]), bits(host[k])), k
    for k in TC.OUT_I32:
        assert np.array_equal(dev[k], host[k]), k


# (mode, gates, stored nodes, S, max_sweeps, host copies of the offset tables)
MIXED = [(0, True, True, 8, None, True), (1, True, False, 8, None, False), (0, False, False, 1, None, True), (1, False, True, 2, None, True),
         (0, True, True, 8, 0, True), (1, True, True, 5, 1, False)]


@pytest.fixture(scope='module')
def mixed():
    """the mixed batch and, per mode, its gate costs: computed once and left unchanged"""
    sc = mixed_scene()
    entry, exit = poses_for(sc)
    return sc, {mode: TC.gate_costs(sc, entry, exit, R, mode) for mode in (0, 1)}, stored_nodes(sc, 41)


@pytest.mark.parametrize('mode,gates,with_sn,S,max_sweeps,host_tables', MIXED)
def test_mixed_batch_equals_host_bit_for_bit(mixed, mode, gates, with_sn, S, max_sweeps, host_tables):
    sc, ends, sn = mixed
    En, Xn = ends[mode] if gates else (None, None)
    sn = sn if with_sn else None
    host = TC.twin(sc, R, mode, E=En, X=Xn, stored_node=sn, S=S, max_sweeps=max_sweeps)
    U, I = L.EUNSUPPORTED, L.EINVAL
    assert host['status'].tolist() == [0, 0, 0, 0, U, 0, I, U, 0, 0, U, 0, 0]
    if max_sweeps is None and S > 1:
        assert host['sweeps'].max() >= 1 and (host['cost'][host['status'] == 0] <= host['stored'][host['status'] == 0]).all()
    assert_same(device_tour(sc, mode, En, Xn, sn, S=S, max_sweeps=max_sweeps, host_tables=host_tables), host)


@pytest.mark.parametrize('mode', [0, 1])
def test_cell_cap_equals_host_bit_for_bit(mode):
    sc = cap_cells_scene()
    host = TC.twin(sc, R, mode, S=3, max_sweeps=3)
    assert host['status'].tolist() == [0] and host['sweeps'][0] == 3
    assert_same(device_tour(sc, mode, S=3, max_sweeps=3), host)


def test_block_cap_equals_host_bit_for_bit():
    sc = cap_block_scene()
    assert int(sc.doff[-1]) == 1024 * 1024
    entry, exit = poses_for(sc)
    En, Xn = TC.gate_costs(sc, entry, exit, R, 0)
    host = TC.twin(sc, R, 0, E=En, X=Xn, S=1, max_sweeps=1)
    assert host['status'].tolist() == [0]
    assert_same(device_tour(sc, 0, En, Xn, S=1, max_sweeps=1), host)


@pytest.mark.parametrize('reversing', [False, True], ids=['dubins', 'rs'])
def test_cell_tour_in_chunks(monkeypatch, mixed, reversing):
    sc, ends, sn = mixed
    mode = int(reversing)
    entry, exit = poses_for(sc)
    host = TC.twin(sc, R, mode, E=ends[mode][0], X=ends[mode][1], stored_node=sn, S=4)
    sizes = CL._tour_block_sizes(sc.coff, sc.voff)
    assert np.array_equal(np.concatenate([[0], np.cumsum(sizes)]), sc.doff)
    monkeypatch.setattr(CL, 'TOUR_D_BUDGET', 8 * 5000)
    chunks = CL._tour_chunks(sizes, CL.TOUR_D_BUDGET)
    assert len(chunks) >= 3 and chunks[0][0] == 0 and chunks[-1][1] == sc.n and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    pin, pout = np.stack(sc.poses()[:3], axis=1), np.stack(sc.poses()[3:], axis=1)
    t = CL.cell_tour(sc.coff, sc.voff, pin, pout, sc.w, R, reversing=reversing, entry=entry, exit=exit, stored_node=sn, starts=4)
    dev = dict(order=t.order, node=t.node, cost=t.cost, stored=t.stored_cost, joint_length=t.joint_length, winner=t.winner, sweeps=t.sweeps,
               skipped=t.skipped, status=t.status, tours=t.tours, costs=t.costs)
    for k in TC.OUT_F64:
        assert np.array_equal(bits(_np(dev[k])), bits(host[k])), k
    for k in TC.OUT_I32:
        assert np.array_equal(_np(dev[k]), host[k]), k
    assert _np(t.field(5)).tolist() == host['order'][sc.coff[5]:sc.coff[6]].tolist()
