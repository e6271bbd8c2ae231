"""The CSR toolkit of engine's binding layer on CPU tensors -- the owner of every element, the scalar-or-one-per broadcast, the join of
several tables, the grouping by owner -- and the two joins built on it, _cover_paths and _mission_table, each against a plain numpy
restatement written here.  No device is touched: the helpers take the device their tensors live on."""
import numpy as np
import pytest
import torch

from field_coverage_path_planning_amd import engine as E

CPU = torch.device('cpu')
t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64))
f64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
i8 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int8))


# ---- the owner of every element ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('off', [[0, 2, 2, 5], [0, 0, 0], [0, 3], [0], [0, 0, 4, 4, 5, 5]])
def test_owners(off):
    want = np.concatenate([np.full(b - a, r) for r, (a, b) in enumerate(zip(off[:-1], off[1:]))] + [np.zeros(0)]).astype(np.int64)
    got = E._owners(t64(off), off[-1])
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    got32 = E._owners(t64(off), off[-1], torch.int32)
    assert got32.dtype == torch.int32 and np.array_equal(got32.numpy(), want)


# ---- a scalar, or one value per row ------------------------------------------------------------------------------------------------------
def test_one_per():
    assert E._one_per(f64([2.5]), 3, 'angle', 'value per field').tolist() == [2.5, 2.5, 2.5]
    assert E._one_per(f64(2.5), 3, 'angle', 'value per field').tolist() == [2.5, 2.5, 2.5]           # (a 0-d tensor)
    full = f64([1.0, 2.0, 3.0])
    assert E._one_per(full, 3, 'angle', 'value per field').tolist() == [1.0, 2.0, 3.0]
    assert E._one_per(f64([[1.0], [2.0]]), 2, 'angle', 'value per field').shape == (2,)
    assert E._one_per(f64([7.0]), 1, 'angle', 'value per field').tolist() == [7.0]                 # n == 1: nothing to expand
    assert E._one_per(t64([4]), 0, 'pair_field', 'field index per pair').numel() == 0             # one for all of none
    assert all(E._one_per(t, n, 'a', 'b').is_contiguous() for t, n in ((f64([2.5]), 3), (full, 3), (full[::2], 2)))
    with pytest.raises(ValueError, match='^angle must be a scalar or hold one value per field$'):
        E._one_per(f64([1.0, 2.0]), 3, 'angle', 'value per field')
    with pytest.raises(ValueError, match='^pair_field must be a scalar or hold one field index per pair$'):
        E._one_per(t64([0, 1]), 1, 'pair_field', 'field index per pair')
    with pytest.raises(ValueError, match='^pair_field must be a scalar or hold one field index per pair$'):
        E._pair_field([0, 1, 0], 2, CPU)
    assert E._pair_field(1, 3, CPU).tolist() == [1, 1, 1] and E._pair_field(np.array([2, 0]), 2, CPU).dtype == torch.int64


# ---- the join ----------------------------------------------------------------------------------------------------------------------------
def _np_join(tables):
    """tables: [(offsets list, [column arrays])] -> (first, starts, offsets, columns)"""
    first, starts, off = [0], [0], []
    for o, cols in tables:
        off += [v + starts[-1] for v in o[:-1]]
        first.append(first[-1] + len(o) - 1)
        starts.append(starts[-1] + len(cols[0]))
    ncol = len(tables[0][1]) if tables else 0
    return first, starts, off + [starts[-1]], [np.concatenate([c[j] for _, c in tables]) for j in range(ncol)]


def _check_join(tables, hosts, want_host):
    dtypes = (torch.float64, torch.int8)
    got = E._join_csr([t64(o) for o, _ in tables], hosts, [(f64(c[0]), i8(c[1])) for _, c in tables], dtypes, CPU)
    first, starts, off, cols = _np_join(tables)
    assert got[0].dtype == np.int64 and got[0].tolist() == first and got[1].dtype == np.int64 and got[1].tolist() == starts
    assert got[2].dtype == torch.int64 and got[2].tolist() == off and got[2].is_contiguous()
    if want_host:
        assert got[3].dtype == np.int64 and got[3].flags['C_CONTIGUOUS'] and got[3].tolist() == off
    else:
        assert got[3] is None
    assert [c.dtype for c in got[4]] == list(dtypes) and len(got[4]) == 2
    for g, w in zip(got[4], cols or [np.zeros(0), np.zeros(0)]):
        assert np.array_equal(g.numpy(), w) and g.is_contiguous()


A = ([0, 2, 5], [np.arange(5.0), np.arange(5) % 3])
EMPTY = ([0, 0], [np.zeros(0), np.zeros(0)])                    # one path, no sample
B = ([0, 1, 1, 4], [10.0 + np.arange(4), -np.ones(4)])


def test_join_csr():
    _check_join([], [], True)                                   # zero sets: the offsets [0], a host copy (every set of none brought one)
    _check_join([A], [np.array(A[0])], True)
    _check_join([A, EMPTY, B], [np.array(A[0]), np.array(EMPTY[0]), np.array(B[0], dtype=np.int32)], True)
    _check_join([A, EMPTY, B], [np.array(A[0]), None, np.array(B[0])], False)          # one set's offsets live on the device only
    _check_join([B, A], [None, None], False)


# ---- the grouping ------------------------------------------------------------------------------------------------------------------------
def _np_group(owner, n):
    order = sorted(range(len(owner)), key=lambda k: owner[k])                         # (sorted() is stable)
    counts = [sum(1 for o in owner if o == g) for g in range(n)]
    return order, [0] + list(np.cumsum(counts))


@pytest.mark.parametrize('owner,n', [([2, 0, 2, 0, 3, 0], 5), ([1, 0], 2), ([], 3), ([], 0), ([0, 0, 0], 1), ([3, 2, 1, 0, 3, 2, 1, 0], 4)])
def test_group_by(owner, n):
    order, goff = E._group_by(t64(owner), n, 'out of range')
    want_order, want_off = _np_group(owner, n)
    assert order.tolist() == want_order and goff.tolist() == [int(v) for v in want_off]
    assert goff.dtype == torch.int64 and goff.is_contiguous() and goff.numel() == n + 1


def test_group_by_range():
    for owner, n in (([0, 3], 3), ([-1, 0], 2), ([0], 0)):
        with pytest.raises(ValueError, match='^out of range$'):
            E._group_by(t64(owner), n, 'out of range')
    order, goff = E._group_by(t64([4, -1, 1]), 3)                # not asked to look: such rows belong to no group
    assert order.tolist() == [1, 2, 0] and goff.tolist() == [1, 1, 2, 2]


# ---- the two joins of the chain ----------------------------------------------------------------------------------------------------------
def _loops(host=True):
    """a HeadlandPaths of three rings on fields [1, 0, 1], passes [0, 0, 1], with 3, 0 and 4 samples; host=False: its offsets without their
    host copy, as a set whose offsets live on the device only"""
    off = [0, 3, 3, 7]
    part = i8([0, 1, 4, 0, 0, 1, 4])
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt)
    return E.HeadlandPaths(t64(off), np.array(off) if host else None, f64(np.arange(7.0)), f64(10.0 + np.arange(7)), f64(0.1 * np.arange(7)),
                           f64(0.01 * np.arange(7)), part, i8([1, 1, -1, 1, 1, 1, 1]), torch.arange(7, dtype=torch.int32), z(3), z(3), z(3), z(3, torch.int32), t64(np.arange(15)),
                           t64([[1, 0], [0, 0], [1, 1]]), 0.5)


def _tuple_set():
    """two open paths of 2 and 3 samples on fields [0, 1]"""
    return np.array([0, 2, 5]), 100.0 + np.arange(5), 200.0 + np.arange(5), np.arange(5) * 0.5, np.zeros(5), np.array([0, 0, 1, 0, 0]), np.ones(5)


def test_path_set_methods():
    hp = _loops()
    assert hp.closed is True and E.FieldPaths.closed is False and E.PathSet.closed is False
    assert hp.path_field().tolist() == [1, 0, 1] and hp.drive_order().tolist() == [0, 1, 2] and hp.drive_order(True).tolist() == [2, 0, 1]
    assert hp.work().tolist() == [True, False, True, True, True, False, True]
    assert hp.pass_id().dtype == torch.int32 and hp.pass_id().tolist() == [-1, -1, -1, -3, -3, -3, -3]
    assert [t.tolist() for t in hp.ring(2)] == [t.tolist() for t in (hp.x[3:], hp.y[3:], hp.heading[3:], hp.part[3:])]
    ps = E.PathSet(hp.offsets, hp.offsets_host, hp.x, hp.y, hp.heading, hp.kappa, hp.part, hp.gear)
    assert ps.path_field().tolist() == [0, 1, 2] and ps.pass_id().tolist() == [0, 0, 0, 2, 2, 2, 2] and ps.drive_order(True).tolist() == [0, 1, 2]
    fp = E.FieldPaths(*[getattr(hp, k) for k in ('offsets', 'offsets_host', 'x', 'y', 'heading', 'kappa', 'part', 'gear', 'leg')], None, None, None, None)
    assert fp.work().tolist() == [True, False, False, True, True, False, False] and fp.pass_id() is fp.leg and fp.path_field().tolist() == [0, 1, 2]


@pytest.mark.parametrize('host', [True, False])
def test_cover_paths(host):
    hp = _loops(host)
    off, x, y, _, _, _, _ = _tuple_set()
    work, pas = [1, 0, 1, 1, 0], None
    n_paths, total, poff, poff_h, gx, gy, gw, gp, fpo, ids = E._cover_paths((hp, (off, x, y, [0, 1], work, pas)), 2, CPU)
    assert (n_paths, total) == (5, 12) and poff.tolist() == [0, 3, 3, 7, 9, 12]
    assert (poff_h.tolist() == poff.tolist() and poff_h.dtype == np.int64) if host else poff_h is None
    assert np.array_equal(gx.numpy(), np.concatenate([np.arange(7.0), x])) and np.array_equal(gy.numpy(), np.concatenate([10.0 + np.arange(7), y]))
    assert gw.dtype == torch.uint8 and gw.tolist() == [1, 0, 1, 1, 1, 0, 1] + work
    assert gp.dtype == torch.int32 and gp.tolist() == [-1, -1, -1, -3, -3, -3, -3] + [3, 3, 4, 4, 4]       # the tuple's default: the path's index
    # owners [1, 0, 1, 0, 1]: field 0 has paths 1 and 3, field 1 has 0, 2 and 4, each in the order given
    assert ids.tolist() == [1, 3, 0, 2, 4] and fpo.tolist() == [0, 2, 5] and fpo.dtype == torch.int64
    one = E._cover_paths(hp, 3, CPU)                             # a single set, itself: field 2 has no path
    assert one[0] == 3 and one[9].tolist() == [1, 0, 2] and one[8].tolist() == [0, 1, 3, 3]
    alone = E._cover_paths((off, x, y, None, None, None), 1, CPU)          # a single set as a tuple: field 0, all work, pass = path
    assert alone[0] == 2 and alone[6].tolist() == [1] * 5 and alone[7].tolist() == [0, 0, 1, 1, 1] and alone[8].tolist() == [0, 2]
    none = E._cover_paths((), 2, CPU)
    assert none[:2] == (0, 0) and none[2].tolist() == [0] and none[8].tolist() == [0, 0, 0] and none[9].numel() == 0
    with pytest.raises(ValueError, match='path_field must name a field of the batch'):
        E._cover_paths(hp, 1, CPU)
    with pytest.raises(ValueError, match='a path set needs one field per path'):
        E._cover_paths((off, x, y, [0], None, None), 2, CPU)


@pytest.mark.parametrize('innermost_first', [False, True])
@pytest.mark.parametrize('host', [True, False])
def test_mission_table(host, innermost_first):
    hp = _loops(host)
    tup = _tuple_set()
    t = E._mission_table([hp, tup + ([0, 1], False)], CPU, innermost_first, n_fields=3)
    assert isinstance(t, E._MissionTable) and t.n == 3 and t.first.tolist() == [0, 3, 5] and t.starts.tolist() == [0, 7, 12]
    ps = t.paths
    assert isinstance(ps, E.PathSet) and ps.offsets.tolist() == [0, 3, 3, 7, 9, 12] and ps.offsets_host.tolist() == [0, 3, 3, 7, 9, 12]
    assert ps.offsets_host.dtype == np.int64
    for got, a, b in zip((ps.x, ps.y, ps.heading, ps.kappa, ps.part, ps.gear), (hp.x, hp.y, hp.heading, hp.kappa, hp.part, hp.gear), tup[1:]):
        assert np.array_equal(got.numpy(), np.concatenate([a.numpy(), np.asarray(b).astype(a.numpy().dtype)])) and got.is_contiguous()
    # items in driving order: the loops as stored (rings 0, 1, 2) or the innermost pass first (ring 2, then 0, 1), then the open paths;
    # grouped by field, stable: field 0 has ring 1 and path 3, field 1 rings 0 and 2 (or 2 and 0) and path 4, field 2 nothing
    ring_items = [2, 0] if innermost_first else [0, 2]
    assert t.ioff.tolist() == [0, 2, 5, 5] and t.ioff_h.tolist() == [0, 2, 5, 5]
    assert t.ipath.tolist() == [1, 3] + ring_items + [4] and t.ipath_h.tolist() == t.ipath.tolist()
    assert t.iset.tolist() == [0, 1, 0, 0, 1] and t.iset.dtype == torch.int32
    assert t.iclosed.tolist() == [1, 0, 1, 1, 0] and t.iclosed.dtype == torch.int32
    assert t.longest == 4                                        # the longest CLOSED path: ring 2's four samples, not the open path of three
    assert E._mission_table([hp], CPU).n == 2 and E._mission_table([hp], CPU, entry=np.zeros((4, 3))).n == 4
    assert E._mission_table([tup + (0, False)], CPU, n_fields=1).longest == 0
    empty = E._mission_table([], CPU, n_fields=2)
    assert empty.ioff.tolist() == [0, 0, 0] and empty.paths.offsets.tolist() == [0] and empty.longest == 0 and empty.ipath.numel() == 0
    with pytest.raises(ValueError, match='an item names a field outside'):
        E._mission_table([hp], CPU, n_fields=1)
    with pytest.raises(ValueError, match='an item set needs six columns'):
        E._mission_table([tup[:6] + (np.ones(4), [0, 1], False)], CPU)
