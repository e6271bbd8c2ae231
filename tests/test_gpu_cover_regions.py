"""The coverage regions on the device (fcpp_cover_regions_counts / fcpp_cover_regions_fill: csrc/fcpp_regions.hip) against their host twin
(fcpp_debug_cover_regions, tests/test_cover_regions_host.py) -- offsets, records, the labels after counts and the labels after fill, all
integers, all == -- on every shape of tests/cover_region_cases.py under both connectivities, on a batch of 65 fields of mixed sizes with
and without the host copies of the offsets, and on the second rounds DESIGN.md section 4 names: 3 x 3 tiles whose last tiles are 2 cells
wide (every 130 x 130 shape), more seam lanes than one launch of the seam kernel, fields of more cells than one numbering block and of no
multiple of it, more roots in a block than it has threads (the checkerboard), more blocks than one round of the scan.  Then
engine.coverage_regions and plan_polygon_fields(missed_min_area=...) on a small planned holed square."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import cover_region_cases as C
from tests.support import Gpu as BaseGpu

pytestmark = pytest.mark.gpu

SHAPES = C.shapes()
HOLED = [[(0, 0), (30, 0), (30, 30), (0, 30)], [(12, 12), (18, 12), (18, 18), (12, 18)]]
W, RES = 4.0, 0.25


def _ptr(t):
    return None if t is None else t.data_ptr()


def _hp(a):
    return None if a is None else a.ctypes.data


class Gpu(BaseGpu):
    def __init__(self):
        super().__init__()
        self.n_cu = self.torch.cuda.get_device_properties(self.dev).multi_processor_count


@pytest.fixture(scope='module')
def gpu():
    g = Gpu()
    g.ctx.bind_stream()
    return g


def dev_regions(g, packed, mask, value, connectivity, host_offsets=True):
    """the two device entries on exactly sized tensors -> the dict C.twin gives (numpy)"""
    torch = g.torch
    dims, off, flat = packed
    n, total = len(dims), len(flat)
    d_dims, d_off, d_grid = g.up(dims), g.up(off), g.up(flat)
    labels = torch.full((total,), -7, dtype=torch.int32, device=g.dev)
    roff = torch.full((n + 1,), -7, dtype=torch.int64, device=g.dev)
    roff_h = np.full(n + 1, -7, np.int64)
    g.ctx.bind_stream()
    rc = g.lib.fcpp_cover_regions_counts(g.h, n, _ptr(d_dims), _ptr(d_off), _hp(off) if host_offsets else None, _ptr(d_grid), mask, value, connectivity,
                                         _ptr(labels), _ptr(roff), _hp(roff_h) if host_offsets else None)
    assert rc == 0, g.lib.fcpp_last_error()
    roff_np = roff.cpu().numpy()
    if host_offsets:
        assert np.array_equal(roff_h, roff_np)
    keys = labels.cpu().numpy()
    k = int(roff_np[-1])
    rec = torch.full((k, 6), -7, dtype=torch.int64, device=g.dev)
    rc = g.lib.fcpp_cover_regions_fill(g.h, n, _ptr(d_dims), _ptr(d_off), _hp(off) if host_offsets else None, _ptr(labels), _ptr(roff),
                                       _hp(roff_h) if host_offsets else None, k, _ptr(rec))
    assert rc == 0, g.lib.fcpp_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d_grid.cpu().numpy(), flat) and np.array_equal(roff.cpu().numpy(), roff_np)        # inputs stay
    return dict(offsets=roff_np, records=rec.cpu().numpy().reshape(-1).view(C.REC), keys=keys, index=labels.cpu().numpy())


def same(dev, host):
    assert np.array_equal(dev['offsets'], host['offsets']), (dev['offsets'][:8], host['offsets'][:8])
    for k in ('keys', 'index'):
        bad = np.flatnonzero(dev[k] != host[k])
        assert bad.size == 0, (k, bad.size, bad[:8], dev[k][bad[:8]], host[k][bad[:8]])
    bad = np.flatnonzero(dev['records'] != host['records'])
    assert bad.size == 0, (bad.size, bad[:4], dev['records'][bad[:4]], host['records'][bad[:4]])


@pytest.mark.parametrize('connectivity', (4, 8))
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_every_host_shape_equals_the_twin(gpu, name, connectivity):
    grids = SHAPES[name][0]
    same(dev_regions(gpu, C.pack(grids), 3, 1, connectivity), C.twin(grids, 3, 1, connectivity))


@pytest.mark.parametrize('kind', sorted(C.KINDS))
def test_named_kinds_on_garbage_bytes(gpu, kind):
    grids = SHAPES['random_bytes'][0]
    mask, value = C.KINDS[kind]
    for connectivity in (4, 8):
        same(dev_regions(gpu, C.pack(grids), mask, value, connectivity), C.twin(grids, mask, value, connectivity))


@pytest.fixture(scope='module')
def batch65():
    grids = C.mixed_batch(65)
    assert sum(g.size == 0 for g in grids) >= 5 and grids[0].shape == (1, 1) and grids[1].shape == (150, 200)
    return grids, {c: C.twin(grids, 3, 1, c) for c in (4, 8)}


@pytest.mark.parametrize('host_offsets', (True, False))
@pytest.mark.parametrize('connectivity', (4, 8))
def test_batch_of_65_mixed_fields(gpu, batch65, connectivity, host_offsets):
    grids, host = batch65
    same(dev_regions(gpu, C.pack(grids), 3, 1, connectivity, host_offsets=host_offsets), host[connectivity])


def test_no_field_and_only_empty_fields(gpu):
    for grids in ([], [np.zeros((0, 0), np.uint8)] * 3):
        got = dev_regions(gpu, C.pack(grids), 3, 1, 4)
        assert got['offsets'].tolist() == [0] * (len(grids) + 1) and len(got['records']) == 0


# ---- second rounds --------------------------------------------------------------------------------------------------------------------
def test_more_seam_lanes_than_one_launch(gpu):
    """the seam kernel is launched with at most 4 workgroups per compute unit, 256 lanes each, 128 lanes per tile: 8 tiles per compute unit
    in a round.  Full 65 x 65 fields (four tiles each, one region iff all four seams are joined) until the tiles need a second round --
    which also is more fields and more numbering blocks than one round of 256 of the scan."""
    grids = C.seam_batch(gpu.n_cu)
    n = len(grids)
    assert C.tiles_of(grids) > C.seam_round_tiles(gpu.n_cu) and n > 256 and C.blocks_of(grids) > 256
    for connectivity in (4, 8):
        got = dev_regions(gpu, C.pack(grids), 3, 1, connectivity)
        same(got, C.twin(grids, 3, 1, connectivity))
        assert all(np.diff(got['offsets'])[i] == 1 for i in range(n) if i % 3)


def test_one_field_of_many_numbering_blocks(gpu):
    """1100 x 1000 random cells near the percolation threshold: 269 numbering blocks of 4096 in ONE field (the scan's second round, a last
    block of 2272 cells), 18 x 16 tiles (the last ones 12 and 40 cells wide), regions that wind through many tiles"""
    g = C.many_blocks_field()
    assert C.blocks_of([g]) == 269 and g.size % C.BLOCK_CELLS == 2272
    for connectivity in (4, 8):
        got = dev_regions(gpu, C.pack([g]), 3, 1, connectivity)
        same(got, C.twin([g], 3, 1, connectivity))
        assert got['records']['cells'].max() > 10 * C.BLOCK_CELLS          # a region of many blocks and tiles


def test_blocks_of_roots_only(gpu):
    """a field of isolated cells in every other column of every other row, and the checkerboard: at least 1000 and 2048 roots in a block of 256 threads"""
    grids = C.roots_only()
    got = dev_regions(gpu, C.pack(grids), 3, 1, 4)
    same(got, C.twin(grids, 3, 1, 4))
    assert np.diff(got['offsets']).tolist() == [10000, 20000]


def test_call_errors_come_before_any_kernel(gpu):
    torch = gpu.torch
    dims, off, flat = C.pack([SHAPES['full'][0][0], SHAPES['no_wrap_65'][0][0]])
    n, total = 2, len(flat)
    d_dims, d_off, d_grid = gpu.up(dims), gpu.up(off), gpu.up(flat)
    labels = torch.full((total,), -7, dtype=torch.int32, device=gpu.dev)
    roff = torch.full((n + 1,), -7, dtype=torch.int64, device=gpu.dev)
    counts = lambda *a: gpu.lib.fcpp_cover_regions_counts(*a)
    good = [gpu.h, n, _ptr(d_dims), _ptr(d_off), None, _ptr(d_grid), 3, 1, 4, _ptr(labels), _ptr(roff), None]

    def with_(k, v):
        a = list(good)
        a[k] = v
        return a
    for k in (0, 2, 3, 5, 9, 10):
        assert counts(*with_(k, None)) == L.EINVAL, k
    for k, v in ((6, 256), (6, -1), (7, 4), (7, 300), (8, 6), (8, 0)):
        assert counts(*with_(k, v)) == L.EINVAL, (k, v)
    assert counts(*with_(1, -1)) == L.ESIZE
    for bad in (off + 1, off[[0, 2, 1]], off + np.array([0, 0, 1])):
        bad_h = np.ascontiguousarray(bad, dtype=np.int64)
        bad_d = gpu.up(bad_h)
        assert counts(*with_(3, _ptr(bad_d))) == L.ESIZE
        assert counts(*with_(4, _hp(bad_h))) == L.ESIZE
    wrong = dims.copy()
    wrong[1, 2] += 1
    d_wrong = gpu.up(wrong)
    assert counts(*with_(2, _ptr(d_wrong))) == L.ESIZE
    torch.cuda.synchronize()
    assert (labels == -7).all() and (roff == -7).all()          # nothing ran
    assert counts(*good) == 0
    k = int(roff[-1])
    rec = torch.full((k, 6), -7, dtype=torch.int64, device=gpu.dev)
    keys = labels.clone()
    fill = lambda *a: gpu.lib.fcpp_cover_regions_fill(*a)
    fgood = [gpu.h, n, _ptr(d_dims), _ptr(d_off), None, _ptr(labels), _ptr(roff), None, k, _ptr(rec)]

    def fwith(j, v):
        a = list(fgood)
        a[j] = v
        return a
    for j in (0, 2, 3, 5, 6, 9):
        assert fill(*fwith(j, None)) == L.EINVAL, j
    for j, v in ((1, -1), (8, -1), (8, k + 1), (8, k - 1)):
        assert fill(*fwith(j, v)) == L.ESIZE, (j, v)
    r = roff.cpu().numpy()
    for bad in (r + 1, r[[0, 2, 1]] + np.array([0, 5, 0])):
        bad_h = np.ascontiguousarray(bad, dtype=np.int64)
        bad_d = gpu.up(bad_h)
        assert fill(*fwith(6, _ptr(bad_d))) == L.ESIZE
        assert fill(*fwith(7, _hp(bad_h))) == L.ESIZE
    assert fill(*fwith(2, _ptr(d_wrong))) == L.ESIZE
    torch.cuda.synchronize()
    assert (rec == -7).all() and torch.equal(labels, keys)      # nothing ran
    assert fill(*fgood) == 0


# ---- through the engine ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planned(gpu):
    kw = dict(width=W, radius=2.0, spacing=0.5, angles=[0.0, 0.5], passes=1)
    plan = E.plan_polygon_fields([HOLED], headland_paths=True, coverage_resolution=RES, **kw)
    cov = E.polygon_coverage([HOLED], W, RES, paths=(plan.paths, plan.headland_paths), want_grid=True)
    return kw, plan, cov


def _packed(cov):
    return cov.dims.cpu().numpy(), np.asarray(cov.cell_offsets_host, np.int64), cov.cells.cpu().numpy()


@pytest.mark.parametrize('connectivity', (4, 8))
@pytest.mark.parametrize('kind', ('missed', 'covered', 'spill', (4, 4)))
def test_engine_coverage_regions_equal_the_twin(gpu, planned, kind, connectivity):
    kw, plan, cov = planned
    mask, value = C.KINDS[kind] if isinstance(kind, str) else kind
    host = C.twin(None, mask, value, connectivity, packed=_packed(cov))
    reg = cov.regions(kind=kind, connectivity=connectivity, want_labels=True)
    r = host['records']
    assert np.array_equal(reg.offsets.cpu().numpy(), host['offsets']) and np.array_equal(reg.offsets_host, host['offsets'])
    assert np.array_equal(reg.first.cpu().numpy(), r['first']) and np.array_equal(reg.cells.cpu().numpy(), r['cells'])
    assert np.array_equal(reg.bbox.cpu().numpy(), np.column_stack([r['a_min'], r['a_max'], r['b_min'], r['b_max']]))
    assert np.array_equal(reg.sums.cpu().numpy(), np.column_stack([r['sum_a'], r['sum_b']]))
    assert np.array_equal(reg.labels.cpu().numpy(), host['index']) and reg.dropped.sum() == 0
    nx, ny = (int(v) for v in cov.dims[0, 2:].tolist())
    assert reg.label_grid(0).shape == (ny, nx) and reg.field(0) == slice(0, len(r))
    if kind == 'missed':
        cnt = cov.counts.cpu().numpy()[0]
        assert r['cells'].sum() == cnt[0] - cnt[1] and len(r) >= 1
    # the same float64 expressions on the host
    org = cov.origin().cpu().numpy()[0]
    assert np.array_equal(reg.area.cpu().numpy(), r['cells'].astype(np.float64) * (RES * RES))
    cen = np.column_stack([org[0] + (r['sum_a'] / r['cells'] + 0.5) * RES, org[1] + (r['sum_b'] / r['cells'] + 0.5) * RES])
    assert np.array_equal(reg.centroid.cpu().numpy(), cen)
    bnd = np.column_stack([org[0] + r['a_min'] * RES, org[1] + r['b_min'] * RES, org[0] + (r['a_max'] + 1.0) * RES, org[1] + (r['b_max'] + 1.0) * RES])
    assert np.array_equal(reg.bounds.cpu().numpy(), bnd)


def test_min_area_drops_records_and_remaps_labels(gpu, planned):
    kw, plan, cov = planned
    full = E.coverage_regions(cov, 'missed', want_labels=True)
    cells = full.cells.cpu().numpy()
    assert len(cells) >= 2 and cells.min() < cells.max()          # something to drop and something to keep
    cut = float(np.sort(cells)[len(cells) // 2]) * RES * RES       # the median region's area: it and the larger ones stay
    reg = E.coverage_regions(cov, 'missed', min_area=cut, want_labels=True)
    keep = cells * (RES * RES) >= cut
    assert 0 < keep.sum() < len(cells)
    assert reg.offsets_host.tolist() == [0, int(keep.sum())] and reg.offsets.cpu().numpy().tolist() == [0, int(keep.sum())]
    assert reg.dropped.cpu().numpy().tolist() == [[int((~keep).sum()), int(cells[~keep].sum())]]
    assert reg.dropped[0, 0] + len(reg.cells) == len(cells) and reg.dropped[0, 1] + reg.cells.sum() == cells.sum()
    for name in ('first', 'cells', 'bbox', 'sums', 'area', 'centroid', 'bounds'):
        assert np.array_equal(getattr(reg, name).cpu().numpy(), getattr(full, name).cpu().numpy()[keep]), name
    new = np.where(keep, np.cumsum(keep) - 1, -2)
    lab = full.labels.cpu().numpy()
    assert np.array_equal(reg.labels.cpu().numpy(), np.where(lab >= 0, new[np.maximum(lab, 0)], -1))
    with pytest.raises(ValueError):
        E.coverage_regions(plan.coverage)                           # made without want_grid
    with pytest.raises(ValueError):
        E.coverage_regions(cov, kind='mist')
    with pytest.raises(ValueError):
        E.coverage_regions(cov, connectivity=6)
    with pytest.raises(ValueError):
        reg2 = E.coverage_regions(cov)
        reg2.label_grid(0)


def test_plan_polygon_fields_with_and_without_missed_min_area(gpu, planned):
    kw, plan, cov = planned
    torch = gpu.torch
    with_ = E.plan_polygon_fields([HOLED], headland_paths=True, coverage_resolution=RES, missed_min_area=1.0, **kw)
    own = E.coverage_regions(with_.coverage, 'missed', min_area=1.0)
    assert with_.coverage.cells is not None and with_.missed is not None and plan.missed is None and plan.coverage.cells is None
    for name in ('offsets', 'first', 'cells', 'bbox', 'sums', 'area', 'centroid', 'bounds', 'dropped'):
        assert torch.equal(getattr(with_.missed, name), getattr(own, name)), name
    assert torch.equal(with_.coverage.cells, cov.cells)
    # every other member of the plan, bit for bit
    again = E.plan_polygon_fields([HOLED], headland_paths=True, coverage_resolution=RES, **kw)
    for other in (with_, again):
        for name in ('angle_index', 'angle'):
            assert torch.equal(getattr(other, name), getattr(plan, name)), name
        for part, names in (('paths', ('offsets', 'x', 'y', 'heading', 'kappa', 'part', 'gear', 'leg')), ('headland_paths', ('offsets', 'x', 'y')),
                            ('coverage', ('counts', 'status', 'dims', 'cell_offsets')), ('swaths', ('offsets',)), ('work', ('x', 'y'))):
            for name in names:
                a, b = getattr(getattr(other, part), name), getattr(getattr(plan, part), name)
                assert torch.equal(a.view(torch.uint8) if a.dtype.is_floating_point else a, b.view(torch.uint8) if b.dtype.is_floating_point else b), (part, name)
    assert again.missed is None and again.coverage.cells is None
    with pytest.raises(ValueError):
        E.plan_polygon_fields([HOLED], missed_min_area=1.0, **kw)
