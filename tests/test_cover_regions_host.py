"""The coverage regions on the host (fcpp_debug_cover_regions: csrc/fcpp_regionfn.h, the member and neighbour functions the kernels run)
against a flood fill written here (tests/cover_region_cases.py: plain numpy / Python, a stack): offsets, records, the labels after counts
and the labels after fill, on every shape of the cases module under both connectivities; the named kinds on a hand-made byte grid; the
records' sums and boxes against numpy; the call's errors; and one end-to-end case through fcpp_debug_polygon_cover.  Every value is an
integer: every comparison is ==.  tests/test_gpu_cover_regions.py compares the device entries with this twin."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from tests import cover_region_cases as C
from tests.support import check_entries
from tests.test_polygon_cover_host import RECT40, host_cover, layout, swaths

ENTRIES = {'fcpp_cover_regions_counts': 12, 'fcpp_cover_regions_fill': 10, 'fcpp_debug_cover_regions': 12}
EINVAL, ESIZE = L.EINVAL, L.ESIZE
SHAPES = C.shapes()


def test_entries_are_declared_bound_and_exported():
    check_entries(ENTRIES)


@pytest.mark.parametrize('connectivity', (4, 8))
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_twin_equals_flood_fill(name, connectivity):
    grids, known = SHAPES[name]
    got = C.twin(grids, 3, 1, connectivity)
    want = C.flood_batch(grids, 3, 1, connectivity)
    per_field = np.diff(got['offsets']).tolist()
    print(name, connectivity, per_field)
    if known is not None:
        assert per_field == known[connectivity]
    for k in ('offsets', 'records', 'keys', 'index'):
        assert np.array_equal(got[k], want[k]), k
    # what the rule says of every result
    dims, off, flat = C.pack(grids)
    mem = (flat & 3) == 1
    assert np.array_equal(got['keys'] >= 0, mem) and np.array_equal(got['index'] >= 0, mem)
    assert (got['keys'][~mem] == -1).all() and (got['index'][~mem] == -1).all()
    for i in range(len(grids)):
        r = got['records'][got['offsets'][i]:got['offsets'][i + 1]]
        assert (np.diff(r['first']) > 0).all()                  # ascending key
        assert r['cells'].sum() == np.count_nonzero(mem[off[i]:off[i + 1]])
        keys = got['keys'][off[i]:off[i + 1]]
        assert np.array_equal(keys[r['first']], r['first'])   # the key is a member of its own region: its smallest


def test_full_grid_is_one_region_with_key_zero():
    got = C.twin(SHAPES['full'][0], 3, 1, 4)
    r = got['records']
    assert len(r) == 1 and (r['first'][0], r['cells'][0]) == (0, 16900)
    assert (r['a_min'][0], r['a_max'][0], r['b_min'][0], r['b_max'][0]) == (0, 129, 0, 129)
    assert r['sum_a'][0] == r['sum_b'][0] == 130 * (129 * 130 // 2)


def test_far_key_is_the_field_minimum():
    got = C.twin(SHAPES['far_key'][0], 3, 1, 4)
    assert got['records']['first'].tolist() == [3 * 200 + 150]


def test_comb_teeth_collapse_through_the_spine():
    got = C.twin(SHAPES['comb'][0], 3, 1, 4)
    g = SHAPES['comb'][0][0]
    assert (got['keys'].reshape(g.shape)[g == 1] == 0).all()


BYTES = np.array([[0, 1, 1, 3, 7, 2, 2, 0],
                  [1, 1, 3, 7, 7, 2, 0, 1],
                  [5, 1, 0, 3, 3, 6, 2, 1],
                  [2, 0, 1, 0, 7, 7, 3, 3]], dtype=np.uint8)


@pytest.mark.parametrize('connectivity', (4, 8))
@pytest.mark.parametrize('kind', sorted(C.KINDS))
def test_named_kinds(kind, connectivity):
    mask, value = C.KINDS[kind]
    got = C.twin([BYTES], mask, value, connectivity)
    assert C.same(got, C.flood_batch([BYTES], mask, value, connectivity))
    want = {'missed': (BYTES & 3) == 1, 'overlapped': (BYTES & 4) != 0, 'spill': (BYTES & 3) == 2, 'covered': (BYTES & 3) == 3}[kind]
    assert np.array_equal(got['index'].reshape(BYTES.shape) >= 0, want) and want.any()


@pytest.mark.parametrize('connectivity', (4, 8))
def test_records_against_numpy(connectivity):
    grids = SHAPES['random_bytes'][0] + C.mixed_batch(12, seed=3)
    got = C.twin(grids, 3, 1, connectivity)
    dims, off, flat = C.pack(grids)
    assert got['offsets'][-1] > 100
    for i, g in enumerate(grids):
        ny, nx = g.shape
        idx = got['index'][off[i]:off[i + 1]].reshape(ny, nx)
        r = got['records'][got['offsets'][i]:got['offsets'][i + 1]]
        assert idx.max(initial=-1) == len(r) - 1
        b, a = np.nonzero(idx >= 0)
        k = idx[b, a]
        assert np.array_equal(np.bincount(k, minlength=len(r)), r['cells'])
        assert np.array_equal(np.bincount(k, weights=a, minlength=len(r)).astype(np.int64), r['sum_a'])
        assert np.array_equal(np.bincount(k, weights=b, minlength=len(r)).astype(np.int64), r['sum_b'])
        for name, col, fn in (('a_min', a, np.minimum), ('a_max', a, np.maximum), ('b_min', b, np.minimum), ('b_max', b, np.maximum)):
            ext = np.full(len(r), 1 << 30 if fn is np.minimum else -1, np.int64)
            fn.at(ext, k, col)
            assert np.array_equal(ext, r[name]), name
        first = np.full(len(r), 1 << 40, np.int64)
        np.minimum.at(first, k, b * nx + a)
        assert np.array_equal(first, r['first'])


def test_mask_that_selects_everything_and_nothing():
    g = [BYTES]
    assert np.diff(C.twin(g, 0, 0, 4)['offsets']).tolist() == [1]                # every cell is a member
    assert C.twin(g, 255, 200, 8)['offsets'][-1] == 0


def test_call_errors():
    lib = L.load()
    g = [BYTES, BYTES[:2]]
    dims, off, flat = C.pack(g)
    for mask, value, conn in ((3, 4, 4), (256, 1, 4), (3, -1, 4), (-1, 0, 4), (3, 1, 6), (3, 1, 0), (1, 3, 8)):
        C.twin(g, mask, value, conn, expect=EINVAL)
    ro = np.zeros(3, np.int64)
    call = lambda d, o, f, cap=0: lib.fcpp_debug_cover_regions(len(d), C._p(d), C._p(o), C._p(f), 3, 1, 4, C._p(ro), cap, None, None, None)
    assert call(dims, off, flat) == 0
    assert lib.fcpp_debug_cover_regions(2, None, C._p(off), C._p(flat), 3, 1, 4, C._p(ro), 0, None, None, None) == EINVAL
    assert lib.fcpp_debug_cover_regions(2, C._p(dims), None, C._p(flat), 3, 1, 4, C._p(ro), 0, None, None, None) == EINVAL
    assert lib.fcpp_debug_cover_regions(2, C._p(dims), C._p(off), None, 3, 1, 4, C._p(ro), 0, None, None, None) == EINVAL
    assert lib.fcpp_debug_cover_regions(-1, C._p(dims), C._p(off), C._p(flat), 3, 1, 4, C._p(ro), 0, None, None, None) == ESIZE
    assert call(dims, off, flat, cap=-1) == ESIZE
    bad = off.copy(); bad[0] = 1
    assert call(dims, bad, flat) == ESIZE                       # does not start at 0
    bad = off.copy(); bad[1] = off[2]; bad[2] = off[1]
    assert call(dims, bad, flat) == ESIZE                       # decreases
    bad = off.copy(); bad[2] += 1
    assert call(dims, bad, flat) == ESIZE                       # disagrees with nx ny
    bad = dims.copy(); bad[0, 2], bad[0, 3] = bad[0, 3], -bad[0, 2]
    assert call(bad, off, flat) == ESIZE                        # a negative size
    bad = dims.copy(); bad[0, 2], bad[0, 3] = 1 << 20, 1 << 20
    assert call(bad, off, flat) == ESIZE                        # more than 2^28 cells
    assert b'' != lib.fcpp_last_error()
    # no field at all is a valid call
    assert lib.fcpp_debug_cover_regions(0, C._p(dims), C._p(off[:1].copy()), None, 3, 1, 4, C._p(ro), 0, None, None, None) == 0 and ro[0] == 0


def test_missed_strips_of_a_rectangle_under_three_passes():
    """40 x 20 m under three passes of width 4 m at y = 2, 10, 18: the strips 4 < y < 8 and 12 < y < 16 are missed, and nothing else"""
    res = 0.25
    out = host_cover([RECT40], 4.0, res, layout(1, swaths((2, 10, 18))))
    cnt = out['counts'][0]
    assert cnt[0] == 12800 and cnt[0] - cnt[1] == 2 * 160 * 16 and cnt[3] == 0          # the scene gives two strips of 40 m x 4 m
    dims, off, flat = out['dims'], out['cell_offsets'], out['grid']
    for connectivity in (4, 8):
        got = C.twin(None, *C.KINDS['missed'], connectivity, packed=(dims, off, flat))
        r = got['records']
        assert len(r) == 2 and r['cells'].sum() == cnt[0] - cnt[1] and r['cells'].tolist() == [2560, 2560]
        # in metres, through the grid's origin: gx = gy = -2
        y_lo = out['gy'][0] + r['b_min'] * res
        y_hi = out['gy'][0] + (r['b_max'] + 1) * res
        assert y_lo.tolist() == [4.0, 12.0] and y_hi.tolist() == [8.0, 16.0]
        cx = out['gx'][0] + (r['sum_a'] / r['cells'] + 0.5) * res
        cy = out['gy'][0] + (r['sum_b'] / r['cells'] + 0.5) * res
        assert cx.tolist() == [20.0, 20.0] and cy.tolist() == [6.0, 14.0]
        assert C.same(got, C.flood_batch(out['grids'], 3, 1, connectivity))
    assert C.twin(None, *C.KINDS['covered'], 4, packed=(dims, off, flat))['offsets'].tolist() == [0, 3]


def test_second_round_cases_reach_the_rounds_they_are_named_for():
    """what tests/test_gpu_cover_regions.py drives the kernels' strided loops with, asserted from the inputs; the twin
    agrees with the flood fill on the smaller ones, and on every case the records add up to the members"""
    g = SHAPES['checkerboard'][0][0]
    assert C.tiles_of([g]) == 9 and g.shape[1] % C.T == 2 and g.shape[0] % C.T == 2          # 3 x 3 tiles, the last ones 2 cells wide
    assert g.size > C.BLOCK_CELLS and g.size % C.BLOCK_CELLS                                    # more than one numbering block, no multiple
    assert np.count_nonzero(g.reshape(-1)[:C.BLOCK_CELLS] == 1) > 256                           # more roots in a block than threads
    for grid in C.roots_only():
        per_block = [np.count_nonzero(grid.reshape(-1)[k:k + C.BLOCK_CELLS] == 1) for k in range(0, grid.size, C.BLOCK_CELLS)]
        assert min(per_block[:-1]) >= 1000 > 256 and grid.size > C.BLOCK_CELLS
    assert np.diff(C.twin(C.roots_only(), 3, 1, 4)['offsets']).tolist() == [10000, 20000]
    batch = C.seam_batch(C.MI355X_CUS)
    assert C.tiles_of(batch) > C.seam_round_tiles(C.MI355X_CUS) == 2048 and len(batch) > 256 and C.blocks_of(batch) > 256
    got = C.twin(batch, 3, 1, 4)
    assert all(np.diff(got['offsets'])[i] == 1 for i in range(len(batch)) if i % 3)
    assert C.same(C.twin(batch[:6], 3, 1, 8), C.flood_batch(batch[:6], 3, 1, 8))
    big = C.many_blocks_field()
    assert C.blocks_of([big]) == 269 > 256 and big.size % C.BLOCK_CELLS == 2272 and C.tiles_of([big]) == 18 * 16
    for connectivity in (4, 8):
        r = C.twin([big], 3, 1, connectivity)['records']
        assert r['cells'].sum() == np.count_nonzero(big == 1) and r['cells'].max() > 10 * C.BLOCK_CELLS
