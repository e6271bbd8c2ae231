"""Grids, an independent flood fill and the host twin's call for the coverage-region tests (tests/test_cover_regions_host.py checks the twin
against the flood fill; tests/test_gpu_cover_regions.py the device entries against the twin on the same grids).  A grid is a (ny, nx) uint8
array of coverage bytes (bit 0 inside, bit 1 covered, bit 2 overlapped); unless a case says otherwise 1 marks a member of kind 'missed' and 3
a non-member."""
import numpy as np

from field_coverage_path_planning_amd import _lib as L
from tests.support import p as _p

KINDS = {'missed': (3, 1), 'overlapped': (4, 4), 'spill': (3, 2), 'covered': (3, 3)}
REC = np.dtype([('first', np.int64), ('cells', np.int64), ('a_min', np.int32), ('a_max', np.int32), ('b_min', np.int32), ('b_max', np.int32),
                ('sum_a', np.int64), ('sum_b', np.int64)])
assert REC.itemsize == 48
T = 64                      # the kernels' tile edge
BLOCK_CELLS = 4096          # the kernels' numbering block


def members(shape, where):
    """a (ny, nx) grid: 1 where `where` (bool array), 3 elsewhere"""
    g = np.full(shape, 3, np.uint8)
    g[where] = 1
    return g


def pack(grids):
    """list of (ny, nx) uint8 grids -> dims (n, 4 int64: gx, gy as float64 bits, nx, ny), cell_offsets (n + 1), the bytes (flat)"""
    n = len(grids)
    dims = np.zeros((n, 4), np.int64)
    dims[:, 0] = np.arange(n, dtype=np.float64).view(np.int64)          # (any origin: the rule does not read it)
    dims[:, 1] = (-2.5 * np.arange(n, dtype=np.float64)).view(np.int64)
    for i, g in enumerate(grids):
        dims[i, 2], dims[i, 3] = g.shape[1], g.shape[0]
    off = np.concatenate([[0], np.cumsum([g.size for g in grids])]).astype(np.int64)
    flat = np.concatenate([np.ascontiguousarray(g, dtype=np.uint8).reshape(-1) for g in grids] + [np.zeros(0, np.uint8)])
    return dims, off, flat


def flood(g, mask, value, connectivity):
    """One grid by a stack flood fill in row-major order -> (records, keys, index): regions are met in ascending key"""
    ny, nx = g.shape
    mem = (g & mask) == value
    keys = np.full((ny, nx), -1, np.int32)
    index = np.full((ny, nx), -1, np.int32)
    step = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (1, -1), (-1, 1), (1, 1)] if connectivity == 8 else [])
    recs = []
    memb = mem.tolist()
    seen = [[False] * nx for _ in range(ny)]
    for b0 in range(ny):
        for a0 in range(nx):
            if not memb[b0][a0] or seen[b0][a0]:
                continue
            k, key = len(recs), b0 * nx + a0
            cells = []
            stack = [(a0, b0)]
            seen[b0][a0] = True
            while stack:
                a, b = stack.pop()
                cells.append((a, b))
                for da, db in step:
                    p, q = a + da, b + db
                    if 0 <= p < nx and 0 <= q < ny and memb[q][p] and not seen[q][p]:
                        seen[q][p] = True
                        stack.append((p, q))
            ca = np.array(cells, dtype=np.int64)
            keys[ca[:, 1], ca[:, 0]] = key
            index[ca[:, 1], ca[:, 0]] = k
            recs.append((key, len(cells), ca[:, 0].min(), ca[:, 0].max(), ca[:, 1].min(), ca[:, 1].max(), ca[:, 0].sum(), ca[:, 1].sum()))
    return np.array(recs, dtype=REC).reshape(-1), keys, index


def flood_batch(grids, mask, value, connectivity):
    """every grid -> dict like twin()'s"""
    parts = [flood(g, mask, value, connectivity) for g in grids]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([p[k].reshape(-1) for p in parts] + [np.zeros(0, dt)])
    return dict(offsets=off, records=cat(0, REC), keys=cat(1, np.int32), index=cat(2, np.int32))


def twin(grids, mask, value, connectivity, expect=0, packed=None):
    """fcpp_debug_cover_regions -> dict: offsets (n + 1), records (REC), keys / index (int32 per cell: the labels after counts / after fill)"""
    lib = L.load()
    dims, off, flat = pack(grids) if packed is None else packed
    n = len(dims)
    ro = np.full(n + 1, -7, np.int64)
    rc = lib.fcpp_debug_cover_regions(n, _p(dims), _p(off), _p(flat), mask, value, connectivity, _p(ro), 0, None, None, None)
    assert rc == expect, (rc, lib.fcpp_last_error())
    if expect:
        return None
    total = int(ro[-1])
    recs = np.zeros(total, REC)
    recs['first'] = -7
    keys, index = np.full(len(flat), -7, np.int32), np.full(len(flat), -7, np.int32)
    ro2 = np.full(n + 1, -7, np.int64)
    rc = lib.fcpp_debug_cover_regions(n, _p(dims), _p(off), _p(flat), mask, value, connectivity, _p(ro2), total, _p(recs), _p(keys), _p(index))
    assert rc == 0, lib.fcpp_last_error()
    assert np.array_equal(ro, ro2)
    return dict(offsets=ro, records=recs, keys=keys, index=index)


def same(a, b):
    """two results agree in every value"""
    return all(np.array_equal(a[k], b[k]) for k in ('offsets', 'records', 'keys', 'index'))


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------
def _spiral(n=130, centre=64, arms=14):
    """a one-cell-wide square spiral with one-cell gaps that winds out from the common corner of the four tiles around (centre, centre)"""
    w = np.zeros((n, n), bool)
    a = b = centre
    w[b, a] = True
    length, d = 2, 0
    for k in range(2 * arms):
        da, db = [(1, 0), (0, 1), (-1, 0), (0, -1)][d]
        for _ in range(length):
            a, b = a + da, b + db
            if 0 <= a < n and 0 <= b < n:
                w[b, a] = True
        d = (d + 1) % 4
        if k % 2 == 1:
            length += 2
    return w


def _serpentine(n=130):
    w = np.zeros((n, n), bool)
    w[0::2, :] = True
    w[1::4, n - 1] = True
    w[3::4, 0] = True
    return w


def _comb(n=130):
    """teeth in tile column 0 (every other row, columns 0 .. 63), the spine in tile column 1 (column 64)"""
    w = np.zeros((n, n), bool)
    w[0::2, :T] = True
    w[:, T] = True
    return w


def _far_key():
    """the bulk in tile row 1, column 0; a one-cell path leaves it to the right and climbs in tile column 2 up to row 3: the key lies there"""
    w = np.zeros((130, 200), bool)
    w[70:121, 5:51] = True
    w[70, 51:151] = True
    w[3:70, 150] = True
    return w


def _isolated(nx=60, ny=20):
    w = np.zeros((ny, nx), bool)
    w[0::2, 0::2] = True
    return w


def _gaps(m=200):
    w = np.ones(m, bool)
    w[[0, 5, 6, 63, 64, 65, 100, 128, 199]] = False
    return w


def shapes():
    """name -> (list of grids, {connectivity: regions per field} or None where the flood fill alone says)"""
    ii = np.arange(130)
    diag = np.zeros((130, 130), bool)
    diag[ii, ii] = True
    anti = np.zeros((130, 130), bool)
    anti[np.arange(128), 127 - np.arange(128)] = True          # through (64, 63) -> (63, 64)
    chk = (ii[:, None] + ii[None, :]) % 2 == 0
    no_wrap = np.zeros((10, 65), bool)
    no_wrap[:, 0] = no_wrap[:, 64] = True
    rng = np.random.default_rng(11)
    return {
        'one_member': ([members((1, 1), np.ones((1, 1), bool))], {4: [1], 8: [1]}),
        'one_other': ([members((1, 1), np.zeros((1, 1), bool))], {4: [0], 8: [0]}),
        'row_200': ([members((1, 200), _gaps()[None, :])], {4: [5], 8: [5]}),
        'column_200': ([members((200, 1), _gaps()[:, None])], {4: [5], 8: [5]}),
        'empty': ([members((130, 130), np.zeros((130, 130), bool))], {4: [0], 8: [0]}),
        'full': ([members((130, 130), np.ones((130, 130), bool))], {4: [1], 8: [1]}),
        'checkerboard': ([members((130, 130), chk)], {4: [8450], 8: [1]}),
        'diagonal': ([members((130, 130), diag)], {4: [130], 8: [1]}),
        'anti_diagonal': ([members((130, 130), anti)], {4: [128], 8: [1]}),
        'serpentine': ([members((130, 130), _serpentine())], {4: [1], 8: [1]}),
        'comb': ([members((130, 130), _comb())], {4: [1], 8: [1]}),
        'spiral': ([members((130, 130), _spiral())], {4: [1], 8: [1]}),
        'far_key': ([members((130, 200), _far_key())], {4: [1], 8: [1]}),
        'full_rows_two_fields': ([members((5, 10), np.ones((5, 10), bool)), members((4, 10), np.ones((4, 10), bool))], {4: [1, 1], 8: [1, 1]}),
        'no_wrap_65': ([members((10, 65), no_wrap)], {4: [2], 8: [2]}),
        'failed_in_the_middle': ([members((5, 5), np.ones((5, 5), bool)), np.zeros((0, 0), np.uint8), members((3, 7), chk[:3, :7])],
                                 {4: [1, 0, 11], 8: [1, 0, 1]}),
        'isolated_300': ([members((20, 60), _isolated())], {4: [300], 8: [300]}),
        'random_bytes': ([rng.integers(0, 256, (70, 131), dtype=np.uint8), rng.integers(0, 8, (129, 67), dtype=np.uint8)], None),
    }


def mixed_batch(n=65, seed=5):
    """n fields of mixed sizes, 1 x 1 up to 200 x 150, some empty, bytes 0 .. 7 with about half the cells missed"""
    rng = np.random.default_rng(seed)
    grids = []
    for i in range(n):
        if i % 9 == 4:
            grids.append(np.zeros((0, 0), np.uint8))
            continue
        nx, ny = (1, 1) if i == 0 else (200, 150) if i == 1 else (int(rng.integers(1, 201)), int(rng.integers(1, 151)))
        g = rng.integers(0, 8, (ny, nx), dtype=np.uint8)
        g[rng.random((ny, nx)) < 0.45] = 1
        grids.append(g)
    return grids


# ---- second rounds of the kernels' strided loops ------------------------------------------------------------------
SEAM_BLOCKS_PER_CU = 4      # the seam kernel's launch: at most this many workgroups of 256 lanes per compute unit, 128 lanes per tile
MI355X_CUS = 256


def tiles_of(grids):
    return sum(-(-g.shape[0] // T) * -(-g.shape[1] // T) for g in grids)


def blocks_of(grids):
    return sum(-(-g.size // BLOCK_CELLS) for g in grids)


def seam_round_tiles(n_cu):
    """the tiles whose seam lanes ONE round of the seam kernel's launch covers"""
    return SEAM_BLOCKS_PER_CU * n_cu * 256 // (2 * T)


def seam_batch(n_cu, seed=2):
    """2 n_cu + 40 fields of 65 x 65 (four tiles each, two in three of them full: one region iff all four seams are joined): more tiles
    than one round of the seam kernel on n_cu compute units, and more fields and numbering blocks than one round of 256 of the scan"""
    rng = np.random.default_rng(seed)
    full = np.ones((65, 65), bool)
    return [members((65, 65), full if i % 3 else rng.random((65, 65)) < 0.6) for i in range(2 * n_cu + 40)]


def many_blocks_field(seed=9):
    """1100 x 1000 random cells near the percolation threshold: 269 numbering blocks in ONE field, the last of 2272 cells; 18 x 16 tiles, the
    last ones 12 and 40 cells wide; regions that wind through many tiles"""
    rng = np.random.default_rng(seed)
    return members((1000, 1100), rng.random((1000, 1100)) < 0.59)


def roots_only():
    """isolated cells in every other column of every other row, and the checkerboard (connectivity 4): 1000 or more and 2048 roots per block"""
    ii = np.arange(200)
    return [members((200, 200), (ii[:, None] % 2 == 0) & (ii[None, :] % 2 == 0)), members((200, 200), (ii[:, None] + ii[None, :]) % 2 == 1)]
