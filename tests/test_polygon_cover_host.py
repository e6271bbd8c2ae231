"""The polygon coverage report on the host (fcpp_debug_polygon_cover: csrc/fcpp_pcoverfn.h, the expressions the kernels run): known cell
counts of the 40 x 20 rectangle (checked with numpy against the rule; no cell centre lies on a boundary), the covered predicate against
the CPU oracle's cover_grid (an independent implementation of fcpp_cover_grid's predicate, which caps = 1 reproduces), the inside bit
against the oracle's point_in_polygon per ring, the work mask, joints and flat ends, pass ids, failed fields, odd paths and the layout of
the path table.  tests/test_gpu_polygon_cover.py compares the device entries with this twin bit for bit."""
import numpy as np
import pytest

import oracle as orc
from field_coverage_path_planning_amd import _lib as L
from tests.support import check_entries, p as _p
from tests.test_swaths_host import ELL, HOLE, pack, star

ENTRIES = {'fcpp_polygon_cover_sizes': 14, 'fcpp_polygon_cover': 26, 'fcpp_debug_polygon_cover': 25}
RECT40 = [(0, 0), (40, 0), (40, 20), (0, 20)]
EINVAL, EUNSUPPORTED = -1, -3


def line(x0, y0, x1, y1, m):
    return np.column_stack([np.linspace(x0, x1, m), np.linspace(y0, y1, m)])


def swaths(ys, x0=0.0, x1=40.0, m=3):
    return [line(x0, y, x1, y, m) for y in ys]


def layout(n, paths, owner=None, work=None, pas=None, order=None, force_ids=False):
    """The path table of a call.  paths: list of (m, 2) arrays; owner: the field of every path (default 0); work / pas: None, or a list
    with an array (or None: all work / the constant 0) per path; order: the paths' order in storage (default: as listed).  -> dict of the
    arrays the entries take: path_offsets, x, y, work, pass, field_path_offsets, path_ids (None when the grouped order is the identity)."""
    paths = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in paths]
    owner = [0] * len(paths) if owner is None else list(owner)
    store = list(range(len(paths))) if order is None else list(order)
    lens = [len(paths[p]) for p in store]
    poff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    xy = np.concatenate([paths[p] for p in store]) if store else np.zeros((0, 2))
    w = None if work is None else np.concatenate([np.ones(len(paths[p]), np.uint8) if work[p] is None else np.asarray(work[p], np.uint8)
                                                  for p in store] + [np.zeros(0, np.uint8)])
    ps = None if pas is None else np.concatenate([np.zeros(len(paths[p]), np.int32) if pas[p] is None
                                                  else np.broadcast_to(np.asarray(pas[p], np.int32), (len(paths[p]),)) for p in store]
                                                 + [np.zeros(0, np.int32)])
    own_s = np.asarray([owner[p] for p in store], dtype=np.int64)
    ids = np.argsort(own_s, kind='stable').astype(np.int64)
    fpo = np.concatenate([[0], np.cumsum(np.bincount(own_s, minlength=n)[:n])]).astype(np.int64) if n else np.zeros(1, np.int64)
    if not force_ids and np.array_equal(ids, np.arange(len(ids))):
        ids = None
    return dict(n_paths=len(store), path_offsets=poff, x=np.ascontiguousarray(xy[:, 0]), y=np.ascontiguousarray(xy[:, 1]), work=w,
                **{'pass': ps}, field_path_offsets=fpo, path_ids=ids)


def host_cover(fields, W, res, lay, caps=0, want_grid=True, expect=0):
    """fcpp_debug_polygon_cover -> dict: dims (n, 4 int64: gx, gy as float64 bits), gx, gy, nx, ny, cell_offsets, counts (n, 4), status, grid
    (flat) and grids (list of (ny, nx) views)"""
    lib = L.load()
    ro, vo, x, y = pack(fields)
    n = len(ro) - 1
    out = dict(dims=np.full((n, 4), -7, np.int64), cell_offsets=np.full(n + 1, -7, np.int64), counts=np.full((n, 4), -7, np.int64),
               status=np.full(n, -7, np.int32))
    head = (n, _p(ro), len(vo) - 1, _p(vo), len(x), _p(x), _p(y), float(W), float(res), int(caps), lay['n_paths'], _p(lay['path_offsets']),
            len(lay['x']), _p(lay['x']), _p(lay['y']), _p(lay['work']), _p(lay['pass']), _p(lay['field_path_offsets']), _p(lay['path_ids']))
    if expect:          # (a call error: found with the paths in hand)
        assert lib.fcpp_debug_polygon_cover(*head, None, None, 0, None, _p(out['counts']), None) == expect
        return None
    rc = lib.fcpp_debug_polygon_cover(*head, _p(out['dims']), _p(out['cell_offsets']), 0, None, None, _p(out['status']))
    assert rc == 0, lib.fcpp_last_error()
    total = int(out['cell_offsets'][-1])
    grid = np.full(total, 0xEE, np.uint8) if want_grid else None
    off2, st2 = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
    rc = lib.fcpp_debug_polygon_cover(*head, None, _p(off2), total, _p(grid), _p(out['counts']), _p(st2))
    assert rc == 0, lib.fcpp_last_error()
    assert np.array_equal(off2, out['cell_offsets']) and np.array_equal(st2, out['status'])
    out['gx'], out['gy'] = out['dims'][:, 0].copy().view(np.float64), out['dims'][:, 1].copy().view(np.float64)
    out['nx'], out['ny'] = out['dims'][:, 2], out['dims'][:, 3]
    out['grid'] = grid
    if want_grid:
        out['grids'] = [grid[out['cell_offsets'][i]:out['cell_offsets'][i + 1]].reshape(int(out['ny'][i]), int(out['nx'][i])) for i in range(n)]
        for i, g in enumerate(out['grids']):        # the counts are the grid's
            cnt = [np.count_nonzero(g & 1), np.count_nonzero((g & 3) == 3), np.count_nonzero((g & 5) == 5), np.count_nonzero((g & 3) == 2)]
            assert cnt == out['counts'][i].tolist() and not (g & 0xF8).any()
            assert not ((g & 4) != 0)[(g & 2) == 0].any()              # overlapped implies covered
    return out


def test_entries_are_declared_bound_and_exported():
    check_entries(ENTRIES)


# ---- the rectangle's known answers ----------------------------------------------------------------------------------------------------------
FIVE = (2, 6, 10, 14, 18)
KNOWN = [
    ('full_flat', swaths(FIVE), None, 0, (12800, 0, 0)),
    ('full_round', swaths(FIVE), None, 1, (12800, 0, 1040)),
    ('short_flat', swaths(FIVE, 2.0, 38.0), None, 0, (11520, 0, 0)),
    ('short_round', swaths(FIVE, 2.0, 38.0), None, 1, (12560, 0, 0)),
    ('two_overlapping', swaths((2, 5)), None, 0, (4480, 640, 0)),
]


@pytest.mark.parametrize('name,paths,pas,caps,want', KNOWN, ids=[k[0] for k in KNOWN])
def test_rectangle_known_counts(name, paths, pas, caps, want):
    out = host_cover([RECT40], 4.0, 0.25, layout(1, paths, pas=pas), caps=caps)
    assert out['status'][0] == 0 and (out['nx'][0], out['ny'][0]) == (176, 96)
    assert (out['gx'][0], out['gy'][0]) == (-2.0, -2.0)
    assert out['counts'][0].tolist() == [12800, *want]


def test_same_pass_id_is_no_overlap_and_ids_only_compare():
    two = swaths((2, 5))
    one = host_cover([RECT40], 4.0, 0.25, layout(1, two, pas=[1, 1]))
    assert one['counts'][0].tolist() == [12800, 4480, 0, 0]
    other = host_cover([RECT40], 4.0, 0.25, layout(1, two, pas=[4711, 4711]))
    assert np.array_equal(one['grid'], other['grid']) and np.array_equal(one['counts'], other['counts'])
    # two different ids, whatever their values and whichever comes first
    a = host_cover([RECT40], 4.0, 0.25, layout(1, two, pas=[1, 4711]))
    b = host_cover([RECT40], 4.0, 0.25, layout(1, two, pas=[-5, 3], order=[1, 0]))
    assert a['counts'][0].tolist() == [12800, 4480, 640, 0] and np.array_equal(a['grid'], b['grid'])


# ---- against the oracle ----------------------------------------------------------------------------------------------------------------------
def _zigzag(seed, m, lo, hi):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(lo[0], hi[0], m), rng.uniform(lo[1], hi[1], m)])


ORACLE_FIELDS = [RECT40, [ELL, HOLE], star(7, 7)]


def test_round_caps_equal_the_oracles_cover_grid():
    """caps = 1, all samples working, one path per field: covered + spill and grid bit 1 are cover_grid's A count and A bit"""
    paths = [np.concatenate([swaths(FIVE)[0], swaths(FIVE)[1][::-1], [[5.0, 12.0], [5.0, 12.0], [50.0, 30.0]]]),
             _zigzag(3, 40, (-5, -5), (65, 55)), _zigzag(4, 30, (150, -260), (440, 10))]
    for W, res in ((4.0, 0.25), (3.2, 0.7)):
        out = host_cover(ORACLE_FIELDS, W, res, layout(3, paths, owner=[0, 1, 2]), caps=1)
        for i in range(3):
            cnt, g = orc.cover_grid(out['gx'][i], out['gy'][i], res, 0.5, W / 2, int(out['nx'][i]), int(out['ny'][i]), paths[i], strict=True)
            assert out['status'][i] == 0 and cnt[1] == out['counts'][i][1] + out['counts'][i][3] and cnt[1] > 0
            assert np.array_equal(g & 1, (out['grids'][i] >> 1) & 1)


def _inside_by_oracle(field, out, i, res):
    rings = field if isinstance(field, list) and np.ndim(field[0]) == 2 else [field]
    nx, ny = int(out['nx'][i]), int(out['ny'][i])
    want = np.zeros((ny, nx), np.uint8)
    for b in range(ny):
        Y = out['gy'][i] + (b + 0.5) * res
        for a in range(nx):
            X = out['gx'][i] + (a + 0.5) * res
            for r in rings:
                want[b, a] ^= orc.point_in_polygon(X, Y, r)
    return want


STAR300 = star(300, 300)


def test_inside_bit_equals_point_in_polygon_per_ring():
    """shapes without ties: integer vertices against half-integer cell centres, a random star (more than 256 edges)"""
    fields = [[ELL, HOLE], ELL, STAR300]
    for W, res in ((2.0, 1.0), (6.0, 3.0)):
        out = host_cover(fields, W, res, layout(3, []))
        assert out['status'].tolist() == [0, 0, 0] and not out['counts'][:, 1:].any()
        for i, f in enumerate(fields):
            assert np.array_equal(out['grids'][i] & 1, _inside_by_oracle(f, out, i, res)), i
    out = host_cover(fields, 2.0, 1.0, layout(3, []))
    assert out['counts'][0][0] == 60 * 20 + 25 * 30 - 100 and out['counts'][1][0] == 60 * 20 + 25 * 30


# ---- work mask, joints, flat ends -----------------------------------------------------------------------------------------------------------
SQ30 = [(0, 0), (30, 0), (30, 30), (0, 30)]


def test_a_connector_covers_nothing():
    a, b = line(2, 2, 38, 2, 5), line(38, 10, 2, 10, 5)
    turn = np.column_stack([38 + 4 * np.sin(np.linspace(0, np.pi, 9)), 6 - 4 * np.cos(np.linspace(0, np.pi, 9))])
    path = np.concatenate([a, turn, b])
    work = np.concatenate([np.ones(5), np.zeros(9), np.ones(5)]).astype(np.uint8)
    one = host_cover([RECT40], 4.0, 0.25, layout(1, [path], work=[work], pas=[0]))
    two = host_cover([RECT40], 4.0, 0.25, layout(1, [a, b], pas=[0, 0]))
    assert np.array_equal(one['grid'], two['grid']) and one['counts'][0].tolist() == [12800, 2 * 36 * 4 * 16, 0, 0]
    # without the mask the connector is swept too (it leaves the field: spill)
    allw = host_cover([RECT40], 4.0, 0.25, layout(1, [path], pas=[0]))
    assert allw['counts'][0][1] > one['counts'][0][1] and allw['counts'][0][3] > 0


def _arc():
    t = np.linspace(0.0, np.pi / 2, 40)
    return np.column_stack([10 + 6 * np.cos(t), 10 + 6 * np.sin(t)])


def test_arc_joints_close_the_wedges_and_ends_stay_flat():
    flat = host_cover([SQ30], 4.0, 0.25, layout(1, [_arc()]), caps=0)
    rnd = host_cover([SQ30], 4.0, 0.25, layout(1, [_arc()]), caps=1)
    assert rnd['counts'][0][1] > flat['counts'][0][1] > 0
    g = (flat['grids'][0] >> 1) & 1
    assert not (g & ~((rnd['grids'][0] >> 1) & 1)).any()             # round ends only add
    # the swept area: the quarter annulus of radii 4 and 8, and less than that with two half discs (the discs of the first and last
    # interior joints reach behind the flat ends by r minus the sample spacing: the rule's, and round ends reach r)
    assert np.pi * 12 - 1.0 < flat['counts'][0][1] * 0.0625 < rnd['counts'][0][1] * 0.0625 < np.pi * 12 + np.pi * 4 + 1.0
    X = flat['gx'][0] + (np.arange(int(flat['nx'][0])) + 0.5) * 0.25
    Y = flat['gy'][0] + (np.arange(int(flat['ny'][0])) + 0.5) * 0.25
    # chords longer than r: nothing behind the flat end lines (dot < 0 at the start, dot > len2 at the end), and round ends do reach there
    t = np.linspace(0.0, np.pi / 2, 5)
    coarse = np.column_stack([10 + 6 * np.cos(t), 10 + 6 * np.sin(t)])
    c0 = (host_cover([SQ30], 4.0, 0.25, layout(1, [coarse]), caps=0)['grids'][0] >> 1) & 1
    c1 = (host_cover([SQ30], 4.0, 0.25, layout(1, [coarse]), caps=1)['grids'][0] >> 1) & 1
    assert c0.any() and not (c0 & ~c1).any()
    for a, b in ((coarse[0], coarse[1]), (coarse[-1], coarse[-2])):
        behind = (X[None, :] - a[0]) * (b[0] - a[0]) + (Y[:, None] - a[1]) * (b[1] - a[1]) < -1e-9
        assert not c0[behind].any() and c1[behind].any()
    # the outer side (farther than 6 from the centre): along every row the covered cells are contiguous
    outer = np.hypot(X[None, :] - 10.0, Y[:, None] - 10.0) >= 6.0
    rows = 0
    for b in range(g.shape[0]):
        cells = g[b][outer[b] & (X > 10.0)]
        on = np.flatnonzero(cells)
        if on.size:
            rows += 1
            assert cells[on[0]:on[-1] + 1].all(), b
    assert rows > 30


def test_a_nan_sample_cuts_the_run():
    run = line(4, 6, 36, 6, 5)
    cut = run.copy()
    cut[2] = (np.nan, 6.0)
    a = host_cover([RECT40], 4.0, 0.25, layout(1, [cut], pas=[0]))
    b = host_cover([RECT40], 4.0, 0.25, layout(1, [run[:2], run[3:]], pas=[0, 0]))
    assert np.array_equal(a['grid'], b['grid']) and a['counts'][0].tolist() == [12800, 2 * 8 * 4 * 16, 0, 0]
    inf = run.copy()
    inf[2] = (20.0, np.inf)
    assert np.array_equal(host_cover([RECT40], 4.0, 0.25, layout(1, [inf], pas=[0]))['grid'], a['grid'])


# ---- failures and odd inputs ----------------------------------------------------------------------------------------------------------------
def test_failed_fields_leave_their_neighbours_alone():
    bad = [(0, 0), (10, 0), (10, np.nan), (0, 10)]
    paths = [swaths(FIVE)[0], line(1, 1, 9, 9, 4), swaths(FIVE)[1]]
    out = host_cover([RECT40, bad, [RECT40[:2]], [], RECT40], 4.0, 0.25, layout(5, paths, owner=[0, 1, 4]))
    assert out['status'].tolist() == [0, EINVAL, EINVAL, EINVAL, 0]
    solo = [host_cover([RECT40], 4.0, 0.25, layout(1, [p])) for p in (paths[0], paths[2])]
    assert out['nx'].tolist() == [176, 0, 0, 0, 176] and not out['counts'][1:4].any() and not out['dims'][1:4].any()
    assert np.array_equal(out['grids'][0], solo[0]['grids'][0]) and np.array_equal(out['grids'][4], solo[1]['grids'][0])
    # more than 2^28 cells
    big = host_cover([RECT40, [(0, 0), (4000, 0), (4000, 2000), (0, 2000)], RECT40], 4.0, 0.25 / 2, layout(3, paths, owner=[0, 1, 2]))
    assert big['status'].tolist() == [0, EUNSUPPORTED, 0] and big['nx'].tolist() == [352, 0, 352] and not big['counts'][1].any()
    assert host_cover([RECT40], 4.0, 1e-3, layout(1, paths[:1]))['status'].tolist() == [EUNSUPPORTED]


def test_call_errors():
    lay = layout(1, swaths(FIVE))
    for W, res, caps in ((0.0, 0.25, 0), (np.inf, 0.25, 0), (4.0, 0.0, 0), (4.0, np.nan, 0), (4.0, 0.25, 2)):
        lib = L.load()
        ro, vo, x, y = pack([RECT40])
        cnt = np.zeros(4, np.int64)
        rc = lib.fcpp_debug_polygon_cover(1, _p(ro), 1, _p(vo), 4, _p(x), _p(y), float(W), float(res), caps, lay['n_paths'], _p(lay['path_offsets']),
                                          len(lay['x']), _p(lay['x']), _p(lay['y']), None, None, _p(lay['field_path_offsets']), None, None, None, 0,
                                          None, _p(cnt), None)
        assert rc == EINVAL
    bad_ids = dict(lay, path_ids=np.asarray([0, 1, 2, 3, 5], np.int64))
    host_cover([RECT40], 4.0, 0.25, bad_ids, expect=EINVAL)
    host_cover([RECT40], 4.0, 0.25, dict(lay, field_path_offsets=np.asarray([0, 6], np.int64)), expect=-6)
    host_cover([RECT40], 4.0, 0.25, dict(lay, field_path_offsets=np.asarray([1, 5], np.int64)), expect=-6)


def test_odd_paths_and_empty_batches():
    base = host_cover([RECT40, SQ30], 4.0, 0.25, layout(2, swaths(FIVE), owner=[0] * 5))
    assert base['counts'][1].tolist() == [14400, 0, 0, 0]                      # a field without paths
    odd = swaths(FIVE) + [np.zeros((0, 2)), np.asarray([[20.0, 10.0]])]
    out = host_cover([RECT40, SQ30], 4.0, 0.25, layout(2, odd, owner=[0] * 7, order=[5, 0, 1, 6, 2, 3, 4]))
    assert np.array_equal(out['grid'], base['grid']) and np.array_equal(out['counts'], base['counts'])
    one = host_cover([RECT40], 4.0, 0.25, layout(1, [np.asarray([[20.0, 10.0]])]), caps=1)
    assert one['counts'][0].tolist() == [12800, 0, 0, 0]
    none = host_cover([], 4.0, 0.25, layout(0, []))
    assert none['cell_offsets'].tolist() == [0] and none['grid'].size == 0


def test_the_path_table_may_be_permuted():
    fields = [RECT40, SQ30, [ELL, HOLE]]
    paths = swaths(FIVE) + [_arc(), line(1, 1, 29, 29, 7)] + [_zigzag(5, 12, (0, 0), (60, 50))]
    owner = [0] * 5 + [1, 1] + [2]
    pas = [0, 1, 2, 3, 4, 0, 1, 0]
    grouped = host_cover(fields, 4.0, 0.5, layout(3, paths, owner, pas=pas))
    forced = host_cover(fields, 4.0, 0.5, layout(3, paths, owner, pas=pas, force_ids=True))
    mixed = layout(3, paths, owner, pas=pas, order=[7, 2, 5, 0, 6, 4, 1, 3])
    assert mixed['path_ids'] is not None and not np.array_equal(mixed['path_ids'], np.arange(8))
    perm = host_cover(fields, 4.0, 0.5, mixed)
    for other in (forced, perm):
        assert np.array_equal(other['grid'], grouped['grid']) and np.array_equal(other['counts'], grouped['counts'])
    assert grouped['counts'][:, 1].all()


# ---- second rounds: many chunks, the early exit, many rings ----------------------------------------------------------------------------------
# The device's tile kernel tests a field's chunk boxes 256 at a time, one ballot word per wavefront of 64, and stops a tile once all its cells
# are overlapped; the sizes kernel reads a field's rings 64 at a time.  None of that is in the twin, so the twin's checkers cannot see it:
# tests/test_gpu_polygon_cover.py runs the cases below on the device, and the tests here assert -- from the inputs, the 256-segment chunk
# rule and numpy -- that every case reaches the round it is named for.
CHUNK, TILE, WORDS = 256, 64, (64, 128, 192, 256)
W4, RES4 = 4.0, 0.25
SIDE = [(100, 100), (130, 100), (130, 130), (100, 130)]          # a second field before RECT40, so that its chunks do not start at 0


def short_paths(seed, count, lo=(-1.0, -1.0), hi=(41.0, 21.0), step=1.5):
    """`count` paths of 2 or 3 samples, steps of at most `step` m along each axis, starting anywhere in lo .. hi: one chunk each"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        m = int(rng.integers(2, 4))
        out.append(rng.uniform(lo, hi) + np.cumsum(rng.uniform(-step, step, (m, 2)), axis=0))
    return out


def field_chunks(lay, f):
    """the chunks of field f in the order the glue lists them (fcpp_glue_cover.cpp: pcover_chunks, restated): (path, first sample, segments)"""
    fpo, poff, ids = lay['field_path_offsets'], lay['path_offsets'], lay['path_ids']
    out = []
    for s in range(fpo[f], fpo[f + 1]):
        p = s if ids is None else int(ids[s])
        out += [(p, k, min(CHUNK, poff[p + 1] - 1 - k)) for k in range(poff[p], poff[p + 1] - 1, CHUNK)]
    return out


def tile_hits(lay, f, dims_row, width, res):
    """(tiles, chunks) bool: the box of the chunk's samples grown by width / 2 meets the rectangle of the tile's cell centres (every
    segment of these cases works, so a chunk's box is its samples' box)"""
    gx, gy = dims_row[:2].copy().view(np.float64)
    nx, ny = int(dims_row[2]), int(dims_row[3])
    boxes = np.array([[lay['x'][k:k + c + 1].min(), lay['y'][k:k + c + 1].min(), lay['x'][k:k + c + 1].max(), lay['y'][k:k + c + 1].max()]
                      for _, k, c in field_chunks(lay, f)]).reshape(-1, 4)
    tiles = []
    for ty in range(-(-ny // TILE)):
        for tx in range(-(-nx // TILE)):
            i1, j1 = min(tx * TILE + TILE - 1, nx - 1), min(ty * TILE + TILE - 1, ny - 1)
            tiles.append([gx + (tx * TILE + 0.5) * res, gy + (ty * TILE + 0.5) * res, gx + (i1 + 0.5) * res, gy + (j1 + 0.5) * res])
    t, r = np.array(tiles)[:, None, :], width / 2
    b = boxes[None, :, :]
    return ~((b[..., 0] - t[..., 2] > r) | (t[..., 0] - b[..., 2] > r) | (b[..., 1] - t[..., 3] > r) | (t[..., 1] - b[..., 3] > r))


def many_chunks_case(count, permuted):
    """[SIDE, RECT40]: RECT40 under `count` short paths with five pass ids; SIDE's three paths stand between them in storage.  Steps of
    at most 0.1 m: with flat ends a path sweeps a strip 4 m long and a cell or two wide, so even 513 of them leave most cells open and
    every further one changes the grid"""
    paths = short_paths(count, count, step=0.1) + swaths((104, 112, 120), 100.0, 130.0)
    owner = [1] * count + [0] * 3
    pas = [k % 5 for k in range(count)] + [0, 1, 2]
    order = np.random.default_rng(count + 1).permutation(len(paths)).tolist() if permuted else [0, count, 1, count + 1, count + 2] + list(range(2, count))
    return [SIDE, RECT40], layout(2, paths, owner, pas=pas, order=order)


MANY_CHUNKS = [(c, p) for c in (65, 256, 257, 513) for p in (False, True)]


@pytest.mark.parametrize('count,permuted', MANY_CHUNKS)
def test_many_chunks_cases_reach_the_ballot_words_they_are_named_for(count, permuted):
    fields, lay = many_chunks_case(count, permuted)
    chunks = field_chunks(lay, 1)
    assert len(chunks) == count and len(field_chunks(lay, 0)) == 3 and lay['path_ids'] is not None          # RECT40's chunks start at 3
    assert all(c in (1, 2) for _, _, c in chunks) and len(set(lay['pass'].tolist())) == 5
    out = host_cover(fields, W4, RES4, lay)
    assert (out['nx'][1], out['ny'][1]) == (176, 96)          # 3 x 2 tiles
    hits = tile_hits(lay, 1, out['dims'][1], W4, RES4)
    assert hits.shape == (6, count)
    for word in WORDS:          # chunks whose index within the field is at least 64 / 128 / 192 (later ballot words) / 256 (round two)
        assert hits[:, word:].any() == (count > word), word
        if count >= word + 64:
            assert hits[:, word:].any(axis=1).all()          # ... in every tile, where a whole word of chunks lies there
    # and every ballot word's chunks change the answer: the twin's grid of the field's first 64 k chunks differs from that of its first
    # 64 (k + 1) (the rule does not depend on the order, so a device that loads the wrong chunk for a later word cannot give this grid)
    grids = [host_cover(fields, W4, RES4, dict(lay, field_path_offsets=np.array([0, 3, 3 + min(k, count)], np.int64)))['grid']
             for k in range(0, count + 64, 64)]
    assert np.array_equal(grids[-1], out['grid']) and all(not np.array_equal(a, b) for a, b in zip(grids[:-1], grids[1:]))
    assert out['counts'][1, 1] > 0 and out['counts'][1, 2] > 0 and out['counts'][1, 3] > 0


# the early exit: COVER_ROWS each driven twice with different pass ids and reaching past the grid overlap EVERY cell of the grid, margin
# cells included (a tile stops only when all its valid cells are overlapped, and every tile of this grid has margin cells); FIVE alone
# overlaps every in-field cell and leaves the margin rows open, so no tile may stop
COVER_ROWS = (-2,) + FIVE + (22,)
EARLY = [(rows, rev) for rows in ('five', 'cover') for rev in (False, True)]


def early_exit_case(rows, reverse):
    ys = FIVE if rows == 'five' else COVER_ROWS
    first = swaths(ys, -5.0, 45.0) + swaths(ys, -5.0, 45.0)
    pas = list(range(len(ys))) + list(range(100, 100 + len(ys)))
    more = short_paths(503, 250, (2.0, 2.0), (38.0, 18.0)) + short_paths(504, 127, (-1.5, -1.5), (41.5, -0.5)) \
        + short_paths(505, 126, (-1.5, 20.5), (41.5, 21.5))          # inside the field, in the lower and in the upper margin rows
    paths = first + more
    pas += list(range(200, 200 + len(more)))
    order = list(range(len(paths)))[::-1] if reverse else None
    return [RECT40], layout(1, paths, pas=pas, order=order), len(first)


@pytest.mark.parametrize('rows,reverse', EARLY)
def test_early_exit_cases_overlap_what_they_are_named_for(rows, reverse):
    fields, lay, n_first = early_exit_case(rows, reverse)
    chunks = field_chunks(lay, 0)
    assert len(chunks) == n_first + 503 > 2 * CHUNK and n_first == {'five': 10, 'cover': 14}[rows]
    # the twin on the covering rows alone
    ys = FIVE if rows == 'five' else COVER_ROWS
    alone = host_cover(fields, W4, RES4, layout(1, swaths(ys, -5.0, 45.0) * 2, pas=list(range(len(ys))) + list(range(100, 100 + len(ys)))))
    g = alone['grids'][0]
    assert ((g[(g & 1) == 1] & 5) == 5).all() and alone['counts'][0].tolist()[:3] == [12800, 12800, 12800]
    tiles = [g[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] for ty in range(2) for tx in range(3)]
    done = [bool(((t & 4) != 0).all()) for t in tiles]
    assert done == [rows == 'cover'] * 6
    # the covering rows stand in the first round of 256 chunks (listed order) or behind all 503 others (reversed: rounds two and three)
    where = [k for k, (p, _, _) in enumerate(chunks) if lay['path_offsets'][p + 1] - lay['path_offsets'][p] == 3 and lay['x'][lay['path_offsets'][p]] == -5.0]
    assert len(where) == n_first and (min(where) == 503 > CHUNK if reverse else max(where) < CHUNK)
    # the later paths lie in every tile, inside the field and in the margin rows, and bring new pass ids: nothing they add may show
    # where the rows already overlap, and all of it must show where they do not
    hits = tile_hits(lay, 0, alone['dims'][0], W4, RES4)
    late = [k for k in range(len(chunks)) if k not in where]
    assert hits[:, late].any(axis=1).all()
    full = host_cover(fields, W4, RES4, lay)
    changed = np.count_nonzero(full['grids'][0] != g)
    assert (changed == 0) == (rows == 'cover') and (rows == 'cover' or changed > 300)


# many rings: the field of 259 rings (tests/test_inset_host.py), its two copies with the LAST ring spoilt, and fields of exactly 64 and 65
# rings with their spoilt copies (the sizes kernel reads 64 rings a round)
def many_ring_fields():
    from tests.test_inset_host import HOLED, holed_square, spoilt_last_ring
    r64, r65 = holed_square(63, cols=8), holed_square(64, cols=8)
    return [HOLED, spoilt_last_ring(HOLED, 'short'), r64, spoilt_last_ring(r65, 'nan'), r65, spoilt_last_ring(HOLED, 'nan'),
            spoilt_last_ring(r65, 'short'), spoilt_last_ring(r64, 'nan')]


MANY_RING_PATHS = [line(-3, -3, 173, 163, 60), line(-3, -3, 83, 83, 30), line(-3, 83, 83, -3, 30)]
W_RINGS, RES_RINGS = 4.0, 0.5


def many_rings_case():
    return many_ring_fields(), layout(8, MANY_RING_PATHS, owner=[0, 2, 4])


def test_many_ring_fields_inside_bit_equals_point_in_polygon_per_ring():
    """the oracle's point_in_polygon per ring, asked for the cells of the ring's bounding box grown by a cell (a point outside a ring's
    bounding box is outside the ring); no cell centre lies on an edge: centres are odd multiples of 0.25, the outline is integer, the
    holes' vertices end in .1 .. .9 and their edges slant"""
    fields, lay = many_rings_case()
    assert [len(f) for f in fields] == [259, 259, 64, 65, 65, 259, 65, 64]
    out = host_cover(fields, W_RINGS, RES_RINGS, lay)
    assert out['status'].tolist() == [0, EINVAL, 0, EINVAL, 0, EINVAL, EINVAL, EINVAL]
    assert (out['nx'][0], out['ny'][0]) == (348, 328) and not out['dims'][[1, 3, 5, 6, 7]].any() and not out['counts'][[1, 3, 5, 6, 7]].any()
    for i in (0, 2, 4):
        nx, ny, gx, gy = int(out['nx'][i]), int(out['ny'][i]), out['gx'][i], out['gy'][i]
        want = np.zeros((ny, nx), np.uint8)
        for r in fields[i]:
            a0, b0 = (int(v) for v in np.floor((r.min(axis=0) - (gx, gy)) / RES_RINGS) - 1)
            a1, b1 = (int(v) for v in np.ceil((r.max(axis=0) - (gx, gy)) / RES_RINGS) + 1)
            for b in range(max(b0, 0), min(b1, ny)):
                for a in range(max(a0, 0), min(a1, nx)):
                    want[b, a] ^= orc.point_in_polygon(gx + (a + 0.5) * RES_RINGS, gy + (b + 0.5) * RES_RINGS, r)
        assert np.array_equal(out['grids'][i] & 1, want), i
        holes = sum(np.count_nonzero(want[int((r[:, 1].min() - gy) / RES_RINGS):int((r[:, 1].max() - gy) / RES_RINGS) + 1,
                                          int((r[:, 0].min() - gx) / RES_RINGS):int((r[:, 0].max() - gx) / RES_RINGS) + 1] == 0) > 0 for r in fields[i][1:])
        assert holes == len(fields[i]) - 1          # every hole, the last one included, takes cells out
        assert out['counts'][i][1] > 0 and out['counts'][i][3] > 0
