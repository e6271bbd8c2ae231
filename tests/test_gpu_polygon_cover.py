"""The polygon coverage report on the device (fcpp_polygon_cover_sizes / fcpp_polygon_cover: csrc/fcpp_pcover.hip) against its host twin
(fcpp_debug_polygon_cover, tests/test_polygon_cover_host.py) bit for bit -- sizes, status, counts and every grid byte -- on batches of 1
and 65 fields chosen for the kernels' edges: a grid of exactly 64 and of 65 columns, partial tiles in both directions, a path of more
than 256 samples (chunk edges inside a run), a field of more than 256 edges, both caps, with and without work / pass / path_ids / the
grid / the host copies of the offsets; against fcpp_cover_grid (a device operator against a device operator); through
plan_polygon_fields; and on guarded buffers (tests/guarded.py).  Second rounds: one field under 65 / 256 / 257 / 513 chunks (the ballot words
and rounds of the chunk loop), tiles that may and may not stop early, fields of 64 / 65 / 259 rings."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.guarded import Arena
from tests.support import Gpu
from tests.test_polygon_cover_host import (EARLY, FIVE, MANY_CHUNKS, RECT40, RES_RINGS, SQ30, STAR300, W_RINGS, _arc, _zigzag, early_exit_case,
                                            field_chunks, host_cover, layout, line, many_chunks_case, many_rings_case, swaths)
from tests.test_swaths_host import ELL, HOLE, pack, star

pytestmark = pytest.mark.gpu

W, RES = 4.0, 0.25
NARROW64 = [(100, 0), (112, 0), (112, 9), (100, 9)]             # nx = 48 + 16 = 64
NARROW65 = [(100, 0), (112.25, 0), (112.25, 9), (100, 9)]       # nx = 49 + 16 = 65
LONG = line(0, 10, 40, 10, 401)                                  # a 40 m swath at spacing 0.1: two chunks, the edge inside the run


def _ptr(t):
    return None if t is None else t.data_ptr()


def _hp(a):
    return None if a is None else a.ctypes.data


@pytest.fixture(scope='module')
def gpu():
    g = Gpu()
    g.ctx.bind_stream()
    return g


def dev_cover(g, fields, lay, caps=0, want_grid=True, host_offsets=True, res=RES, width=W):
    """the two device entries on exactly sized tensors -> the dict host_cover gives (numpy)"""
    torch = g.torch
    ro, vo, x, y = pack(fields)
    n = len(ro) - 1
    t = [g.up(a) for a in (ro, vo, x, y)]
    head = (g.h, n, _ptr(t[0]), len(vo) - 1, _ptr(t[1]), len(x), _ptr(t[2]), _ptr(t[3]), float(width), float(res))
    dims = torch.full((n, 4), -7, dtype=torch.int64, device=g.dev)
    coff = torch.full((n + 1,), -7, dtype=torch.int64, device=g.dev)
    coff_h = np.full(n + 1, -7, np.int64)
    st1 = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    g.ctx.bind_stream()
    rc = g.lib.fcpp_polygon_cover_sizes(*head, _ptr(dims), _ptr(coff), _hp(coff_h) if host_offsets else None, _ptr(st1))
    assert rc == 0, g.lib.fcpp_last_error()
    coff_np = coff.cpu().numpy()
    if host_offsets:
        assert np.array_equal(coff_h, coff_np)
    total = int(coff_np[-1])
    p = {k: g.up(lay[k]) for k in ('path_offsets', 'x', 'y', 'work', 'pass', 'field_path_offsets', 'path_ids')}
    grid = torch.full((total,), 0xEE, dtype=torch.uint8, device=g.dev) if want_grid else None
    counts = torch.full((n, 4), -7, dtype=torch.int64, device=g.dev)
    st2 = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    rc = g.lib.fcpp_polygon_cover(*head, int(caps), lay['n_paths'], _ptr(p['path_offsets']), _hp(lay['path_offsets']) if host_offsets else None,
                                  len(lay['x']), _ptr(p['x']), _ptr(p['y']), _ptr(p['work']), _ptr(p['pass']), _ptr(p['field_path_offsets']),
                                  _ptr(p['path_ids']), _ptr(coff), _hp(coff_h) if host_offsets else None, _ptr(grid), _ptr(counts), _ptr(st2))
    assert rc == 0, g.lib.fcpp_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(st1.cpu().numpy(), st2.cpu().numpy())
    return dict(dims=dims.cpu().numpy(), cell_offsets=coff_np, status=st2.cpu().numpy(), counts=counts.cpu().numpy(),
                grid=None if grid is None else grid.cpu().numpy())


def same(dev, host, with_grid=True):
    for k in ('dims', 'cell_offsets', 'status', 'counts'):
        assert np.array_equal(dev[k], host[k]), k
    if with_grid:
        bad = np.flatnonzero(dev['grid'] != host['grid'])
        assert bad.size == 0, (bad.size, bad[:8], dev['grid'][bad[:8]], host['grid'][bad[:8]])


# ---- batches of one ---------------------------------------------------------------------------------------------------------------------------
def _connected():
    a, b = line(2, 2, 38, 2, 5), line(38, 10, 2, 10, 5)
    turn = np.column_stack([38 + 4 * np.sin(np.linspace(0, np.pi, 9)), 6 - 4 * np.cos(np.linspace(0, np.pi, 9))])
    return np.concatenate([a, turn, b]), np.concatenate([np.ones(5), np.zeros(9), np.ones(5)]).astype(np.uint8)


def _nan_run():
    run = line(101, 4, 111, 4, 9)
    run[4] = (np.nan, 4.0)
    return run


ONE = {
    'rect_swaths': ([RECT40], dict(paths=swaths(FIVE))),
    'rect_overlap': ([RECT40], dict(paths=swaths((2, 5)))),
    'rect_long_run': ([RECT40], dict(paths=[LONG, swaths(FIVE)[0]], pas=[7, 7])),
    'rect_connector': ([RECT40], dict(paths=[_connected()[0]], work=[_connected()[1]], pas=[None])),
    'nx64': ([NARROW64], dict(paths=[line(101, 2, 111, 2, 30), _nan_run()])),
    'nx65': ([NARROW65], dict(paths=[line(101, 2, 112, 2, 30), _nan_run()])),
    'ell_hole': ([[ELL, HOLE]], dict(paths=[_zigzag(3, 40, (-5, -5), (65, 55))])),
    'star300': ([STAR300], dict(paths=[_zigzag(4, 30, (150, -260), (440, 10))])),
    'arc': ([SQ30], dict(paths=[_arc()])),
    'no_paths': ([SQ30], dict(paths=[])),
    'invalid': ([[(0, 0), (10, 0), (10, np.nan), (0, 10)]], dict(paths=swaths(FIVE))),
}


@pytest.mark.parametrize('caps', [0, 1])
@pytest.mark.parametrize('name', list(ONE))
def test_one_field_equals_the_host_twin(gpu, name, caps):
    fields, kw = ONE[name]
    lay = layout(1, **kw)
    same(dev_cover(gpu, fields, lay, caps=caps), host_cover(fields, W, RES, lay, caps=caps))


# ---- a batch of 65 ------------------------------------------------------------------------------------------------------------------------------
def _batch65():
    rng = np.random.default_rng(65)
    fields = [RECT40, NARROW64, [ELL, HOLE], NARROW65, STAR300, SQ30, [(0, 0), (10, 0), (10, np.nan), (0, 10)],
              [(0, 0), (5000, 0), (5000, 4000), (0, 4000)], star(7, 7), ELL]
    paths = swaths(FIVE) + [LONG] + [line(101, 2, 111, 2, 30), _nan_run()] + [_zigzag(3, 40, (-5, -5), (65, 55))] + [line(101, 6, 112, 6, 12)]
    owner = [0] * 6 + [1, 1] + [2] + [3]
    paths += [_zigzag(4, 30, (150, -260), (440, 10)), _arc(), line(1, 1, 9, 9, 4), line(0, 0, 4000, 4000, 300), _zigzag(6, 300, (180, -240), (420, 0))]
    owner += [4, 5, 6, 7, 8]
    conn, cw = _connected()
    work = [None] * len(paths)
    while len(fields) < 65:
        w, h = rng.uniform(5.0, 45.0), rng.uniform(5.0, 45.0)
        ox, oy = rng.uniform(-500.0, 500.0, 2)
        fields.append([(ox, oy), (ox + w, oy), (ox + w, oy + h), (ox, oy + h)])
        for k in range(int(rng.integers(0, 4))):
            yk = oy + rng.uniform(0.0, h)
            paths.append(line(ox - 1.0, yk, ox + w + 1.0, yk + rng.uniform(-2, 2), int(rng.integers(2, 40))))
            owner.append(len(fields) - 1)
            work.append((rng.uniform(size=len(paths[-1])) < 0.8).astype(np.uint8))
    paths.append(conn)
    owner.append(0)
    work.append(cw)
    pas = [np.asarray(rng.integers(0, 3, len(p)), np.int32) for p in paths]
    return fields, paths, owner, work, pas


@pytest.fixture(scope='module')
def batch65():
    fields, paths, owner, work, pas = _batch65()
    assert len(fields) == 65
    order = np.random.default_rng(1).permutation(len(paths)).tolist()
    lays = {'full': layout(65, paths, owner, work=work, pas=pas, order=order),
            'bare': layout(65, [paths[k] for k in np.argsort(owner, kind='stable')], sorted(owner))}
    assert lays['full']['path_ids'] is not None and lays['bare']['path_ids'] is None and lays['bare']['work'] is None
    return fields, lays, {(k, caps): host_cover(fields, W, RES, lays[k], caps=caps) for k, caps in (('full', 0), ('bare', 1))}


def test_batch_of_65_with_masks_and_permuted_paths(gpu, batch65):
    fields, lays, host = batch65
    h = host[('full', 0)]
    assert h['status'][6] == -1 and h['status'][7] == -3 and np.count_nonzero(h['status']) == 2
    assert h['counts'][:, 1].sum() > 0 and h['counts'][:, 2].sum() > 0 and h['counts'][:, 3].sum() > 0
    same(dev_cover(gpu, fields, lays['full'], caps=0, host_offsets=True), h)


def test_batch_of_65_bare_paths_without_host_offsets_or_grid(gpu, batch65):
    fields, lays, host = batch65
    h = host[('bare', 1)]
    same(dev_cover(gpu, fields, lays['bare'], caps=1, host_offsets=False), h)
    same(dev_cover(gpu, fields, lays['bare'], caps=1, host_offsets=True, want_grid=False), h, with_grid=False)


# ---- second rounds: the chunk loop's ballot words and rounds, the early exit, the ring loops -----------------------------------------------------
# (tests/test_polygon_cover_host.py asserts without a device that every case reaches what it is named for)
@pytest.mark.parametrize('caps', [0, 1])
@pytest.mark.parametrize('count,permuted', MANY_CHUNKS)
def test_many_chunks_of_one_field(gpu, count, permuted, caps):
    """65 / 256 / 257 / 513 chunks: chunk base + w * 64 + bit of ballot words 1 .. 3, and of the second and third round of 256"""
    fields, lay = many_chunks_case(count, permuted)
    assert len(field_chunks(lay, 1)) == count
    same(dev_cover(gpu, fields, lay, caps=caps), host_cover(fields, W, RES, lay, caps=caps))


@pytest.mark.parametrize('rows,reverse', EARLY)
def test_a_tile_stops_only_when_all_its_cells_are_overlapped(gpu, rows, reverse):
    """the twin skips nothing.  'cover', listed order: every tile is all overlapped after 14 chunks and stops before the second round;
    reversed, the covering rows come last and stopping early would lose them.  'five': the margin rows stay open, no tile may stop,
    and what the later rounds' paths add there must show."""
    fields, lay, _ = early_exit_case(rows, reverse)
    same(dev_cover(gpu, fields, lay), host_cover(fields, W, RES, lay))


def test_many_rings(gpu):
    """259 rings (the sizes kernel's fifth round of 64, the tile kernel's bisection over 259 rings), 64 and 65 rings, and the copies
    whose LAST ring alone is spoilt: sizes, status, the inside bit and the counts"""
    fields, lay = many_rings_case()
    host = host_cover(fields, W_RINGS, RES_RINGS, lay)
    assert host['status'].tolist() == [0, -1, 0, -1, 0, -1, -1, -1] and host['counts'][[0, 2, 4], 1].all()
    same(dev_cover(gpu, fields, lay, res=RES_RINGS, width=W_RINGS), host)


# ---- against fcpp_cover_grid --------------------------------------------------------------------------------------------------------------------
def test_round_caps_equal_cover_grid_on_the_rectangle(gpu):
    path = np.concatenate([LONG, swaths(FIVE)[0][::-1], swaths(FIVE)[4], [[50.0, 30.0]]])
    out = dev_cover(gpu, [RECT40], layout(1, [path]), caps=1)
    gx, gy = out['dims'][0, :2].copy().view(np.float64)
    nx, ny = (int(v) for v in out['dims'][0, 2:])
    job = E.make_cover_job(gx, gy, RES, nx, ny, W / 2, len(path), shift=0.5, strict=True)
    counts, grid = E.cover_grid([job], path[:, 0], path[:, 1], want_grid=True)
    assert int(counts[0, 1]) == out['counts'][0, 1] + out['counts'][0, 3] > 0
    assert np.array_equal(grid.cpu().numpy() & 1, (out['grid'] >> 1) & 1)


# ---- through the public chain -------------------------------------------------------------------------------------------------------------------
def test_plan_polygon_fields_reports_what_polygon_coverage_gives(gpu):
    fields = [RECT40, [ELL, HOLE], star(7, 7)]
    kw = dict(width=W, radius=2.0, spacing=0.5, angles=[0.0, 0.5], passes=1)
    plan = E.plan_polygon_fields(fields, headland_paths=True, coverage_resolution=RES, **kw)
    cov = plan.coverage
    direct = E.polygon_coverage(fields, W, RES, paths=(plan.paths, plan.headland_paths), want_grid=True)
    assert np.array_equal(cov.counts.cpu().numpy(), direct.counts.cpu().numpy()) and np.array_equal(cov.status.cpu().numpy(), [0, 0, 0])
    assert np.array_equal(cov.dims.cpu().numpy(), direct.dims.cpu().numpy()) and np.array_equal(cov.cell_offsets_host, direct.cell_offsets_host)
    c = direct.counts.cpu().numpy()
    for i in range(3):
        g = direct.grid(i).cpu().numpy()
        assert g.shape == tuple(int(v) for v in direct.dims[i, [3, 2]].tolist())
        assert [np.count_nonzero(g & 1), np.count_nonzero((g & 3) == 3), np.count_nonzero((g & 5) == 5), np.count_nonzero((g & 3) == 2)] == c[i].tolist()
    assert np.allclose(direct.field_area.cpu().numpy(), c[:, 0] * RES * RES) and abs(float(direct.field_area[0]) - 800.0) < 1e-9
    assert np.allclose((direct.covered_area + direct.missed_area).cpu().numpy(), direct.field_area.cpu().numpy())
    assert np.allclose(direct.rate.cpu().numpy(), c[:, 1] / c[:, 0]) and (direct.rate > 0.5).all()
    assert np.array_equal(direct.overlap_area.cpu().numpy(), c[:, 2] * RES * RES) and np.array_equal(direct.spill_area.cpu().numpy(), c[:, 3] * RES * RES)
    # the same report from the raw arrays of the two path sets
    fp, hp = plan.paths, plan.headland_paths
    n_fp = int(fp.offsets.numel()) - 1
    ring = np.repeat(np.arange(len(hp.offsets_host) - 1), np.diff(hp.offsets_host))
    raw = E.polygon_coverage(fields, W, RES, paths=((fp.offsets, fp.x, fp.y, np.arange(n_fp), fp.part == 0, fp.leg),
                                                     (hp.offsets, hp.x, hp.y, hp.ring_pair[:, 0], (hp.part == 0) | (hp.part == 4), -1 - ring)))
    assert np.array_equal(raw.counts.cpu().numpy(), c)
    # without the argument nothing is reported; the loops only add to the rectangle's rate
    bare = E.plan_polygon_fields(fields, headland_paths=True, **kw)
    assert bare.coverage is None and bare.headland_paths is not None
    no_loops = E.plan_polygon_fields([RECT40], coverage_resolution=RES, **kw)
    with_loops = E.plan_polygon_fields([RECT40], headland_paths=True, coverage_resolution=RES, **kw)
    assert no_loops.headland_paths is None and float(with_loops.coverage.rate[0]) >= float(no_loops.coverage.rate[0]) > 0.0


# ---- guarded buffers ----------------------------------------------------------------------------------------------------------------------------
def _second_rounds_together():
    """the 257-path field and the 259-ring field in one batch, at the coarser resolution"""
    from tests.test_inset_host import HOLED
    fields, lay = many_chunks_case(257, True)
    assert len(field_chunks(lay, 1)) == 257 and len(HOLED) == 259
    poff = lay['path_offsets']
    paths = [np.column_stack([lay['x'][a:b], lay['y'][a:b]]) for a, b in zip(poff[:-1], poff[1:])]
    owner = np.empty(len(paths), np.int64)
    owner[lay['path_ids']] = np.repeat(np.arange(2), np.diff(lay['field_path_offsets']))
    pas = [lay['pass'][a] for a in poff[:-1]]
    return fields + [HOLED], layout(3, paths + [line(-3, -3, 173, 163, 60)], owner.tolist() + [2], pas=pas + [9], work=[None] * (len(paths) + 1))


@pytest.mark.parametrize('full', [True, False, 'second_rounds'], ids=['all_arrays', 'optional_arrays_null', 'second_rounds'])
def test_guarded_buffers(gpu, full):
    fields = [RECT40, NARROW65, [(0, 0), (10, 0), (10, np.nan), (0, 10)], [ELL, HOLE]]
    paths = swaths(FIVE) + [LONG, line(101, 2, 112, 2, 30), line(1, 1, 9, 9, 4), _zigzag(3, 40, (-5, -5), (65, 55))]
    owner = [0] * 6 + [1, 2, 3]
    rng = np.random.default_rng(2)
    W, RES = 4.0, 0.25
    if full == 'second_rounds':
        fields, lay = _second_rounds_together()
        RES = RES_RINGS
    elif full:
        lay = layout(4, paths, owner, work=[(rng.uniform(size=len(p)) < 0.9).astype(np.uint8) for p in paths], pas=[k % 3 for k in range(len(paths))],
                     order=rng.permutation(len(paths)).tolist())
    else:
        lay = layout(4, paths, owner)
    host = host_cover(fields, W, RES, lay, caps=0)
    ro, vo, x, y = pack(fields)
    n, total = len(fields), int(host['cell_offsets'][-1])
    # (no expected element may be all 0x5A bytes: the counts, offsets and dims of these fields are not)
    A = Arena().input('ro', ro).input('vo', vo).input('x', x).input('y', y)
    A.output('dims', np.int64, 4 * n).output('coff', np.int64, n + 1).output('status', np.int32, n).build(gpu.dev)
    head = lambda a: (gpu.h, n, a.ptr('ro'), len(vo) - 1, a.ptr('vo'), len(x), a.ptr('x'), a.ptr('y'), W, RES)
    gpu.ctx.bind_stream()
    assert gpu.lib.fcpp_polygon_cover_sizes(*head(A), A.ptr('dims'), A.ptr('coff'), None, A.ptr('status')) == 0, gpu.lib.fcpp_last_error()
    A.check(dict(dims=host['dims'].reshape(-1), coff=host['cell_offsets'], status=host['status']))
    B = Arena().input('ro', ro).input('vo', vo).input('x', x).input('y', y).input('poff', lay['path_offsets']).input('px', lay['x']).input('py', lay['y'])
    B.input('fpo', lay['field_path_offsets']).input('coff', host['cell_offsets'])
    for k, name in (('work', 'work'), ('pass', 'pass'), ('path_ids', 'ids')):
        if lay[k] is not None:
            B.input(name, lay[k])
    B.output('counts', np.int64, 4 * n)
    if full:
        B.output('grid', np.uint8, total).output('status', np.int32, n)
    B.build(gpu.dev)
    rc = gpu.lib.fcpp_polygon_cover(*head(B), 0, lay['n_paths'], B.ptr('poff'), None, len(lay['x']), B.ptr('px'), B.ptr('py'), B.ptr('work'), B.ptr('pass'),
                                    B.ptr('fpo'), B.ptr('ids'), B.ptr('coff'), None, B.ptr('grid'), B.ptr('counts'), B.ptr('status'))
    assert rc == 0, gpu.lib.fcpp_last_error()
    want = dict(counts=host['counts'].reshape(-1))
    if full:
        want.update(grid=host['grid'], status=host['status'])
    B.check(want)
