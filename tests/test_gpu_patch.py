"""The patch passes on the device (fcpp_patch_sizes / fcpp_patch_counts / fcpp_patch_fill: csrc/fcpp_patch.hip) against their host twin
(fcpp_debug_patch_swaths, tests/test_patch_host.py) -- frame, records, bitmap, run counts, offsets and every swath element, all == -- on
every shape of tests/patch_cases.py at four angles and two joins, on a batch of 65 mixed fields with and without the host copies of the
offsets, and on the second rounds DESIGN.md section 4 names: a line of 141 bitmap words (three rounds of the runs kernel's lanes) with a
gap across the first bin of round two, more lines than one launch of the runs kernel holds, more regions than one round of the scan, a
field of more than one numbering block and of no multiple of it, a wavefront with two labels and two bitmap words.  Then
engine.patch_swaths and plan_polygon_fields(patch=True) on a small planned holed square."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import patch_cases as P
from tests.support import Gpu as BaseGpu

pytestmark = pytest.mark.gpu

SHAPES = P.shapes()
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


def dev_patch(g, packed, angle, width=W, res=RES, margin=None, join=None, host_offsets=True):
    """the three device entries on exactly sized tensors, every output pre-filled with garbage -> the dict P.twin gives (numpy)"""
    torch = g.torch
    dims, off, flat, roff = packed
    n, k = len(dims), int(roff[-1])
    margin = res / 2 if margin is None else margin
    join = width if join is None else join
    th = P.angles_of(packed, angle)
    d_dims, d_off, d_lab, d_roff, d_th = g.up(dims), g.up(off), g.up(flat), g.up(roff), g.up(th)
    garbage = lambda count, dt: torch.full((count,), -7, dtype=dt, device=g.dev)
    i64, f64 = torch.int64, torch.float64
    frame, rec, totals = garbage(2 * n, f64), garbage(8 * k, i64), np.full(2, -7, np.int64)
    ho = (_hp(off), _hp(roff)) if host_offsets else (None, None)
    rule = (float(width), float(margin), float(join))
    g.ctx.bind_stream()
    rc = g.lib.fcpp_patch_sizes(g.h, n, _ptr(d_dims), _ptr(d_off), ho[0], float(res), _ptr(d_lab), _ptr(d_roff), ho[1], k, _ptr(d_th), *rule,
                                _ptr(frame), _ptr(rec), _hp(totals))
    assert rc == 0, g.lib.fcpp_last_error()
    nl, nw = int(totals[0]), int(totals[1])
    bitmap, cnt, loff, soff = garbage(nw, i64), garbage(nl, i64), garbage(nl + 1, i64), garbage(n + 1, i64)
    soff_h = np.full(n + 1, -7, np.int64)
    rc = g.lib.fcpp_patch_counts(g.h, n, _ptr(d_dims), _ptr(d_off), ho[0], float(res), _ptr(d_lab), _ptr(d_roff), ho[1], k, _ptr(frame), *rule, _ptr(rec),
                                 nl, nw, _ptr(bitmap), _ptr(cnt), _ptr(loff), _ptr(soff), _hp(soff_h) if host_offsets else None)
    assert rc == 0, g.lib.fcpp_last_error()
    soff_np = soff.cpu().numpy()
    if host_offsets:
        assert np.array_equal(soff_h, soff_np)
    ms = int(soff_np[-1])
    ax, ay, bx, by, length = (garbage(ms, f64) for _ in range(5))
    line, region = garbage(ms, torch.int32), garbage(ms, i64)
    before = [t.clone() for t in (frame, rec, bitmap, loff)]
    rc = g.lib.fcpp_patch_fill(g.h, n, _ptr(d_dims), float(res), _ptr(d_roff), ho[1], k, _ptr(frame), *rule, _ptr(rec), nl, nw, _ptr(bitmap), _ptr(loff), ms,
                               _ptr(ax), _ptr(ay), _ptr(bx), _ptr(by), _ptr(line), _ptr(length), _ptr(region))
    assert rc == 0, g.lib.fcpp_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d_lab.cpu().numpy(), flat) and np.array_equal(d_roff.cpu().numpy(), roff)        # inputs stay
    assert all(torch.equal(a, b) for a, b in zip(before, (frame, rec, bitmap, loff)))
    c = lambda t: t.cpu().numpy()
    return dict(frame=c(frame).reshape(n, 2), records=c(rec).view(P.REC), totals=np.array([nl, nw, ms], np.int64), bitmap=c(bitmap).view(np.uint64),
                line_counts=c(cnt), line_offsets=c(loff), swath_offsets=soff_np, ax=c(ax), ay=c(ay), bx=c(bx), by=c(by), line=c(line), length=c(length),
                region=c(region))


def same(dev, host):
    bad = P.same(dev, host)
    if bad is not None:
        d, h = np.asarray(dev[bad]).reshape(-1), np.asarray(host[bad]).reshape(-1)
        at = np.flatnonzero(d != h)[:6] if d.shape == h.shape else []
        raise AssertionError((bad, d.shape, h.shape, list(at), d[at].tolist() if len(at) else None, h[at].tolist() if len(at) else None))


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_every_host_shape_equals_the_twin(gpu, name):
    grids, n_reg = SHAPES[name]
    packed = P.pack(grids, n_reg)
    for angle in P.ANGLES:
        for join in P.JOINS:
            same(dev_patch(gpu, packed, angle, join=join), P.twin(packed, angle, join=join))


@pytest.fixture(scope='module')
def batch65():
    grids = P.mixed_batch(65)
    assert sum(g.size == 0 for g in grids) >= 5 and grids[0].shape == (1, 1) and grids[1].shape == (150, 200)
    packed = P.pack(grids)
    th = P.mixed_angles(65)
    return packed, th, {j: P.twin(packed, th, join=j) for j in P.JOINS}


@pytest.mark.parametrize('host_offsets', (True, False))
@pytest.mark.parametrize('join', P.JOINS)
def test_batch_of_65_mixed_fields(gpu, batch65, join, host_offsets):
    packed, th, host = batch65
    assert host[join]['totals'][2] > 500
    same(dev_patch(gpu, packed, th, join=join, host_offsets=host_offsets), host[join])


def test_no_field_no_region_and_only_empty_fields(gpu):
    for grids in ([], [np.zeros((0, 0), np.int32)] * 3, [P.lab((4, 4), np.zeros((4, 4), bool))]):
        packed = P.pack(grids)
        got = dev_patch(gpu, packed, 0.3)
        assert got['totals'].tolist() == [0, 0, 0] and got['swath_offsets'].tolist() == [0] * (len(grids) + 1)
        same(got, P.twin(packed, 0.3))


def test_margin_width_and_unsupported_regions(gpu):
    g = P.lab((3, 3), None, 1)
    g[0, 0] = g[2, 2] = 0
    one = P.lab((1, 2), None, 1)
    one[0, 0] = 0
    packed = P.pack([g, one])
    kw = dict(width=1e-7, margin=0.0, join=0.0)
    got = dev_patch(gpu, packed, 0.0, **kw)
    same(got, P.twin(packed, 0.0, **kw))
    assert got['records']['status'].tolist() == [L.EUNSUPPORTED, L.EUNSUPPORTED, 0, 0]
    packed = P.pack(SHAPES['blobs'][0])
    for kw in (dict(margin=0.0, join=0.5), dict(margin=1.0, join=40.0), dict(width=0.3, margin=0.1, join=0.0)):
        same(dev_patch(gpu, packed, -1.1, **kw), P.twin(packed, -1.1, **kw))


# ---- second rounds --------------------------------------------------------------------------------------------------------------------
def test_a_line_of_three_rounds_with_a_gap_across_the_round(gpu):
    """1 x 9000 at res 0.25, theta = 0: ONE line of 141 words, three rounds of the runs kernel's 64 lanes; 10 empty bins straddle bin
    4096.  join 0: the second run starts in round two and its previous set bin (4090) lies in round one -- the carried prefix max; join W:
    no start in round two or three, the only record is closed with the carried last set bin"""
    packed = P.pack([P.long_sliver()])
    split = dev_patch(gpu, packed, 0.0, join=0.0)
    same(split, P.twin(packed, 0.0, join=0.0))
    assert split['totals'].tolist() == [1, 141, 2] and np.allclose(split['length'], [4091 * 0.25 + 0.25, (9000 - 4101) * 0.25 + 0.25])
    joined = dev_patch(gpu, packed, 0.0, join=W)
    same(joined, P.twin(packed, 0.0, join=W))
    assert joined['totals'].tolist() == [1, 141, 1]
    # the same cells as a column: 9000 lines of one word at theta = 0, one line of 141 words at pi / 2
    col = P.pack([P.long_sliver().T.copy()])
    for angle in (0.0, np.pi / 2):
        same(dev_patch(gpu, col, angle, join=0.0), P.twin(col, angle, join=0.0))


def test_more_lines_than_one_launch_of_the_runs_kernel(gpu):
    """the runs kernel is launched with at most 4 workgroups of 4 wavefronts per compute unit, a wavefront per line; isolated cells, a
    region and a line each, until the lines need a second round -- also more regions than one round of 256 of the layout's scan, and more
    lines than one round of the offsets' scan"""
    g = P.many_lines(gpu.n_cu)
    packed = P.pack([g, P.lab((2, 2))])
    for join in P.JOINS:
        got = dev_patch(gpu, packed, 0.3, join=join)
        assert got['totals'][0] > P.runs_round_lines(gpu.n_cu) and int(packed[3][-1]) > 256
        same(got, P.twin(packed, 0.3, join=join))
        assert (got['line_counts'] == 1).all()


def test_fields_of_many_numbering_blocks(gpu):
    """the checkerboard (20 000 cells: 4 numbering blocks and 3616 cells, 10 000 regions: 40 rounds of the scan) and a 150 x 200 field of
    blobs (7 blocks and 1328 cells) whose regions span several blocks"""
    cb = SHAPES['checkerboard'][0][0]
    big = P.blobs(8, 150, 200, 50, 0.7)
    assert cb.size % P.BLOCK_CELLS == 3616 and big.size % P.BLOCK_CELLS == 1328
    assert len(np.unique(np.flatnonzero(big.reshape(-1) == 5) // P.BLOCK_CELLS)) >= 3          # one region's cells in three blocks
    packed = P.pack([cb, big])
    for angle in (0.0, 0.3):
        same(dev_patch(gpu, packed, angle), P.twin(packed, angle))


def test_a_wavefront_of_two_labels_and_two_words(gpu):
    packed = P.pack([P.two_labels_two_words()])
    for join in P.JOINS:
        got = dev_patch(gpu, packed, 0.0, join=join)
        same(got, P.twin(packed, 0.0, join=join))
    assert got['records']['B'].tolist() == [200, 130] and got['line_counts'].tolist() == [2, 1]          # (the 130 bins between region 0's halves exceed J = 16)


def test_call_errors_leave_every_output_untouched(gpu):
    torch = gpu.torch
    packed = P.pack([P.lab((4, 5)), P.lab((2, 2))])
    dims, off, flat, roff = packed
    n, k = 2, 2
    d_dims, d_off, d_lab, d_roff, d_th = gpu.up(dims), gpu.up(off), gpu.up(flat), gpu.up(roff), gpu.up(np.zeros(2))
    garbage = lambda count, dt: torch.full((count,), -7, dtype=dt, device=gpu.dev)
    i64, f64 = torch.int64, torch.float64
    frame, rec, totals = garbage(4, f64), garbage(16, i64), np.full(2, -7, np.int64)
    sizes = lambda *a: gpu.lib.fcpp_patch_sizes(*a)
    good = [gpu.h, n, _ptr(d_dims), _ptr(d_off), None, RES, _ptr(d_lab), _ptr(d_roff), None, k, _ptr(d_th), W, RES / 2, W, _ptr(frame), _ptr(rec),
            _hp(totals)]

    def with_(base, j, v):
        a = list(base)
        a[j] = v
        return a
    bad_off, bad_roff = [off + 1, off + np.array([0, 0, 1])], [roff + 1, roff[[0, 2, 1]] + np.array([0, 5, 0])]
    wrong = dims.copy()
    wrong[1, 2] += 1
    d_wrong = gpu.up(wrong)
    scalars = lambda w, m, j: ((w, 0.0), (w, -1.0), (w, np.nan), (m, -0.1), (m, 2.0), (m, np.inf), (j, -1.0), (j, np.nan), (5, 0.0), (5, -1.0), (5, np.inf))
    for j in (0, 2, 3, 6, 7, 10, 14, 15, 16):
        assert sizes(*with_(good, j, None)) == L.EINVAL, j
    for j, v in scalars(11, 12, 13):
        assert sizes(*with_(good, j, v)) == L.EINVAL, (j, v)
    for th in (np.nan, np.inf, 1.0001e5):
        d_bad = gpu.up(np.array([0.0, th]))
        assert sizes(*with_(good, 10, _ptr(d_bad))) == L.EINVAL
    for j, v in ((1, -1), (9, -1), (9, 3), (9, 1)):
        assert sizes(*with_(good, j, v)) == L.ESIZE, (j, v)
    for bad in bad_off:
        bad_h = np.ascontiguousarray(bad, dtype=np.int64)
        bad_d = gpu.up(bad_h)
        assert sizes(*with_(good, 3, _ptr(bad_d))) == L.ESIZE and sizes(*with_(good, 4, _hp(bad_h))) == L.ESIZE
    for bad in bad_roff:
        bad_h = np.ascontiguousarray(bad, dtype=np.int64)
        bad_d = gpu.up(bad_h)
        assert sizes(*with_(good, 7, _ptr(bad_d))) == L.ESIZE and sizes(*with_(good, 8, _hp(bad_h))) == L.ESIZE
    assert sizes(*with_(good, 2, _ptr(d_wrong))) == L.ESIZE
    torch.cuda.synchronize()
    assert (frame == -7).all() and (rec == -7).all() and totals.tolist() == [-7, -7]          # nothing ran
    assert sizes(*good) == 0
    nl, nw = (int(v) for v in totals)
    assert (nl, nw) == (2, 2)

    bitmap, cnt, loff, soff = garbage(nw, i64), garbage(nl, i64), garbage(nl + 1, i64), garbage(n + 1, i64)
    soff_h = np.full(n + 1, -7, np.int64)
    counts = lambda *a: gpu.lib.fcpp_patch_counts(*a)
    cgood = [gpu.h, n, _ptr(d_dims), _ptr(d_off), None, RES, _ptr(d_lab), _ptr(d_roff), None, k, _ptr(frame), W, RES / 2, W, _ptr(rec), nl, nw, _ptr(bitmap),
             _ptr(cnt), _ptr(loff), _ptr(soff), _hp(soff_h)]
    for j in (0, 2, 3, 6, 7, 10, 14, 17, 18, 19, 20):
        assert counts(*with_(cgood, j, None)) == L.EINVAL, j
    for j, v in scalars(11, 12, 13):
        assert counts(*with_(cgood, j, v)) == L.EINVAL, (j, v)
    for j, v in ((1, -1), (9, -1), (9, 3), (15, -1), (16, -1)):
        assert counts(*with_(cgood, j, v)) == L.ESIZE, (j, v)
    for bad in bad_off:
        bad_d = gpu.up(np.ascontiguousarray(bad, dtype=np.int64))
        assert counts(*with_(cgood, 3, _ptr(bad_d))) == L.ESIZE
    for bad in bad_roff:
        bad_d = gpu.up(np.ascontiguousarray(bad, dtype=np.int64))
        assert counts(*with_(cgood, 7, _ptr(bad_d))) == L.ESIZE
    assert counts(*with_(cgood, 2, _ptr(d_wrong))) == L.ESIZE
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in (bitmap, cnt, loff, soff)) and (soff_h == -7).all()          # nothing ran
    assert counts(*cgood) == 0
    ms = int(soff_h[-1])
    assert ms == 2

    outs = [garbage(ms, f64) for _ in range(4)] + [garbage(ms, torch.int32), garbage(ms, f64), garbage(ms, i64)]
    fill = lambda *a: gpu.lib.fcpp_patch_fill(*a)
    fgood = [gpu.h, n, _ptr(d_dims), RES, _ptr(d_roff), None, k, _ptr(frame), W, RES / 2, W, _ptr(rec), nl, nw, _ptr(bitmap), _ptr(loff), ms] \
        + [_ptr(t) for t in outs]
    for j in (0, 2, 4, 7, 11, 14, 15, 17, 18, 19, 20, 21, 22, 23):
        assert fill(*with_(fgood, j, None)) == L.EINVAL, j
    for j, v in scalars(8, 9, 10)[:-3] + ((3, 0.0), (3, -1.0), (3, np.inf)):
        assert fill(*with_(fgood, j, v)) == L.EINVAL, (j, v)
    for j, v in ((1, -1), (6, -1), (6, 3), (12, -1), (13, -1), (16, -1), (16, ms + 1), (16, ms - 1)):
        assert fill(*with_(fgood, j, v)) == L.ESIZE, (j, v)
    for bad in bad_roff:
        bad_d = gpu.up(np.ascontiguousarray(bad, dtype=np.int64))
        assert fill(*with_(fgood, 4, _ptr(bad_d))) == L.ESIZE
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in outs)          # nothing ran
    assert fill(*fgood) == 0
    torch.cuda.synchronize()
    assert not any((t == -7).any() for t in outs)


# ---- through the engine ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planned(gpu):
    kw = dict(width=W, radius=2.0, spacing=0.5, angles=[0.0, 0.5], passes=1)
    plan = E.plan_polygon_fields([HOLED], headland_paths=True, coverage_resolution=RES, **kw)
    cov = E.polygon_coverage([HOLED], W, RES, paths=(plan.paths, plan.headland_paths), want_grid=True)
    full = E.coverage_regions(cov, 'missed')
    cells = full.cells.cpu().numpy()
    cut = float(np.sort(cells)[len(cells) // 2]) * RES * RES          # the median region's area: it and the larger ones stay
    return kw, plan, cov, cut


def test_engine_patch_swaths_cover_every_kept_region(gpu, planned):
    kw, plan, cov, cut = planned
    torch = gpu.torch
    reg = E.coverage_regions(cov, 'missed', min_area=cut, want_labels=True)
    k = int(reg.offsets_host[-1])
    assert k >= 1 and int(reg.dropped[0, 0]) >= 1
    ss, info = E.patch_swaths(reg, W, plan.angle)
    packed = (cov.dims.cpu().numpy(), np.asarray(cov.cell_offsets_host, np.int64), reg.labels.cpu().numpy(), np.asarray(reg.offsets_host, np.int64))
    host = P.twin(packed, plan.angle.cpu().numpy())
    c = lambda t: t.cpu().numpy()
    assert np.array_equal(c(ss.offsets), host['swath_offsets']) and np.array_equal(ss.offsets_host, host['swath_offsets'])
    assert np.array_equal(c(ss.a), np.column_stack([host['ax'], host['ay']])) and np.array_equal(c(ss.b), np.column_stack([host['bx'], host['by']]))
    assert np.array_equal(c(ss.line), host['line']) and np.array_equal(c(ss.length), host['length']) and np.array_equal(c(info.region), host['region'])
    assert np.array_equal(c(info.records).view(P.REC).reshape(-1), host['records']) and np.array_equal(c(info.frame), host['frame'])
    assert np.array_equal(c(info.n_lines), host['records']['K']) and np.array_equal(c(info.status), host['records']['status'])
    assert c(ss.status).tolist() == [0] and c(ss.n_lines).tolist() == [host['records']['K'].sum()] and len(host['ax']) >= k
    assert torch.equal(ss.angle, plan.angle)
    # drive them and look again
    route = E.route_swaths(ss, kw['radius'], spacing=kw['spacing'])
    pp = E.field_paths(ss, kw['radius'], kw['spacing'], order=route)
    as_set = (pp.offsets, pp.x, pp.y, torch.zeros(1, dtype=torch.int64, device=gpu.dev), pp.part == 0, pp.leg + (1 << 30))
    after = E.polygon_coverage([HOLED], W, RES, paths=(plan.paths, plan.headland_paths, as_set), want_grid=True)
    lab, was, now = c(reg.labels), c(cov.cells), c(after.cells)
    kept, dropped = lab >= 0, lab == -2
    assert kept.sum() == c(reg.cells).sum() and dropped.sum() == int(reg.dropped[0, 1])
    assert (now[kept] & 2).all()                                        # every cell of every kept region is covered
    missed = lambda cc: int(cc[0, 0] - cc[0, 1])
    assert missed(c(cov.counts)) - missed(c(after.counts)) >= kept.sum()
    assert np.array_equal(now[dropped], was[dropped])                   # the cells of dropped regions are unchanged
    assert ((now & 2) >= (was & 2)).all() and np.array_equal(now & 1, was & 1)
    # the chain gives the same arrays, bit for bit
    with_ = E.plan_polygon_fields([HOLED], headland_paths=True, coverage_resolution=RES, missed_min_area=cut, patch=True, **kw)
    bits = lambda t: t.view(torch.uint8) if t.dtype.is_floating_point else t
    for name in ('offsets', 'a', 'b', 'line', 'length', 'status', 'n_lines', 'angle'):
        assert torch.equal(bits(getattr(with_.patch, name)), bits(getattr(ss, name))), name
    for name in ('region', 'n_lines', 'n_bins', 'status', 'frame', 'records'):
        assert torch.equal(bits(getattr(with_.patch_info, name)), bits(getattr(info, name))), name
    for name in ('offsets', 'x', 'y', 'heading', 'kappa', 'part', 'gear', 'leg'):
        assert torch.equal(bits(getattr(with_.patch_paths, name)), bits(getattr(pp, name))), name
    for name in ('counts', 'status', 'dims', 'cell_offsets', 'cells'):
        assert torch.equal(getattr(with_.coverage_after, name), getattr(after, name)), name
    assert torch.equal(with_.missed.labels, reg.labels) and torch.equal(with_.missed.first, reg.first)


def test_plan_without_patch_is_the_plan_of_today(gpu, planned):
    kw, plan, cov, cut = planned
    torch = gpu.torch
    again = E.plan_polygon_fields([HOLED], headland_paths=True, coverage_resolution=RES, missed_min_area=cut, **kw)
    patched = E.plan_polygon_fields([HOLED], headland_paths=True, coverage_resolution=RES, missed_min_area=cut, patch=True, **kw)
    assert again.patch is None and again.patch_info is None and again.patch_paths is None and again.coverage_after is None
    assert again.missed.labels is None and patched.missed.labels is not None and plan.patch is None and plan.missed is None
    bits = lambda t: t.view(torch.uint8) if t.dtype.is_floating_point else t
    for other in (again, patched):
        for name in ('angle_index', 'angle'):
            assert torch.equal(getattr(other, name), getattr(plan, name)), name
        for part, names in (('paths', ('offsets', 'x', 'y', 'heading', 'kappa', 'part', 'gear', 'leg')), ('headland_paths', ('offsets', 'x', 'y')),
                            ('coverage', ('counts', 'status', 'dims', 'cell_offsets')), ('swaths', ('offsets', 'a', 'b', 'line', 'length')),
                            ('work', ('x', 'y'))):
            for name in names:
                assert torch.equal(bits(getattr(getattr(other, part), name)), bits(getattr(getattr(plan, part), name))), (part, name)
        assert torch.equal(other.coverage.cells, cov.cells)
    for name in ('offsets', 'first', 'cells', 'bbox', 'sums', 'area', 'centroid', 'bounds', 'dropped'):
        assert torch.equal(bits(getattr(again.missed, name)), bits(getattr(patched.missed, name))), name
    with pytest.raises(ValueError):
        E.plan_polygon_fields([HOLED], headland_paths=True, coverage_resolution=RES, patch=True, **kw)
    with pytest.raises(ValueError):
        E.patch_swaths(again.missed, W, 0.0)                            # made without want_labels
    with pytest.raises(ValueError):
        E.patch_swaths(patched.missed, W, [0.0, 0.1])
