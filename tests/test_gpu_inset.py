"""GPU tests of the polygon inset (run with -m gpu on an MI355X): the kernels of csrc/fcpp_inset.hip against the same rule on the host
(fcpp_debug_inset) BIT FOR BIT -- both pair offset arrays, status, gap, the rings' vertex offsets, x, y and src.  Then the same call
through the guarded arena, and the Python layer: as_fields against the rings packed by hand, and headland -> best_swath_angle ->
polygon_swaths -> route_swaths with every swath end point at least two working widths from the ORIGINAL boundary.

The host reference is computed once per KIND of field at the three distances and shared: the rule takes every (field, distance) pair on
its own (tests/test_inset_host.py::test_statuses_leave_the_neighbours_alone asserts that on the host), so a batch's expected arrays are
the kinds' arrays laid end to end.  The edge counts straddle a wavefront (63 / 64 / 65: the one-wavefront kernel ends at 64 edges) and a
workgroup (256 / 257), the batch sizes 1 / 63 / 65 / 257 straddle them for the scan; 1024 is the edge cap and 1025 is over it.

Second rounds.  The workgroup kernel is launched 1024 pairs at a time: batches of 1023 / 1024 / 1025 / 2049 pairs end just under one
launch, at its end, one pair into a second launch and one pair into a third (LAUNCH_BATCHES).  The kernel's loops over a field's rings
stride by the workgroup's 256 threads: the field of 259 rings (tests/test_inset_host.py: HOLED) drives them into a second round, and
the two copies whose LAST ring alone is spoilt are EINVAL only if that round looks at it."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.guarded import Arena
from tests.support import bits as _bits, np_of as _np
from tests.test_inset_host import DUMBBELL, HOLED, HOLED_DISTS, POND_EDGE, SQUARE, HostInset, boundary_distance, spoilt_last_ring
from tests.test_swaths_host import COMB, ELL, HOLE, RECT, pack, rings_of, star

pytestmark = pytest.mark.gpu

DISTS = (1.6, 4.8, 8.0)
ARC_STEP = 0.1
P_TOL = 1e-9

NAN_FIELD = np.array(ELL, dtype=np.float64)
NAN_FIELD[3, 0] = np.nan
SMALL_SQUARE = np.array([(0, 0), (3, 0), (3, 3), (0, 3)], dtype=np.float64) + (5.0, 5.0)          # narrower than 2 d at every distance
KINDS = [('rect', RECT), ('ell', ELL), ('ell_hole', [ELL, HOLE]), ('comb', COMB), ('merge', [SQUARE, POND_EDGE]), ('dumbbell', DUMBBELL)] \
    + [('star%d' % m, star(m, m)) for m in (3, 7, 63, 64, 65, 257, 300, 1024)] + [('star1025', star(1025, 1025)), ('nan', NAN_FIELD),
                                                                                    ('empty', SMALL_SQUARE)]
SMALL_KINDS = [k for k in KINDS if len(np.concatenate(rings_of(k[1]))) <= 64]


@pytest.fixture(scope='module')
def kinds_host():
    """fcpp_debug_inset of every kind at the three distances, computed once and left unchanged"""
    return HostInset([f for _, f in KINDS], DISTS, ARC_STEP)


def expected(host, picks, cols):
    """the host's arrays for the batch of kinds `picks` at the distance columns `cols`, laid end to end"""
    pro, pvo, ovo, x, y, src, status, gap = [0], [0], [0], [], [], [], [], []
    for k in picks:
        for j in cols:
            p = k * host.D + j
            r0, r1, v0, v1 = host.pro[p], host.pro[p + 1], host.pvo[p], host.pvo[p + 1]
            ovo += (host.ovo[r0 + 1:r1 + 1] - v0 + pvo[-1]).tolist()
            pro.append(pro[-1] + r1 - r0)
            pvo.append(pvo[-1] + v1 - v0)
            x.append(host.x[v0:v1]); y.append(host.y[v0:v1]); src.append(host.src[v0:v1])
            status.append(host.status[k, j]); gap.append(host.gap[k, j])
    return dict(pro=np.asarray(pro, np.int64), pvo=np.asarray(pvo, np.int64), ovo=np.asarray(ovo, np.int64), x=np.concatenate(x),
                y=np.concatenate(y), src=np.concatenate(src).astype(np.int32), status=np.asarray(status, np.int32), gap=np.asarray(gap))


def assert_equal_bits(dev, want):
    assert np.array_equal(_np(dev.pair_ring_offsets), want['pro']) and np.array_equal(dev.pair_ring_offsets_host, want['pro'])
    assert np.array_equal(_np(dev.pair_vert_offsets), want['pvo']) and np.array_equal(dev.pair_vert_offsets_host, want['pvo'])
    assert np.array_equal(_np(dev.status).reshape(-1), want['status'])
    assert np.array_equal(_bits(_np(dev.gap).reshape(-1)), _bits(want['gap']))
    assert np.array_equal(_np(dev.ring_offsets), want['ovo'])
    assert np.array_equal(_np(dev.src), want['src'])
    assert np.array_equal(_bits(_np(dev.x)), _bits(want['x'])) and np.array_equal(_bits(_np(dev.y)), _bits(want['y']))


def test_the_kinds_are_what_they_are_there_for(kinds_host):
    names = [k for k, _ in KINDS]
    st = kinds_host.status
    assert (st[names.index('star1025')] == L.EUNSUPPORTED).all() and (st[names.index('nan')] == L.EINVAL).all()
    assert (st[names.index('star1024')] == 0).all() and (np.delete(st, [names.index('star1025'), names.index('nan')], axis=0) == 0).all()
    e = names.index('empty')
    assert all(kinds_host.pro[e * 3 + j + 1] == kinds_host.pro[e * 3 + j] for j in range(3))
    assert len(kinds_host.rings(names.index('merge'), 0)) == 1 and len(kinds_host.rings(names.index('star257'), 1)) == 4
    assert (kinds_host.src % 2 == 1).sum() > 1000 and kinds_host.gap.max() <= P_TOL


@pytest.mark.parametrize('cols', [(0,), (0, 1, 2)], ids=['D1', 'D3'])
@pytest.mark.parametrize('n', [1, 63, 65, 257])
def test_device_equals_host_bit_for_bit(kinds_host, n, cols):
    picks = [(i + 10) % len(KINDS) for i in range(n)]          # (a batch of one is the 65-vertex star)
    dev = E.polygon_inset([KINDS[k][1] for k in picks], [DISTS[j] for j in cols], ARC_STEP)
    assert_equal_bits(dev, expected(kinds_host, picks, cols))


@pytest.mark.parametrize('n', [1, 65])
def test_small_fields_one_wavefront_kernel(kinds_host, n):
    """a batch of fields of at most 64 edges runs the one-wavefront kernel with its pieces in LDS: the same bits"""
    names = [k for k, _ in KINDS]
    small = [names.index(k) for k, _ in SMALL_KINDS]
    assert {'star63', 'star64', 'ell_hole', 'nan', 'empty'} <= {k for k, _ in SMALL_KINDS} and 'star65' not in dict(SMALL_KINDS)
    picks = [small[(i + 8) % len(small)] for i in range(n)]
    dev = E.polygon_inset([KINDS[k][1] for k in picks], DISTS, ARC_STEP)
    assert_equal_bits(dev, expected(kinds_host, picks, (0, 1, 2)))


# ---- more than one launch of the workgroup kernel ------------------------------------------------------------------------------------------
LAUNCH_PAIRS = 1024          # INSET_LAUNCH_PAIRS of csrc/fcpp_inset.hip
# (fields, distance columns): 1023 = 341 x 3, 1024 = 512 x 2, 1025 = 205 x 5 (columns may repeat), 2049 = 683 x 3, 1025 = 1025 x 1
LAUNCH_BATCHES = [(341, (0, 1, 2)), (512, (0, 2)), (205, (0, 1, 2, 0, 1)), (683, (0, 1, 2)), (1025, (1,))]


def launch_picks(n, last):
    """KINDS cycled to n fields, turned so that the last field is the kind `last`"""
    names = [k for k, _ in KINDS]
    return [(i - (n - 1) + names.index(last)) % len(KINDS) for i in range(n)]


def assert_drives_the_launches(picks, cols, want, last_has_rings):
    """the CPU side of the launch tests: what the batch is named for, from the inputs and the twin's answer"""
    m = len(picks) * len(cols)
    launches = -(-m // LAUNCH_PAIRS)
    assert len(want['status']) == m and launches == {1023: 1, 1024: 1, 1025: 2, 2049: 3}[m]
    assert KINDS[picks[-1]][0] in ('star65', 'empty', 'nan') and sorted(set(picks)) == list(range(len(KINDS)))
    assert max(len(np.concatenate(rings_of(KINDS[k][1]))) for k in picks) > 64          # the workgroup kernel, not the one-wavefront one
    assert (want['pro'][-1] > want['pro'][-2]) == last_has_rings
    grows = np.diff(want['pro']) > 0
    for edge in range(LAUNCH_PAIRS, m, LAUNCH_PAIRS):          # pairs with rings just before every launch edge, and behind it
        assert grows[edge - 3 * len(KINDS):edge].any() and (grows[edge:].any() or not last_has_rings)
    if m == 2049:
        assert grows[LAUNCH_PAIRS:2 * LAUNCH_PAIRS].sum() > 500 and np.count_nonzero(want['status'][LAUNCH_PAIRS:2 * LAUNCH_PAIRS]) > 100


# every batch ending in a pair with rings; where a later launch exists, also ending in an empty inset and in a status (the launch's last
# workgroup returns early there and must still write the end of the rings' offsets)
LAUNCH_CASES = [(n, cols, 'star65') for n, cols in LAUNCH_BATCHES] + [(n, cols, last) for n, cols in LAUNCH_BATCHES[2:] for last in ('empty', 'nan')]
LAUNCH_IDS = ['%dx%d-%s' % (n, len(c), last) for n, c, last in LAUNCH_CASES]


@pytest.mark.parametrize('n,cols,last', LAUNCH_CASES, ids=LAUNCH_IDS)
def test_more_pairs_than_one_launch(kinds_host, n, cols, last):
    """pair = pair0 + blockIdx.x with the slabs by blockIdx.x; out_vert_offsets[total_rings] from the LAST launch, whether its pair has
    rings or returns early (empty, a status).  The inputs' side is asserted without a device in tests/test_inset_host.py."""
    picks = launch_picks(n, last)
    want = expected(kinds_host, picks, cols)
    assert_drives_the_launches(picks, cols, want, last == 'star65')
    dev = E.polygon_inset([KINDS[k][1] for k in picks], [DISTS[j] for j in cols], ARC_STEP)
    assert_equal_bits(dev, want)


# ---- more rings than the workgroup has threads ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def holed_host():
    fields = [spoilt_last_ring(HOLED, 'nan'), HOLED, [ELL, HOLE], spoilt_last_ring(HOLED, 'short')]
    return fields, HostInset(fields, HOLED_DISTS, ARC_STEP)


def holed_want(h):
    return dict(pro=h.pro, pvo=h.pvo, ovo=h.ovo, x=h.x, y=h.y, src=h.src, status=h.status.reshape(-1), gap=h.gap.reshape(-1))


def test_more_rings_than_threads(holed_host):
    """the validity pass and the orientation pass stride over the field's rings by 256: rings 256 .. 258 are the second round's.  The
    spoilt copies are sound up to ring 257; the intact field's last holes are oriented (and so inset) only by that round."""
    fields, h = holed_host
    assert [len(f) for f in fields] == [259, 259, 2, 259]
    assert h.status.tolist() == [[L.EINVAL] * 3, [0] * 3, [0] * 3, [L.EINVAL] * 3]
    n_out = [len(h.rings(1, j)) for j in range(3)]
    assert n_out[0] == n_out[1] == 259 and 1 < n_out[2] != 259          # apart, apart, merged: read from the twin
    dev = E.polygon_inset(fields, HOLED_DISTS, ARC_STEP)
    assert_equal_bits(dev, holed_want(h))


def guarded_counts_and_fill(fields, dists, want):
    """fcpp_inset_counts and fcpp_inset_fill once each, every output on a guarded arena"""
    ctx = E.get_context(None)
    ctx.bind_stream()
    import torch
    dev = torch.device('cuda', ctx.device)
    ro, vo, x, y = pack(fields)
    n, D = len(fields), len(dists)
    m, R, V = n * D, int(want['pro'][-1]), int(want['pvo'][-1])

    def inputs(A):
        return A.input('ro', ro).input('vo', vo).input('x', x).input('y', y).input('dist', np.asarray(dists, dtype=np.float64))

    def head(A):
        return (n, A.ptr('ro'), len(vo) - 1, A.ptr('vo'), len(x), A.ptr('x'), A.ptr('y'), D, A.ptr('dist'), ARC_STEP)

    A = inputs(Arena())
    A.output('pro', np.int64, m + 1).output('pvo', np.int64, m + 1).output('status', np.int32, m).output('gap', np.float64, m).build(dev)
    assert ctx.lib.fcpp_inset_counts(ctx.handle, *head(A), A.ptr('pro'), None, A.ptr('pvo'), None, A.ptr('status'), A.ptr('gap')) == L.OK
    A.check({k: want[k] for k in ('pro', 'pvo', 'status', 'gap')})
    A = inputs(Arena()).input('pro', want['pro']).input('pvo', want['pvo'])
    A.output('ovo', np.int64, R + 1).output('ox', np.float64, V).output('oy', np.float64, V).output('src', np.int32, V).build(dev)
    assert ctx.lib.fcpp_inset_fill(ctx.handle, *head(A), A.ptr('pro'), A.ptr('pvo'), R, V, A.ptr('ovo'), A.ptr('ox'), A.ptr('oy'), A.ptr('src')) == L.OK
    A.check(dict(ovo=want['ovo'], ox=want['x'], oy=want['y'], src=want['src']))


def test_guarded_second_launch(kinds_host):
    """1025 pairs: the one pair of the second launch writes its counts, its rings and the end of the rings' offsets, and nothing beside"""
    n, cols = LAUNCH_BATCHES[2]
    picks = launch_picks(n, 'star65')
    want = expected(kinds_host, picks, cols)
    assert len(want['status']) == 1025 and want['pro'][-1] > want['pro'][-2]
    guarded_counts_and_fill([KINDS[k][1] for k in picks], [DISTS[j] for j in cols], want)


def test_guarded_more_rings_than_threads(holed_host):
    fields, h = holed_host
    guarded_counts_and_fill(fields, HOLED_DISTS, holed_want(h))


# ---- the guarded arena ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('small', [True, False], ids=['wavefront', 'workgroup'])
def test_guarded_counts_and_fill(kinds_host, small):
    ctx = E.get_context(None)
    ctx.bind_stream()
    import torch
    dev = torch.device('cuda', ctx.device)
    names = [k for k, _ in KINDS]
    picks = [names.index(k) for k in (('ell_hole', 'nan', 'star7', 'empty', 'star64', 'merge') if small else
                                      ('ell_hole', 'star1025', 'star65', 'nan', 'empty', 'star257', 'dumbbell'))]
    want = expected(kinds_host, picks, (0, 1, 2))
    ro, vo, x, y = pack([KINDS[k][1] for k in picks])
    n, m = len(picks), len(picks) * 3
    R, V = int(want['pro'][-1]), int(want['pvo'][-1])
    assert (want['status'] != 0).sum() >= 3 and R > 8 and V > 100

    def inputs(A):
        return A.input('ro', ro).input('vo', vo).input('x', x).input('y', y).input('dist', np.asarray(DISTS))

    def head(A):
        return (n, A.ptr('ro'), len(vo) - 1, A.ptr('vo'), len(x), A.ptr('x'), A.ptr('y'), 3, A.ptr('dist'), ARC_STEP)

    for outs in (('status', 'gap'), ('status',), ()):
        A = inputs(Arena())
        A.output('pro', np.int64, m + 1).output('pvo', np.int64, m + 1)
        if 'status' in outs:
            A.output('status', np.int32, m)
        if 'gap' in outs:
            A.output('gap', np.float64, m)
        A.build(dev)
        assert ctx.lib.fcpp_inset_counts(ctx.handle, *head(A), A.ptr('pro'), None, A.ptr('pvo'), None, A.ptr('status'), A.ptr('gap')) == L.OK
        A.check({k: want[k] for k in ('pro', 'pvo') + outs})
    # the fill: pairs with a status or an empty inset own empty ranges and leave everything alone; the good pairs' slots are fully written
    # (check() accepts no element that still holds the pre-fill)
    want.update(ox=want['x'], oy=want['y'])
    for outs in (('ovo', 'ox', 'oy', 'src'), ('src',), ('ox',), ('ovo',)):
        A = inputs(Arena())
        A.input('pro', want['pro']).input('pvo', want['pvo'])
        for k, (dt, cnt) in dict(ovo=(np.int64, R + 1), ox=(np.float64, V), oy=(np.float64, V), src=(np.int32, V)).items():
            if k in outs:
                A.output(k, dt, cnt)
        A.build(dev)
        assert ctx.lib.fcpp_inset_fill(ctx.handle, *head(A), A.ptr('pro'), A.ptr('pvo'), R, V, A.ptr('ovo'), A.ptr('ox'), A.ptr('oy'), A.ptr('src')) == L.OK
        A.check({k: want[k] for k in outs})


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
def test_as_fields_equals_the_rings_packed_by_hand(kinds_host):
    names = [k for k, _ in KINDS]
    picks = [names.index(k) for k in ('ell_hole', 'empty', 'star257', 'nan', 'dumbbell', 'merge')]
    ins = E.polygon_inset([KINDS[k][1] for k in picks], DISTS, ARC_STEP)
    for j in range(3):
        pf = ins.as_fields(j)
        ro, vo, x, y = pack([kinds_host.rings(k, j) for k in picks])
        assert np.array_equal(_np(pf.ring_offsets), ro) and np.array_equal(_np(pf.vert_offsets), vo)
        assert np.array_equal(_bits(_np(pf.x)), _bits(x)) and np.array_equal(_bits(_np(pf.y)), _bits(y))
        for i, k in enumerate(picks):
            got = [_np(r) for r in ins.rings(i, j)]
            assert len(got) == len(kinds_host.rings(k, j)) and all(np.array_equal(a, b) for a, b in zip(got, kinds_host.rings(k, j)))


def test_headland_feeds_the_swath_pipeline():
    W, passes = 3.2, 2
    d = passes * W
    field = [ELL, HOLE]
    lines, work = E.headland([field, SMALL_SQUARE, DUMBBELL], W, passes, arc_step=ARC_STEP)
    assert lines.D == passes and _np(lines.distances).tolist() == [W / 2, W / 2 + W] and (_np(lines.status)[[0, 2]] == 0).all()
    assert work.n == 3 and _np(work.ring_offsets)[1] == _np(work.ring_offsets)[2]          # the small square's work area is empty
    angles = np.linspace(0.0, np.pi, 12, endpoint=False)
    idx, _ = E.best_swath_angle(work, angles, W)
    assert _np(idx)[1] == -1 and (_np(idx)[[0, 2]] >= 0).all()
    ss = E.polygon_swaths(work, angles[np.maximum(_np(idx), 0)], W)
    assert _np(ss.status).tolist() == [0, L.EINVAL, 0]                                      # reported per field, the rest is planned
    rt = E.route_swaths(ss, 8.0)
    assert (_np(rt.status)[[0, 2]] == 0).all()
    off = ss.offsets_host
    assert off[1] >= 8 and off[2] == off[1] and off[3] > off[2]
    assert sorted(_np(rt.field(0)) // 2) == list(range(off[1]))                             # every swath of the L once
    ends = np.vstack([_np(ss.a)[off[0]:off[1]], _np(ss.b)[off[0]:off[1]]])
    dist = boundary_distance(ends, field)
    # The end points are crossings of the work area's rings.  On an offset edge they lie d from the boundary; on the inscribed chord of an
    # arc no nearer than d cos(arc_step / 2).  Which it is: the ring edge an end point lies on, and the src of that edge's first vertex.
    alone = E.polygon_inset([field], [d], ARC_STEP)
    rings = [_np(r) for r in alone.rings(0, 0)]
    src = _np(alone.src)
    p = np.concatenate(rings)
    q = np.concatenate([np.roll(r, -1, axis=0) for r in rings])
    assert np.array_equal(_bits(p[:, 0]), _bits(_np(work.x)[:len(p)]))                      # the work area IS that inset
    ab = q - p
    t = np.clip(((ends[:, None, :] - p[None]) * ab[None]).sum(axis=2) / (ab * ab).sum(axis=1)[None], 0.0, 1.0)
    r = ends[:, None, :] - p[None] - t[:, :, None] * ab[None]
    on = np.hypot(r[:, :, 0], r[:, :, 1])
    edge = on.argmin(axis=1)
    assert on.min(axis=1).max() <= P_TOL                                                    # every end point lies on the ring
    chord = src[edge] % 2 == 1
    bound = np.where(chord, d * np.cos(ARC_STEP / 2), d) - P_TOL
    print('swath end points:', len(ends), 'on chords:', chord.sum(), 'least distance', dist.min(), 'least margin', (dist - bound).min())
    assert (dist >= bound).all()
