"""GPU tests of the field paths (run with -m gpu on an MI355X): the kernels of csrc/fcpp_legs.hip against the same rule on the host
(fcpp_debug_field_paths) BIT FOR BIT on every output -- the rule is one set of host+device expressions, so nothing here is compared to a
bound; then against the parent's per-field path, swath_route, through the project's own operators; the existing path operators fed the
whole batch in one call each; plan_polygon_fields against the stage-by-stage calls; and the two device entries through the guarded arena.

The batches are those of tests/test_gpu_route.py: strips of 0, 1, 2, 3, 4, 5, 63, 64, 65 and 130 swaths (the strip of 130 alone has 261 leg
slots: the 256-lane scan of the slot counts wraps inside one field, and many times in the batch of 65), the square with a hole, the L with
its hole, a 65-vertex star and a field with a NaN vertex (no swaths).  R = 6 as in tests/test_route_host.py.

Against swath_route: the sample counts and `part` are equal, the connector samples equal bit for bit (the same device function), the
headings equal after wrapping the difference (swath_route leaves theta + pi unwrapped), the swath samples within 1e-12 m: both sides
evaluate sx + min(k spacing / len, 1) (ex - sx); a one-ulp difference in torch's division would move a point by at most 2^-52 x 40 m, about
1e-14 m, so the bound is 100 times that.  MEASURED on the MI355X (test_against_swath_route prints it): the swath samples' bits were NOT all
equal -- the largest distance was 3.553e-15 m in all eight cases (one ulp of a coordinate near 20 m), 280 times below the bound."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests.guarded import Arena
from tests.support import np_of as _np
from tests.test_field_paths_host import SAMPLE_KEYS, SAMPLE_TYPES, host_paths, stored_order, wrap_diff
from tests.test_gpu_route import W, batch, field_poses
from tests import test_leg_paths_pinned as PIN
from tests.test_guarded_host import strip
from tests.test_route_host import HOLED_SQUARE, R, bits, cut_with_angle
from tests.test_swaths_host import ELL, HOLE

pytestmark = pytest.mark.gpu

FIELD_KEYS = ('offsets', 'leg_offsets', 'work', 'transit', 'status')
DEV_NAMES = dict(offsets='offsets', leg_offsets='leg_offsets', work='work_length', transit='transit_length', status='status')


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


@pytest.fixture(scope='module')
def reference():
    """per batch size: the fields, the host's cut and the device's -- computed once, left unchanged"""
    out = {}
    for n in (1, 65):
        fields, angles = batch(n)
        cut = cut_with_angle(fields, angles, W)
        ss = E.polygon_swaths(fields, angles, W)
        assert np.array_equal(ss.offsets_host, cut['offsets']) and np.array_equal(bits(_np(ss.a)), bits(cut['a']))
        assert np.array_equal(bits(_np(ss.length)), bits(cut['length']))
        out[n] = (fields, cut, ss)
    assert 130 in np.diff(out[65][1]['offsets']) and 0 in np.diff(out[65][1]['offsets'])
    return out


@pytest.fixture(scope='module')
def routes(reference):
    """a routed order per (batch, mode, with entry / exit): two candidates, three sweeps -- an order that is not the stored one"""
    out = {}
    for n in (1, 65):
        ss = reference[n][2]
        entry, exit = field_poses(n)
        for mode in (0, 1):
            for ends in (False, True):
                r = E.route_swaths(ss, R, reversing=bool(mode), entry=entry if ends else None, exit=exit if ends else None, starts=2, max_sweeps=3,
                                   spacing=0.5)
                out[n, mode, ends] = _np(r.order)
        assert not np.array_equal(out[n, 0, False], stored_order(reference[n][1]['offsets']))
    return out


def assert_equals_host(fp, host):
    for k in FIELD_KEYS:
        assert same_bytes(_np(getattr(fp, DEV_NAMES[k])), host[k]), k
    assert np.array_equal(fp.offsets_host, host['offsets'])
    for k in SAMPLE_KEYS:
        assert same_bytes(_np(getattr(fp, k)), host[k]), k


@pytest.mark.parametrize('ends', [False, True], ids=['open', 'ends'])
@pytest.mark.parametrize('routed', [False, True], ids=['stored', 'routed'])
@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
@pytest.mark.parametrize('n', [1, 65])
def test_device_equals_host_bit_for_bit(reference, routes, n, mode, routed, ends):
    _, cut, ss = reference[n]
    entry, exit = field_poses(n) if ends else (None, None)
    order = routes[n, mode, ends] if routed else None
    for spacing in (0.5, 7.0):
        host = host_paths(cut, E._chord_radius(R, spacing), spacing, mode, order=order, entry=entry, exit=exit)
        fp = E.field_paths(ss, R, spacing, reversing=bool(mode), order=order, entry=entry, exit=exit)
        assert np.all(host['status'] == 0) and host['total'] > (0 if n == 1 and not ends else 100)
        assert_equals_host(fp, host)
        if mode:
            assert (host['gear'] == -1).any() or n == 1
        assert set(np.unique(host['part']).tolist()) == ({0, 1, 2, 3} if ends else {0, 1})


@pytest.mark.parametrize('name', PIN.FIELD_NAMES)
def test_device_gives_the_recorded_field_paths(name):
    """the device entries on the cases of tests/test_leg_paths_pinned.py against the recording: the per-field and per-slot arrays byte for
    byte, the seven sample columns by their SHA-256"""
    import torch
    cut, kw = PIN.field_cases()[name]
    dev = torch.device('cuda', E.get_context(None).device)
    t = {k: torch.as_tensor(np.array(cut[k]), device=dev) for k in ('offsets', 'a', 'b', 'line', 'length', 'angle')}
    ss = E.SwathSet(t['offsets'], cut['offsets'], t['a'], t['b'], t['line'], t['length'], None, None, t['angle'])
    fp = E.field_paths(ss, R, kw['spacing'], reversing=bool(kw['mode']), order=kw['order'], entry=kw['entry'], exit=kw['exit'])
    got = {k: _np(getattr(fp, DEV_NAMES[k])) for k in FIELD_KEYS}
    got.update({k: _np(getattr(fp, k)) for k in SAMPLE_KEYS})
    PIN.assert_pinned(name, got, PIN.FIELD_FULL, PIN.DIGESTS)
    assert np.array_equal(fp.offsets_host, got['offsets'])


def test_failed_fields_on_the_device(reference):
    """an order with a swath twice, an entry of 2 m, a NaN length and a NaN entry pose, each in a field of its own among good ones"""
    import torch
    _, cut, ss = reference[65]
    soff = cut['offsets']
    m = np.diff(soff)
    victims = [int(i) for i in np.flatnonzero(m >= 2)[[0, 1, 2, 3]]]
    order = stored_order(soff)
    order[soff[victims[0]] + 1] = order[soff[victims[0]]] ^ 1
    order[soff[victims[1]]] = 2 * m[victims[1]]
    length = cut['length'].copy()
    length[soff[victims[2]] + 1] = np.nan
    entry, exit = field_poses(65)
    entry[victims[3], 2] = np.nan
    host = host_paths(cut, E._chord_radius(R, 0.5), 0.5, 0, order=order, entry=entry, exit=exit, length=length)
    assert sorted(np.flatnonzero(host['status'] == L.EINVAL).tolist()) == sorted(victims) and set(host['status'].tolist()) == {0, L.EINVAL}
    bad = E.SwathSet(ss.offsets, ss.offsets_host, ss.a, ss.b, ss.line, torch.as_tensor(length, device=ss.length.device), ss.status, ss.n_lines, ss.angle)
    fp = E.field_paths(bad, R, 0.5, order=order, entry=entry, exit=exit)
    for k in ('offsets', 'leg_offsets', 'status') + SAMPLE_KEYS:
        assert same_bytes(_np(getattr(fp, DEV_NAMES.get(k, k))), host[k]), k
    # (NaN totals: equal as NaN, whatever the payload)
    assert np.array_equal(_np(fp.work_length), host['work'], equal_nan=True) and np.array_equal(_np(fp.transit_length), host['transit'], equal_nan=True)
    assert np.isnan(host['work'][victims]).all() and all(host['offsets'][i + 1] == host['offsets'][i] for i in victims)
    good = host_paths(cut, E._chord_radius(R, 0.5), 0.5, 0, order=stored_order(soff), entry=field_poses(65)[0], exit=exit)
    for i in range(65):
        if i not in victims:
            a, b = (slice(int(h['offsets'][i]), int(h['offsets'][i + 1])) for h in (host, good))
            assert same_bytes(host['x'][a], good['x'][b]) and same_bytes(host['gear'][a], good['gear'][b])
    with pytest.raises(L.FcppError):
        E.field_paths(ss, -1.0, 0.5)
    with pytest.raises(L.FcppError):
        E.field_paths(ss, R, float('nan'))


# ---- against the parent's per-field path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('routed', [False, True], ids=['stored', 'routed'])
@pytest.mark.parametrize('reversing', [False, True], ids=['dubins', 'rs'])
def test_against_swath_route(reversing, routed):
    """MEASURED on the MI355X: 'swath bits equal False, max distance 3.553e-15 m' in every case: torch's division and the rule's differ by
    an ulp in some samples; the connector samples, counts, parts and wrapped headings were equal."""
    fields = [HOLED_SQUARE, strip(5)]
    ss = E.polygon_swaths(fields, 0.0, 4.0)
    assert list(np.diff(ss.offsets_host)) == [14, 4]           # (a strip of 5 widths of 3.2 m holds 4 lines at W = 4)
    route = E.route_swaths(ss, R, reversing=reversing, spacing=0.5) if routed else None
    fp = E.field_paths(ss, R, 0.5, reversing=reversing, order=route)
    assert np.all(_np(fp.status) == 0)
    for i in range(2):
        x, y, h, part = (_np(t) for t in E.swath_route(ss, i, R, 0.5, reversing=reversing, order=route))
        fx, fy, fh, fpart = (_np(t) for t in fp.field(i))
        assert len(fx) == len(x) and np.array_equal(fpart, part)
        con = part == 1
        assert con.sum() > 100 and same_bytes(fx[con], x[con]) and same_bytes(fy[con], y[con]) and same_bytes(fh[con], h[con])
        assert np.all(wrap_diff(fh, h) <= 1e-15) and np.all((fh > -np.pi) & (fh <= np.pi))
        d = np.hypot(fx[~con] - x[~con], fy[~con] - y[~con])
        print('field %d reversing=%s routed=%s: %d samples, swath bits equal %s, max distance %.3e m'
              % (i, reversing, routed, len(x), same_bytes(fx[~con], x[~con]) and same_bytes(fy[~con], y[~con]), d.max()))
        assert d.max() <= 1e-12


# ---- the existing path operators, one call each on the whole batch ---------------------------------------------------------------------------
def test_path_operators_take_the_batch(reference):
    _, cut, ss = reference[65]
    fp = E.field_paths(ss, R, 0.5)
    n = 65
    veh = E.make_vehicle(min_turn_radius=R)
    # a speed just under the clamp's limit at the curvature bound 1 / R + 1e-6 of tests/test_gpu_swaths.py
    v_lim = np.sqrt(veh.max_lateral_accel / (1 / R + 1e-6)) * veh.safety_factor * 3.6
    v = np.full(int(fp.x.numel()), 0.999 * v_lim)
    kap = _np(E.curvature(fp.x, fp.y, offsets=fp.offsets))
    vout, nadj = E.speed_plan(fp.x, fp.y, v, veh, clamp=True, offsets=fp.offsets)
    flags, stats = E.validate(fp.x, fp.y, v, veh, offsets=fp.offsets)
    vout, nadj, flags = _np(vout), _np(nadj), _np(flags)
    assert nadj.shape == (n,) and np.all(nadj == 0)             # the Dubins batch passes the clamp untouched
    assert kap.max() <= 1 / R + 1e-6
    checked = 0
    for i in range(n):
        s = slice(int(fp.offsets_host[i]), int(fp.offsets_host[i + 1]))
        if s.stop == s.start:
            continue
        x, y, _, _ = fp.field(i)
        assert same_bytes(_np(E.curvature(x, y)), kap[s])
        vi, ni = E.speed_plan(x, y, v[s], veh, clamp=True)
        assert same_bytes(_np(vi), vout[s]) and int(ni[0]) == nadj[i]
        fi, si = E.validate(x, y, v[s], veh)
        assert same_bytes(_np(fi), flags[s])
        for k in stats:
            assert same_bytes(si[k][:1], stats[k][i:i + 1]), (k, i)
        checked += 1
    assert checked >= 55


# ---- the whole chain ----------------------------------------------------------------------------------------------------------------------
def test_plan_polygon_fields():
    sliver = [(100.0, 0.0), (150.0, 0.0), (150.0, 3.0), (100.0, 3.0)]
    fields = [HOLED_SQUARE, [ELL, HOLE], sliver]
    angles = np.arange(12) * (np.pi / 12)
    entry, exit = field_poses(3)
    plan = E.plan_polygon_fields(fields, 4.0, R, 0.5, angles, passes=1, turn_cost=5.0, entry=entry, exit=exit)
    fp = plan.paths
    assert int(plan.angle_index[2]) == -1 and int(plan.swaths.status[2]) == L.EINVAL and np.diff(plan.swaths.offsets_host)[2] == 0
    assert fp.offsets_host[3] == fp.offsets_host[2] and _np(fp.status).tolist() == [0, 0, 0]
    assert np.all(_np(plan.angle_index)[:2] >= 0) and np.all(np.diff(fp.offsets_host)[:2] > 200)
    # stage by stage on the two fields that have a work area
    lines, work = E.headland(fields[:2], 4.0, 1)
    idx, _ = E.best_swath_angle(work, angles, 4.0, 5.0)
    assert np.array_equal(_np(idx), _np(plan.angle_index)[:2])
    ss = E.polygon_swaths(work, angles[_np(idx)], 4.0)
    route = E.route_swaths(ss, R, entry=entry[:2], exit=exit[:2], starts=8, spacing=0.5)
    want = E.field_paths(ss, R, 0.5, order=route, entry=entry[:2], exit=exit[:2])
    assert np.array_equal(_np(route.order), _np(plan.route.order)) and same_bytes(_np(route.cost), _np(plan.route.cost)[:2])
    assert np.array_equal(want.offsets_host, fp.offsets_host[:3])
    total = int(want.offsets_host[-1])
    for k in SAMPLE_KEYS:
        assert same_bytes(_np(getattr(want, k)), _np(getattr(fp, k))[:total]), k
    assert same_bytes(_np(want.work_length), _np(fp.work_length)[:2]) and same_bytes(_np(want.transit_length), _np(fp.transit_length)[:2])
    # the route's cost is what the path drives (the router's mirrored pairs: tests/test_gpu_route.py's tolerance)
    cost = _np(plan.route.cost)[:2]
    assert np.all(np.abs(_np(fp.transit_length)[:2] - cost) <= 1e-9 * (1 + cost))


# ---- the two device entries through the guarded arena ------------------------------------------------------------------------------------
FILL_SUBSETS = [SAMPLE_KEYS, ('part',), ('x',)]


@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
def test_guarded_buffers(reference, routes, mode):
    import torch
    _, cut, _ = reference[65]
    ctx = E.get_context(None)
    lib, h = ctx.lib, ctx.handle
    dev = torch.device('cuda', ctx.device)
    ctx.bind_stream()
    soff = cut['offsets']
    n, nt = len(soff) - 1, int(soff[-1])
    order = np.ascontiguousarray(routes[65, mode, True], dtype=np.int32)
    entry, exit = field_poses(n)
    radius = E._chord_radius(R, 0.5)
    host = host_paths(cut, radius, 0.5, mode, order=order, entry=entry, exit=exit)
    inputs = dict(soff=soff, ax=cut['ax'], ay=cut['ay'], bx=cut['bx'], by=cut['by'], length=cut['length'], angle=cut['angle'], order=order)
    for name, pose in (('e', entry), ('x', exit)):
        for k, c in enumerate('xyh'):
            inputs[name + c] = np.ascontiguousarray(pose[:, k])

    def arena(extra=()):
        A = Arena()
        for k, a in inputs.items():
            A.input(k, a)
        for k, a in extra:
            A.input(k, a)
        return A

    def head(A, soff_host):
        return (h, n, A.ptr('soff'), E._host_ptr(soff_host), nt, A.ptr('ax'), A.ptr('ay'), A.ptr('bx'), A.ptr('by'), A.ptr('length'), A.ptr('angle'),
                A.ptr('order'), radius, mode, 0.5, A.ptr('ex'), A.ptr('ey'), A.ptr('eh'), A.ptr('xx'), A.ptr('xy'), A.ptr('xh'))

    count_outs = (('offsets', np.int64, n + 1), ('leg_offsets', np.int64, 2 * nt + n + 1), ('work', np.float64, n), ('transit', np.float64, n),
                  ('status', np.int32, n))
    for outs in (FIELD_KEYS, ('offsets', 'leg_offsets')):
        A = arena()
        for k, dt, size in count_outs:
            if k in outs:
                A.output(k, dt, size)
        A.build(dev)
        off_h = np.full(n + 1, -1, np.int64)
        # (the second call has the library read the swath offsets back from the arena)
        rc = lib.fcpp_field_path_counts(*head(A, soff if outs is FIELD_KEYS else None), A.ptr('offsets'), E._host_ptr(off_h), A.ptr('leg_offsets'),
                                        A.ptr('work'), A.ptr('transit'), A.ptr('status'))
        assert rc == L.OK, lib.fcpp_last_error()
        A.check({k: host[k] for k in outs})
        assert np.array_equal(off_h, host['offsets'])
    for outs in FILL_SUBSETS:
        A = arena([('leg_offsets', host['leg_offsets'])])
        for k in SAMPLE_KEYS:
            if k in outs:
                A.output(k, SAMPLE_TYPES[k], host['total'])
        A.build(dev)
        rc = lib.fcpp_field_path_fill(*head(A, soff), A.ptr('leg_offsets'), host['total'], *[A.ptr(k) for k in SAMPLE_KEYS])
        assert rc == L.OK, lib.fcpp_last_error()
        A.check({k: host[k] for k in outs})
