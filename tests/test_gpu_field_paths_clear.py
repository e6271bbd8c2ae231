"""GPU tests of the clear field paths (run with -m gpu on an MI355X): fcpp_field_path_counts_clear / _fill_clear -- k_fpath_legs, then
k_fpath_clear_slots and k_fpath_clear_words of csrc/fcpp_solveclear.hip, then the scan, the groups and the fill as they are -- against the same
rule on the host (fcpp_debug_field_paths_clear) BIT FOR BIT on every output: the rule is one set of host+device expressions, so nothing here
is compared to a bound.  Then the list between the two passes (fcpp_ctx_field_path_clear_passes) at the wavefront and workgroup edges of the
ballot append and of the 8- and 64-lane groups, the independence of the list's order (two runs, identical bits), and the engine.

The scenes are those of tests/test_field_paths_clear_host.py.  engine.connector_clearance solves the shortest word itself, so it can say
"the shortest word is clear", which is leg_rank == 0; the clearance of the words actually DRIVEN (leg_word, leg_seg) is asked of the entry
beneath it, fcpp_conn_clear."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import test_leg_paths_pinned as PIN
from tests.support import Gpu as BaseGpu, np_of as _np
from tests.test_clearance_host import host_clear
from tests.test_field_paths_clear_host import (ALL_CLEAR, ENTRY, EXIT, FIELD_OUTS, HEAD_KEYS, REGION_DUBINS, REGION_RS, SLOT_OUTS, batch_of_65,
                                               driven_pairs, host_paths_clear, routed_order)
from tests.test_field_paths_host import SAMPLE_KEYS, SAMPLE_TYPES, host_paths, stored_order
from tests.test_route_host import HOLED_SQUARE, R, cut_with_angle, host_route, host_transit
from tests.test_solve_clear_host import U_WALL
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu

SPACING = 0.5
NAN_OK = ('work', 'transit')          # NaN for a failed field: equal as NaN, whatever the payload
HEAD_TYPES = dict(offsets=np.int64, leg_offsets=np.int64, work=np.float64, transit=np.float64, status=np.int32)


class Gpu(BaseGpu):
    def up(self, a):
        return None if a is None else self.torch.as_tensor(np.array(a), device=self.dev)          # (a copy: broadcast inputs are read-only)

    def passes(self):
        import ctypes as C
        listed, launches = C.c_int64(-1), C.c_int64(-1)
        assert self.lib.fcpp_ctx_field_path_clear_passes(self.h, C.byref(listed), C.byref(launches)) == 0
        return listed.value, launches.value


@pytest.fixture
def gpu():
    g = Gpu()
    g.ctx.bind_stream()
    return g


def device_paths_clear(g, cut, regions, radius=R, spacing=SPACING, mode=0, order=None, entry=None, exit=None):
    """fcpp_field_path_counts_clear, then fcpp_field_path_fill_clear with the counts call's leg_offsets -> dict like host_paths_clear's, and
    the (listed, word_launches) of the context after each of the two calls"""
    torch = g.torch
    soff = cut['offsets']
    n, nt = len(soff) - 1, int(soff[-1])
    n_slots = 2 * nt + n
    ro, vo, rx, ry = pack(regions)
    keep = [g.up(a) for a in (soff, cut['ax'], cut['ay'], cut['bx'], cut['by'], cut['length'], cut['angle'])]
    keep.append(g.up(None if order is None else np.ascontiguousarray(order, dtype=np.int32)))
    for pose in (entry, exit):
        p = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(-1, 3)
        keep += [g.up(None if p is None else p[:, k]) for k in range(3)]
    reg = [g.up(a) for a in (ro, vo, rx, ry)]
    ptr = E._ptr
    head = (g.h, n, ptr(keep[0]), E._host_ptr(soff), nt, *[ptr(t) for t in keep[1:8]], float(radius), mode, float(spacing), *[ptr(t) for t in keep[8:]],
            ptr(reg[0]), len(vo) - 1, ptr(reg[1]), len(rx), ptr(reg[2]), ptr(reg[3]))
    out = {k: torch.full((n + 1 if k == 'offsets' else n_slots + 1 if k == 'leg_offsets' else n,), -7, dtype=getattr(torch, np.dtype(t).name), device=g.dev)
           for k, t in HEAD_TYPES.items()}
    for k, t, shape in SLOT_OUTS:
        out[k] = torch.full((n_slots,) + shape, -7, dtype=getattr(torch, np.dtype(t).name), device=g.dev)
    for k, t in FIELD_OUTS:
        out[k] = torch.full((n,), -7, dtype=torch.int32, device=g.dev)
    off_h = np.full(n + 1, -1, np.int64)
    rc = g.lib.fcpp_field_path_counts_clear(*head, ptr(out['offsets']), E._host_ptr(off_h), *[ptr(out[k]) for k in HEAD_KEYS[1:]],
                                            *[ptr(out[k]) for k, _, _ in SLOT_OUTS], *[ptr(out[k]) for k, _ in FIELD_OUTS])
    assert rc == L.OK, g.lib.fcpp_last_error()
    after_counts = g.passes()
    total = int(off_h[-1])
    for k in SAMPLE_KEYS:
        out[k] = torch.full((total,), 77, dtype=getattr(torch, np.dtype(SAMPLE_TYPES[k]).name), device=g.dev)
    rc = g.lib.fcpp_field_path_fill_clear(*head, ptr(out['leg_offsets']), total, *[ptr(out[k]) for k in SAMPLE_KEYS])
    assert rc == L.OK, g.lib.fcpp_last_error()
    res = {k: _np(v) for k, v in out.items()}
    assert np.array_equal(off_h, res['offsets'])
    res['total'] = total
    return res, after_counts, g.passes()


def assert_same(dev, host):
    for k in HEAD_KEYS + tuple(k for k, _, _ in SLOT_OUTS) + tuple(k for k, _ in FIELD_OUTS) + SAMPLE_KEYS:
        a, b = np.ascontiguousarray(dev[k]), np.ascontiguousarray(host[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if k in NAN_OK:
            assert np.array_equal(a, b, equal_nan=True), k
            a, b = a[~np.isnan(b)], b[~np.isnan(b)]
        assert np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)), (k, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])


def batch_order(cut, mode):
    """a routed order for a whole batch: fcpp_debug_route on the transit blocks alone, two candidates, three sweeps"""
    T, toff = host_transit(cut, R, mode)
    route = host_route(cut['offsets'], T, toff, None, None, S=2, max_sweeps=3)
    assert not np.array_equal(route['route'], stored_order(cut['offsets']))
    return route['route'].copy()


def scene(n, mode, routed, ends):
    """-> cut, regions, order, entry, exit.  n = 1: the recorded scene of the mode; n = 65: batch_of_65 -- every scene in turn, all-clear
    regions, regions with a NaN vertex -- with field 7 given a bad order (a swath named twice)"""
    if n == 1:
        cut = cut_with_angle([HOLED_SQUARE], 0.0, 4.0)
        order = routed_order(cut, 0, False) if routed else None
        return cut, [REGION_RS if mode else REGION_DUBINS], order, ENTRY[None] if ends else None, EXIT[None] if ends else None
    cut, regions, order, entry, exit = batch_of_65()
    if routed:
        order = batch_order(cut, mode)
    s = int(cut['offsets'][7])
    assert cut['offsets'][8] - s >= 2
    order[s + 1] = order[s] ^ 1
    return cut, regions, order, entry if ends else None, exit if ends else None


# ---- 1. and 3.: device equals host, the fill takes the counts call's offsets, a second run gives identical bits --------------------------
@pytest.mark.parametrize('ends', [False, True], ids=['open', 'ends'])
@pytest.mark.parametrize('routed', [False, True], ids=['stored', 'routed'])
@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
@pytest.mark.parametrize('n', [1, 65])
def test_device_equals_host_bit_for_bit(gpu, n, mode, routed, ends):
    cut, regions, order, entry, exit = scene(n, mode, routed, ends)
    host = host_paths_clear(cut, regions, mode=mode, order=order, entry=entry, exit=exit)
    dev, after_counts, after_fill = device_paths_clear(gpu, cut, regions, mode=mode, order=order, entry=entry, exit=exit)
    assert_same(dev, host)
    assert host['total'] > 100 and (host['leg_rank'] < 0).any()
    if n == 65:
        assert host['status'][7] == L.EINVAL and np.count_nonzero(host['status']) == 1 and L.EINVAL in host['region_status'].tolist()
        assert (host['leg_rank'] > 0).any() and (host['leg_rank'] == 0).any()
    # the fill has no status to go by: it also looks at the legs of the field that failed
    want = shortest_words_listed(cut, regions, mode, order, entry, exit)
    assert after_counts[0] == want > 0 and after_fill[0] >= want and after_fill[1] == after_counts[1] + 1
    again, _, _ = device_paths_clear(gpu, cut, regions, mode=mode, order=order, entry=entry, exit=exit)
    assert_same(again, dev)          # (no output depends on the list's order)


# ---- 2. the list between the passes ----------------------------------------------------------------------------------------------------------
def test_an_all_clear_batch_lists_nothing_and_skips_the_second_pass(gpu):
    cut = cut_with_angle([HOLED_SQUARE] * 5, 0.0, 4.0)
    entry, exit = np.tile(ENTRY, (5, 1)), np.tile(EXIT, (5, 1))
    before = gpu.passes()[1]
    for mode in (0, 1):
        dev, after_counts, after_fill = device_paths_clear(gpu, cut, [ALL_CLEAR] * 5, mode=mode, entry=entry, exit=exit)
        assert after_counts == (0, before) and after_fill == (0, before)
        assert_same(dev, host_paths_clear(cut, [ALL_CLEAR] * 5, mode=mode, entry=entry, exit=exit))
        assert not dev['leg_rank'].any() and not dev['blocked'].any() and not dev['reshaped'].any()


def shortest_words_listed(cut, regions, mode, order, entry, exit):
    """the connector legs whose shortest word starts inside its (valid) region and crosses it, by the host twins of the EXISTING entries"""
    plain = host_paths(cut, R, SPACING, mode, order=order, entry=entry, exit=exit)
    soff = cut['offsets']
    explicit = stored_order(soff) if order is None else order
    listed = 0
    for i in range(len(soff) - 1):
        slots, frm, _ = driven_pairs(cut, i, explicit, entry, exit)
        if not slots or plain['status'][i] != 0:
            continue
        p = np.asarray(slots) + int(2 * soff[i] + i)
        c = host_clear(mode, frm, R, plain['leg_word'][p], np.ascontiguousarray(plain['leg_seg'][p][:, :5 if mode else 3]), i, regions)
        listed += int(np.count_nonzero((c['inside'] == 1) & (c['crossings'] > 0) & (c['field_status'][i] == 0)))
    return listed


@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
def test_65_copies_list_the_legs_that_start_inside_and_cross(gpu, mode):
    cut = cut_with_angle([HOLED_SQUARE] * 65, 0.0, 4.0)
    regions = [REGION_DUBINS] * 65
    entry, exit = np.tile(ENTRY, (65, 1)), np.tile(EXIT, (65, 1))
    want = shortest_words_listed(cut, regions, mode, None, entry, exit)
    assert want > 0 and want % 65 == 0
    before = gpu.passes()[1]
    dev, after_counts, after_fill = device_paths_clear(gpu, cut, regions, mode=mode, entry=entry, exit=exit)
    assert after_counts == (want, before + 1) and after_fill == (want, before + 2)
    assert_same(dev, host_paths_clear(cut, regions, mode=mode, entry=entry, exit=exit))


def one_listed_batch(at):
    """a batch whose ONE listed slot is connector slot `at`: one-swath strips inside an all-clear region as padding (two connector slots
    each, both without a leg: no entry / exit), a field without swaths (one slot) where `at` is even, then the U-turn of
    tests/test_solve_clear_host.py beside its wall: swath 0 north along x = 0, swath 1 south along x = 6, the connector in its slot 2"""
    k, odd = divmod(at - 1, 2)
    m = [1] * k + [0] * odd + [2]
    n = len(m)
    soff = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    nt = int(soff[-1])
    a, b = np.zeros((nt, 2)), np.zeros((nt, 2))
    a[:k], b[:k] = (0.0, 1.6), (30.0, 1.6)
    a[k:], b[k:] = [(0.0, -20.0), (6.0, -20.0)], [(0.0, 0.0), (6.0, 3.0)]
    cut = dict(offsets=soff, a=a, b=b, ax=a[:, 0].copy(), ay=a[:, 1].copy(), bx=b[:, 0].copy(), by=b[:, 1].copy(),
               length=np.hypot(*(b - a).T), angle=np.array([0.0] * (n - 1) + [np.pi / 2]))
    regions = [ALL_CLEAR] * (n - 1) + [U_WALL]
    assert int(soff[-2] + (n - 1)) + 1 == at          # the last field's first connector slot, and one on
    return cut, regions


@pytest.mark.parametrize('at', [63, 64, 255, 256])
@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
def test_one_listed_slot_at_the_wavefront_and_workgroup_edges(gpu, mode, at):
    cut, regions = one_listed_batch(at)
    host = host_paths_clear(cut, regions, mode=mode)
    n_slots = len(host['leg_rank'])
    assert np.flatnonzero(host['leg_rank']).tolist() == [n_slots - 3] and host['leg_rank'][n_slots - 3] >= 1
    assert shortest_words_listed(cut, regions, mode, None, None, None) == 1
    before = gpu.passes()[1]
    dev, after_counts, after_fill = device_paths_clear(gpu, cut, regions, mode=mode)
    assert after_counts == (1, before + 1) and after_fill == (1, before + 2)
    assert_same(dev, host)


# ---- 4. the engine ---------------------------------------------------------------------------------------------------------------------------
def swath_set(gpu, cut):
    t = {k: gpu.up(np.array(cut[k])) for k in ('offsets', 'a', 'b', 'length', 'angle')}
    return E.SwathSet(t['offsets'], cut['offsets'], t['a'], t['b'], None, t['length'], None, None, t['angle'])


@pytest.mark.parametrize('mode', [0, 1], ids=['dubins', 'rs'])
def test_engine_field_paths_clear_of(gpu, mode):
    torch = gpu.torch
    cut, regions, order, entry, exit = batch_of_65()
    ss = swath_set(gpu, cut)
    fp = E.field_paths(ss, R, SPACING, reversing=bool(mode), order=order, entry=entry, exit=exit, clear_of=regions)
    radius = E._chord_radius(R, SPACING)
    host = host_paths_clear(cut, regions, radius=radius, mode=mode, order=order, entry=entry, exit=exit)
    names = dict(offsets='offsets', leg_offsets='leg_offsets', work='work_length', transit='transit_length', status='status')
    got = {k: _np(getattr(fp, names.get(k, k))) for k in HEAD_KEYS + tuple(k for k, _, _ in SLOT_OUTS) + tuple(k for k, _ in FIELD_OUTS) + SAMPLE_KEYS}
    assert_same(got, host)
    assert np.array_equal(fp.offsets_host, host['offsets']) and (host['leg_rank'] > 0).any() and (host['leg_rank'] < 0).any()
    # the driven words by the existing clearance entry, and the shortest words by connector_clearance
    soff = cut['offsets']
    slots, frm, to, pf = [], [], [], []
    for i in range(65):
        s, f, t = driven_pairs(cut, i, order, entry, exit)
        slots += [int(2 * soff[i] + i) + j for j in s]
        frm.append(f)
        to.append(t)
        pf += [i] * len(s)
    slots, frm, to, pf = np.asarray(slots), np.concatenate(frm), np.concatenate(to), np.asarray(pf, dtype=np.int64)
    rank = host['leg_rank'][slots]
    ns = 5 if mode else 3
    region = E.polygon_fields(regions)
    f = [gpu.up(frm[:, k]) for k in range(3)]
    word, seg, pfd = fp.leg_word[gpu.up(slots)].contiguous(), fp.leg_seg[gpu.up(slots)][:, :ns].contiguous(), gpu.up(pf)
    crossings = torch.empty(len(slots), dtype=torch.int32, device=gpu.dev)
    inside = torch.empty(len(slots), dtype=torch.int8, device=gpu.dev)
    gpu.ctx.bind_stream()
    L.check(gpu.lib.fcpp_conn_clear(gpu.h, mode, len(slots), E._ptr(f[0]), E._ptr(f[1]), E._ptr(f[2]), radius, E._ptr(word), E._ptr(seg), E._ptr(pfd),
                                    *region._head(), E._ptr(crossings), E._ptr(inside), None, None))
    clear = (_np(inside) == 1) & (_np(crossings) == 0)
    assert np.array_equal(clear, rank >= 0)
    assert np.array_equal(np.bincount(pf[~clear], minlength=65), host['blocked'])
    shortest = E.connector_clearance(frm, to, regions, pf, radius, reversing=bool(mode))
    assert np.array_equal(_np(shortest.clear), rank == 0)
    # the path operators take the result as it is
    kap = E.curvature(fp.x, fp.y, offsets=fp.offsets)
    veh = E.make_vehicle()
    v = torch.full_like(fp.x, 2.0)
    vout, _ = E.speed_plan(fp.x, fp.y, v, veh, clamp=True, offsets=fp.offsets)
    flags, _ = E.validate(fp.x, fp.y, v, veh, offsets=fp.offsets)
    traj = E.trajectory(fp.x, fp.y, vout, offsets=fp.offsets)
    assert kap.shape == fp.x.shape == vout.shape == flags.shape and traj is not None


def test_engine_field_paths_without_clear_of_calls_the_old_entries(gpu, monkeypatch):
    def refuse(*a):
        raise AssertionError('a clear entry was called without clear_of')
    monkeypatch.setattr(gpu.lib, 'fcpp_field_path_counts_clear', refuse)
    monkeypatch.setattr(gpu.lib, 'fcpp_field_path_fill_clear', refuse)
    name = PIN.FIELD_NAMES[2]
    cut, kw = PIN.field_cases()[name]
    t = {k: gpu.up(np.array(cut[k])) for k in ('offsets', 'a', 'b', 'line', 'length', 'angle')}
    ss = E.SwathSet(t['offsets'], cut['offsets'], t['a'], t['b'], t['line'], t['length'], None, None, t['angle'])
    fp = E.field_paths(ss, R, kw['spacing'], reversing=bool(kw['mode']), order=kw['order'], entry=kw['entry'], exit=kw['exit'])
    names = dict(offsets='offsets', leg_offsets='leg_offsets', work='work_length', transit='transit_length', status='status')
    got = {k: _np(getattr(fp, names[k])) for k in PIN.FIELD_FULL}
    got.update({k: _np(getattr(fp, k)) for k in SAMPLE_KEYS})
    PIN.assert_pinned(name, got, PIN.FIELD_FULL, PIN.DIGESTS)
    assert fp.leg_rank is None and fp.blocked is None and fp.region_status is None


def test_plan_polygon_fields_reshape(gpu):
    """The holed square with one headland pass, region = its surveyed boundary.  Width 2 m, radius 3 m, reversing: at the width 4 and radius 6
    of the other tests a Dubins turn between neighbouring swaths cannot stay inside a headland of one pass whatever word is driven (the
    host twin finds nothing to rescue in either order), so the scene is one where the boundary leaves room for another word."""
    width, radius_, mode = 2.0, 3.0, 1
    angles = [0.0]
    with pytest.raises(ValueError):
        E.plan_polygon_fields([HOLED_SQUARE], width, radius_, SPACING, angles, reshape=True)
    kw = dict(passes=1, reversing=True, entry=ENTRY[None], exit=EXIT[None], clear_of='boundary')
    plan = E.plan_polygon_fields([HOLED_SQUARE], width, radius_, SPACING, angles, reshape=True, **kw)
    plain = E.plan_polygon_fields([HOLED_SQUARE], width, radius_, SPACING, angles, **kw)
    fp = plan.paths
    assert np.array_equal(_np(plan.route.order), _np(plain.route.order)) and plain.paths.leg_rank is None
    # the host twin on the same swaths, order and region decides what there is to see
    ss = plan.swaths
    a, b = _np(ss.a), _np(ss.b)
    cut = dict(offsets=np.asarray(ss.offsets_host, dtype=np.int64), a=a, b=b, ax=a[:, 0].copy(), ay=a[:, 1].copy(), bx=b[:, 0].copy(), by=b[:, 1].copy(),
               length=_np(ss.length), angle=_np(ss.angle))
    order = _np(plan.route.order)
    radius = E._chord_radius(radius_, SPACING)
    host = host_paths_clear(cut, [HOLED_SQUARE], radius=radius, mode=mode, order=order, entry=ENTRY[None], exit=EXIT[None])
    stored = host_paths_clear(cut, [HOLED_SQUARE], radius=radius, mode=mode, entry=ENTRY[None], exit=EXIT[None])
    print('holed square, one headland pass, region = the boundary: planned order reshaped %d blocked %d; stored order reshaped %d blocked %d'
          % (host['reshaped'][0], host['blocked'][0], stored['reshaped'][0], stored['blocked'][0]))
    assert np.array_equal(_np(fp.reshaped), host['reshaped']) and np.array_equal(_np(fp.blocked), host['blocked'])
    assert np.array_equal(_np(fp.leg_rank), host['leg_rank']) and np.array_equal(_np(fp.x).view(np.uint64), host['x'].view(np.uint64))
    if host['reshaped'].sum() == 0:
        # the planned order leaves nothing to rescue here: the stored order does, through the same entries
        assert stored['reshaped'].sum() > 0
        fp = E.field_paths(ss, radius_, SPACING, reversing=True, entry=ENTRY[None], exit=EXIT[None], clear_of=[HOLED_SQUARE])
        assert np.array_equal(_np(fp.reshaped), stored['reshaped']) and np.array_equal(_np(fp.blocked), stored['blocked'])
        order, host = stored_order(cut['offsets']), stored
    assert _np(fp.reshaped).sum() > 0
    # blocked: a recount of the driven words by the existing clearance entry
    slots, frm, _ = driven_pairs(cut, 0, order, ENTRY[None], EXIT[None])
    c = host_clear(mode, frm, radius, _np(fp.leg_word)[slots], np.ascontiguousarray(_np(fp.leg_seg)[slots][:, :5]), 0, [HOLED_SQUARE])
    assert np.count_nonzero(~c['clear']) == int(_np(fp.blocked)[0])
    # the clearance report stays the shortest-word legs as routed
    assert np.array_equal(_np(plan.clearance.clear), _np(plain.clearance.clear))
