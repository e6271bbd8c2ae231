"""The mission paths on the GPU (run with -m gpu on an MI355X): fcpp_mission_solve, _counts and _fill against the host twin
(fcpp_debug_mission_paths), EVERY value bit for bit -- the scenes of tests/test_mission_host.py plus the cases that drive the kernels' loops
round again: 130 source nodes under a wavefront's 64 lanes (a second round and a remainder of 2), 70 target nodes
under the workgroup's 4 wavefronts, more fields than a workgroup of the finish kernel has lanes, fields of one item and of none.  Then the
engine: mission_paths on tuple-form sets, and plan_polygon_fields(mission=...) on a planned holed square -- speed_plan, validate and
trajectory take the mission as it is, and its cover set covers what the separate sets cover."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import mission_cases as C

pytestmark = pytest.mark.gpu

ENDS = [(False, False), (True, True), (True, False), (False, True)]
HOLED = [[(0, 0), (30, 0), (30, 30), (0, 30)], [(12, 12), (18, 12), (18, 18), (12, 18)]]


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope='module')
def gpu():
    import torch
    ctx = E.get_context(None)
    ctx.bind_stream()
    return ctx, torch.device('cuda', ctx.device)


def dev_mission(gpu, mode, ps, items, radius, stride, spacing, entry=None, exit=None):
    """the three device entries on torch tensors -> the dict tests/mission_cases.host_mission gives (outputs pre-filled with -9 / 77)"""
    import torch
    ctx, dev = gpu
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    item_off, item_path, item_closed = items
    nf, ni = len(item_off) - 1, len(item_path)
    ns = 2 * ni + nf if nf else 0
    d = {k: up(ps[k]) for k, _ in C.COLS}
    d_off, d_ioff, d_ipath, d_closed = up(ps['offsets']), up(item_off), up(item_path), up(item_closed)
    ent = [None] * 3 if entry is None else [up(c) for c in C._cols(entry)]
    ext = [None] * 3 if exit is None else [up(c) for c in C._cols(exit)]
    out = {}
    for group, n in ((C.FIELD_OUTS, nf), (C.ITEM_OUTS, ni), (C.SLOT_OUTS, ns)):
        for k, t in group:
            out[k] = up(np.full((n, 5) if k == 'slot_seg' else n, -9, t))
    out['offsets'], out['slot_offsets'] = up(np.full(nf + 1, -9, np.int64)), up(np.full(ns + 1, -9, np.int64))
    head = (mode, nf, _ptr(d_ioff), None, ni, _ptr(d_ipath), None, _ptr(d_closed), len(ps['offsets']) - 1, _ptr(d_off), None, len(ps['x']))
    rec = [_ptr(out[k]) for k in ('status', 'item_station', 'slot_item', 'slot_word', 'slot_seg')]
    rc = ctx.lib.fcpp_mission_solve(ctx.handle, *head, *[_ptr(d[k]) for k in ('x', 'y', 'heading', 'part', 'gear')], *[_ptr(t) for t in ent],
                                    *[_ptr(t) for t in ext], float(radius), stride, *[_ptr(out[k]) for k, _ in C.SOLVE_OUTS])
    assert rc == L.OK, ctx.lib.fcpp_last_error()
    off_h = np.zeros(nf + 1, np.int64)
    rc = ctx.lib.fcpp_mission_counts(ctx.handle, *head, *rec, float(spacing), _ptr(out['offsets']), off_h.ctypes.data, _ptr(out['slot_offsets']))
    assert rc == L.OK, ctx.lib.fcpp_last_error()
    total = int(off_h[-1])
    for k, t in C.SAMPLE_OUTS:
        out['p_' + k] = up(np.full(total, 77, t))
    rc = ctx.lib.fcpp_mission_fill(ctx.handle, *head, *[_ptr(d[k]) for k, _ in C.COLS], *[_ptr(t) for t in ent], float(radius), float(spacing), *rec,
                                   _ptr(out['slot_offsets']), total, *[_ptr(out['p_' + k]) for k, _ in C.SAMPLE_OUTS])
    assert rc == L.OK, ctx.lib.fcpp_last_error()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(res['offsets'], off_h)
    return res


def same(got, want):
    for k, w in want.items():
        if k in ('rc', 'last'):
            continue
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))
        assert bad.size == 0, (k, bad.size, bad[:4] // g.dtype.itemsize)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('ends', ENDS)
def test_holed_square_equals_the_twin(gpu, mode, ends):
    ps, items, _ = C.holed_scene(mode)
    ent, ext = C.holed_ends()
    entry, exit = (ent if ends[0] else None), (ext if ends[1] else None)
    want = C.host_mission(mode, ps, items, C.SCENE_R, C.SCENE_STRIDE, C.SCENE_SPACING, entry=entry, exit=exit)
    assert want['status'][0] == 0 and want['offsets'][-1] > 0
    same(dev_mission(gpu, mode, ps, items, C.SCENE_R, C.SCENE_STRIDE, C.SCENE_SPACING, entry, exit), want)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('ends', ENDS[:2])
def test_batch_equals_the_twin(gpu, mode, ends):
    """every special case of the rule in one batch; field 1 is the loop of 130 stations against the loop of 70: a second round of the
    64-lane source loop with a remainder of 2, and 70 target nodes under 4 wavefronts; fields of 0 items and of 1"""
    ps, items, stride = C.batch_scene()
    ent, ext = C.batch_ends(len(items[0]) - 1)
    entry, exit = (ent if ends[0] else None), (ext if ends[1] else None)
    want = C.host_mission(mode, ps, items, 3.0, stride, 0.5, entry=entry, exit=exit)
    assert list(want['status']) == [0, 0, 0, L.EINVAL, 0, L.EUNSUPPORTED, 0, 0, 0, 0]
    same(dev_mission(gpu, mode, ps, items, 3.0, stride, 0.5, entry, exit), want)


def test_more_fields_than_a_finish_workgroup(gpu):
    """MISSION_BLOCK + 3 fields of two small loops and a line each: the finish kernel's second workgroup, the layers kernel's grid"""
    n = L.MISSION_BLOCK + 3
    rng = np.random.default_rng(5)
    paths, fields = [], []
    for f in range(n):
        cx, cy = 100.0 * f, 7.0 * (f % 5)
        paths += [C.circle_loop(9 + f % 7, 4.0 + f % 3, cx, cy, start=float(rng.random())), C.line(cx - 9.0, cy - 8.0, cx + 9.0, cy - 8.0, 5),
                  C.circle_loop(5 + f % 4, 6.0, cx + 1.0, cy, part=4)]
        fields.append([(3 * f, 1), (3 * f + 1, 0), (3 * f + 2, 1)][:1 + f % 3] if f % 11 else [])
    ps, items = C.path_set(paths), C.items_of(fields)
    want = C.host_mission(0, ps, items, 2.0, 1, 0.5)
    assert np.all(want['status'] == 0) and want['offsets'][-1] > 0
    same(dev_mission(gpu, 0, ps, items, 2.0, 1, 0.5), want)


def test_empty_batches(gpu):
    ps, items = C.path_set([C.line(0.0, 0.0, 1.0, 0.0, 3)]), C.items_of([])
    same(dev_mission(gpu, 0, ps, items, 2.0, 1, 0.5), C.host_mission(0, ps, items, 2.0, 1, 0.5))
    items = C.items_of([[], []])
    same(dev_mission(gpu, 1, ps, items, 2.0, 1, 0.5), C.host_mission(1, ps, items, 2.0, 1, 0.5))


# ---- through the engine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reversing', [False, True])
def test_engine_mission_paths_on_tuple_sets(gpu, reversing):
    """two tuple-form sets and the default station step: the engine's item table, planning radius and stride against the twin called with them"""
    import torch
    loops = C.path_set([C.circle_loop(130, 12.0), C.circle_loop(300, 9.0, 50.0, 0.0), C.circle_loop(70, 7.0, 1.0, 2.0, start=1.0)])
    lines = C.path_set([C.line(-20.0, -5.0, 20.0, -5.0, 41), C.line(30.0, -15.0, 70.0, -15.0, 41)])
    as_tuple = lambda ps, field, closed: (ps['offsets'], ps['x'], ps['y'], ps['heading'], ps['kappa'], ps['part'], ps['gear'], field, closed)
    ent, ext = C.batch_ends(2)
    mp = E.mission_paths([as_tuple(lines, [0, 1], False), as_tuple(loops, [0, 1, 0], True)], 3.0, 0.5, reversing=reversing, entry=ent, exit=ext)
    assert mp.stride == 3 and mp.item_offsets.tolist() == [0, 3, 5] and mp.item_path.tolist() == [0, 2, 4, 1, 3] and mp.item_set.tolist() == [0, 1, 1, 0, 1]
    ps, _ = C.pack_sets([lines, loops])
    items = (np.array([0, 3, 5], np.int64), np.array([0, 2, 4, 1, 3], np.int64), np.array([0, 1, 1, 0, 1], np.int32))
    want = C.host_mission(int(reversing), ps, items, E._chord_radius(3.0, 0.5), 3, 0.5, entry=ent, exit=ext)
    got = dict(offsets=mp.offsets, slot_offsets=mp.slot_offsets, status=mp.status, transit_length=mp.transit_length, skipped=mp.skipped,
               item_station=mp.item_station, slot_item=mp.slot_item, slot_word=mp.slot_word, slot_seg=mp.slot_seg, slot_total=mp.slot_total,
               p_x=mp.x, p_y=mp.y, p_heading=mp.heading, p_kappa=mp.kappa, p_part=mp.part, p_gear=mp.gear, p_slot=mp.slot, p_src=mp.src)
    same({k: v.cpu().numpy() for k, v in got.items()}, want)
    assert np.array_equal(mp.offsets_host, want['offsets'])
    src, src_set = mp.src.cpu().numpy(), mp.src_set.cpu().numpy()
    assert np.array_equal(src_set, np.where(src < 0, -1, (src >= len(lines['x'])).astype(np.int32)))
    x, y, field, work, pas = mp.cover_set(pass_ids=[torch.arange(len(lines['x'])), -1 - torch.arange(len(loops['x']))],
                                          work=[torch.ones(len(lines['x'])), torch.ones(len(loops['x']))])[1:]
    assert np.array_equal(work.cpu().numpy(), (src >= 0).astype(np.uint8)) and field.tolist() == [0, 1] and x is mp.x and y is mp.y
    assert np.array_equal(pas.cpu().numpy(), np.where(src < 0, 0, np.where(src < len(lines['x']), src, -1 - (src - len(lines['x'])))))


def test_plan_polygon_fields_mission(gpu):
    """the chain on a planned holed square: one path per field that the path operators take as it is, whose cover set covers what the
    separate sets cover (the rotated loops hold the same segments, joints do not work), and the options' errors"""
    import torch
    W, RES = 4.0, 0.25
    kw = dict(width=W, radius=2.0, spacing=0.5, angles=[0.0, 0.5], passes=1, headland_paths=True, coverage_resolution=RES, missed_min_area=1.0, patch=True)
    ent, ext = np.array([[-4.0, -3.0, 0.5]]), np.array([[34.0, 33.0, 1.0]])
    plan = E.plan_polygon_fields([HOLED], mission='headland_last', entry=ent, exit=ext, clear_of='boundary', **kw)
    base = E.plan_polygon_fields([HOLED], clear_of='boundary', **kw)
    m = plan.mission
    assert base.mission is None and m is not None and m.status.tolist() == [0] and m.skipped.tolist() == [0]
    hp, fp, pp = plan.headland_paths, plan.paths, plan.patch_paths
    n_rings = int(hp.offsets.numel()) - 1
    assert n_rings == 2 and int(pp.x.numel()) > 0 and m.item_set.tolist() == [0, 1, 2, 2] and m.item_closed.tolist() == [0, 0, 1, 1]
    # the field paths are built without the gates, which the mission joins: the routed order as it is, no entry or exit connector
    gated = E.plan_polygon_fields([HOLED], entry=ent, exit=ext, clear_of='boundary', **kw)
    bare = E.field_paths(plan.swaths, kw['radius'], kw['spacing'], order=plan.route)
    assert gated.mission is None and torch.equal(gated.route.order, plan.route.order) and torch.equal(fp.x.view(torch.int64), bare.x.view(torch.int64))
    assert bool((gated.paths.part >= 2).any()) and not bool((fp.part >= 2).any()) and int(fp.x.numel()) < int(gated.paths.x.numel())
    assert torch.equal(hp.x.view(torch.int64), base.headland_paths.x.view(torch.int64))
    # every source sample is driven, the loops' seams twice
    total_in = int(fp.x.numel()) + int(pp.x.numel()) + int(hp.x.numel())
    src = m.src.cpu().numpy()
    assert (src >= 0).sum() == total_in + n_rings and set(src[src >= 0].tolist()) == set(range(total_in))
    slots = m.slot_word.cpu().numpy()
    assert (slots >= 0).sum() == 5 and m.blocked is not None and 0 <= int(m.blocked[0]) <= 5
    assert abs(float(m.transit_length[0]) - float(m.slot_total[m.slot_word >= 0].sum())) <= 1e-9
    # the path operators take it as it is
    veh = E.make_vehicle()
    v = E.speed_plan(m.x, m.y, torch.full_like(m.x, 2.0), veh, offsets=m.offsets)
    v = v[0] if isinstance(v, tuple) else v
    assert v.shape == m.x.shape and bool(torch.isfinite(v).all())
    assert E.validate(m.x, m.y, v, veh, field_polygons=[HOLED[0]], offsets=m.offsets) is not None
    s = E.trajectory(m.x, m.y, v, offsets=m.offsets)[0]
    assert s.shape == m.x.shape and float(s[-1]) > float(fp.work_length[0])
    # coverage: the mission's cover set against the separate sets, round caps
    as_set = (pp.offsets, pp.x, pp.y, torch.zeros(1, dtype=torch.int64, device=pp.x.device), pp.part == 0, pp.leg + (1 << 30))
    sep = E.polygon_coverage([HOLED], W, RES, paths=(fp, hp, as_set), caps='round')
    one = E.polygon_coverage([HOLED], W, RES, paths=(m.cover_set(pass_ids=[None, pp.leg + (1 << 30), None]),), caps='round')
    print('counts (inside, covered, overlapped, spill): separate sets %s, the mission %s' % (sep.counts.tolist(), one.counts.tolist()))
    assert one.counts[:, :2].tolist() == sep.counts[:, :2].tolist()
    assert one.counts.tolist() == sep.counts.tolist()
    first = E.plan_polygon_fields([HOLED], mission='headland_first', **kw).mission
    assert first.item_set.tolist() == [0, 0, 1, 2] and first.item_closed.tolist() == [1, 1, 0, 0] and first.status.tolist() == [0]
    for bad in (dict(mission='headland_last', headland_paths=False), dict(mission='sideways')):
        with pytest.raises(ValueError):
            E.plan_polygon_fields([HOLED], **{**kw, **bad})
