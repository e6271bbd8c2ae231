"""The loop transits on the device (run with -m gpu on an MI355X): fcpp_loop_transit_solve / _counts / _fill against their host twin
fcpp_debug_loop_transits, bit for bit -- the scene of tests/test_loop_transit_host.py in both modes, a mixed batch (a valid field, a field
without loops, a bad region), station counts around the kernels' workgroup and tile size (second rounds of every lane-, wave-, block- and
tile-strided loop), a region of FCPP_CLEAR_EDGE_CHUNK + 1 edges, the call that lists nothing (no second launch), and the splice
engine.field_paths(loops=...) does, whose CSR curvature, speed_plan, validate and trajectory take as it is."""
import ctypes

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import loop_transit_cases as C
from tests.test_field_paths_clear_host import host_paths_clear
from tests.test_field_paths_host import SAMPLE_KEYS
from tests.test_loop_transit_host import OPEN, straight_loop
from tests.test_route_host import HOLED_SQUARE, cut_with_angle
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu

F64_OUTS = ('in_seg', 'in_len', 'out_seg', 'out_len', 'ride', 'total')


def _t(a, dev):
    import torch
    return torch.as_tensor(np.array(a), device=dev)


def passes(ctx):
    listed, launches = ctypes.c_int64(-1), ctypes.c_int64(-1)
    L.check(ctx.lib.fcpp_ctx_loop_transit_passes(ctx.handle, ctypes.byref(listed), ctypes.byref(launches)))
    return listed.value, launches.value


def dev_transits(mode, frm, to, radius, pair_field, fields, ls, stride, spacing=0.5):
    """the three device entries on plain tensors -> dict like host_transits'"""
    import torch
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    ctx.bind_stream()
    P = E._ptr
    frm, to = np.asarray(frm, dtype=np.float64).reshape(-1, 3), np.asarray(to, dtype=np.float64).reshape(-1, 3)
    n = len(frm)
    f, t = [_t(c, dev) for c in frm.T], [_t(c, dev) for c in to.T]
    pf = _t(np.broadcast_to(np.asarray(pair_field, dtype=np.int64), (n,)), dev)
    ro, vo, rx, ry = pack(fields)
    region = [_t(a, dev) for a in (ro, vo, rx, ry)]
    lt = {k: _t(ls[k], dev) for k in ('off', 'x', 'y', 'heading', 'kappa', 's', 'part', 'gear', 'field_loops')}
    out = {k: torch.full((n, C.NSEG[mode]) if k.endswith('seg') else (n,), -9, dtype=getattr(torch, np.dtype(tp).name), device=dev) for k, tp in C.SOLVE_OUTS}
    n_loops, n_samples = len(ls['off']) - 1, len(ls['x'])
    L.check(ctx.lib.fcpp_loop_transit_solve(ctx.handle, mode, n, *[P(c) for c in f], *[P(c) for c in t], float(radius), P(pf), len(ro) - 1, P(region[0]),
                                            len(vo) - 1, P(region[1]), len(rx), P(region[2]), P(region[3]), n_loops, P(lt['off']), None, n_samples,
                                            P(lt['x']), P(lt['y']), P(lt['heading']), P(lt['s']), P(lt['part']), P(lt['gear']), P(lt['field_loops']), None,
                                            int(stride), *[P(out[k]) for k, _ in C.SOLVE_OUTS]))
    off = torch.full((n + 1,), -9, dtype=torch.int64, device=dev)
    rec = [P(out[k]) for k in ('found', 'loop', 'st_i', 'st_j', 'in_word', 'in_seg', 'out_word', 'out_seg')]
    L.check(ctx.lib.fcpp_loop_transit_counts(ctx.handle, mode, n, *rec, n_loops, P(lt['off']), None, n_samples, float(spacing), P(off), None))
    total = int(off[-1])
    samples = {k: torch.full((total,), 77, dtype=getattr(torch, np.dtype(tp).name), device=dev) for k, tp in C.PATH_OUTS}
    L.check(ctx.lib.fcpp_loop_transit_fill(ctx.handle, mode, n, *[P(c) for c in f], float(radius), *rec, n_loops, P(lt['off']), None, n_samples,
                                           P(lt['x']), P(lt['y']), P(lt['heading']), P(lt['kappa']), P(lt['gear']), float(spacing), P(off), None, total,
                                           *[P(samples[k]) for k, _ in C.PATH_OUTS]))
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['offsets'] = off.cpu().numpy()
    res.update({'p_' + k: v.cpu().numpy() for k, v in samples.items()})
    return res


def same(got, want):
    for k, _ in C.SOLVE_OUTS:
        a, b = got[k], want[k]
        if k in F64_OUTS:
            eq = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
            assert np.all(eq), (k, np.flatnonzero(~eq.reshape(len(a), -1).all(axis=1))[:8])
        else:
            assert np.array_equal(a, b), (k, np.flatnonzero(a != b)[:8], a[:8], b[:8])
    assert np.array_equal(got['offsets'], want['offsets'])
    for k, _ in C.PATH_OUTS:
        assert np.array_equal(got['p_' + k].view(np.uint8), want['p_' + k].view(np.uint8)), k


def both(mode, frm, to, radius, pf, fields, ls, stride):
    want = C.host_transits(mode, frm, to, radius, pf, fields, ls, stride)
    got = dev_transits(mode, frm, to, radius, pf, fields, ls, stride)
    same(got, want)
    return got


@pytest.mark.parametrize('mode', [0, 1])
def test_scene(mode):
    sc = C.scene(mode)
    b = sc['blocked']
    got = both(mode, sc['frm'][b], sc['to'][b], C.SCENE_R, 0, sc['region'], sc['ls'], C.SCENE_STRIDE)
    assert got['found'].sum() >= 1


@pytest.mark.parametrize('mode', [0, 1])
def test_mixed_batch(mode):
    loop = straight_loop()
    fields = [HOLED_SQUARE] + OPEN + [[[(0, 0), (9, 0), (np.nan, 9)]]] + OPEN
    pond = C.ring_loops(C.pond_ring(C.SCENE_RING), C.SCENE_R, mode, C.SCENE_SPACING)
    ls = C.pack_loops(pond + [(2, loop), (3, loop)], 4)
    sc = C.scene(mode)
    b = sc['blocked'][:3]
    frm = np.concatenate([sc['frm'][b], [(-5.0, 0.0, 0.0)] * 3, [(np.nan, 0.0, 0.0)]])
    to = np.concatenate([sc['to'][b], [(14.0, 0.0, 0.0)] * 4])
    pf = np.array([0] * len(b) + [1, 2, 3, 3])
    got = both(mode, frm, to, C.SCENE_R, pf, fields, ls, 3)
    assert list(got['status'][len(b):]) == [0, L.EINVAL, 0, L.EINVAL] and list(got['found'][len(b):]) == [0, 0, 1, 0]


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('stations', [L.TRANSIT_BLOCK - 1, L.TRANSIT_BLOCK, L.TRANSIT_BLOCK + 1, 2 * L.TRANSIT_BLOCK + 1])
def test_second_rounds(mode, stations):
    """one field whose station count sits at the workgroup / tile size: the wavefront's 64-sample steps of the stations kernel, the slots
    per side of the stations pass, the pick pass's tiles and its threads' strided in-stations all go into a second (third) round; the pond
    makes the first launch list items, so the word kernel's groups do too"""
    fields, ls, frm, to = C.second_round_case(mode, stations)
    ctx = E.get_context(None)
    before = passes(ctx)[1]
    got = both(mode, frm, to, 1.5, 0, fields, ls, 1)
    listed, launches = passes(ctx)
    assert got['found'].sum() >= 1 and listed > L.TRANSIT_BLOCK and launches == before + 1


def test_region_of_one_edge_more_than_a_chunk():
    fields, ls, frm, to = C.chunk_plus_one_case()
    for mode in (0, 1):
        got = both(mode, frm, to, 1.5, 0, fields, ls, 1)
        assert got['found'].sum() >= 1


def test_more_pairs_than_a_workgroup():
    """the scan of the pairs' sample counts walks the pairs a workgroup at a time; the per-pair kernels' grids get a second workgroup"""
    fields, ls, frm, to = C.many_pairs_case()
    got = both(0, frm, to, 1.5, 0, fields, ls, 1)
    assert len(got['found']) > L.TRANSIT_BLOCK and got['found'].sum() > L.TRANSIT_BLOCK


def test_nothing_listed_launches_no_second_pass():
    ls = C.pack_loops([(0, straight_loop())], 1)
    frm, to = [(-5.0, 0.0, 0.0), (4.0, -4.0, np.pi / 2)], [(14.0, 0.0, 0.0), (4.0, 14.0, np.pi / 2)]
    ctx = E.get_context(None)
    before = passes(ctx)[1]
    for mode in (0, 1):
        got = both(mode, frm, to, 1.0, 0, OPEN, ls, 2)
        assert np.all(got['found'] == 1)
        assert passes(ctx) == (0, before)


# ---- through the engine ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def engine_scene():
    work = E.polygon_inset([HOLED_SQUARE], [C.SCENE_INSET]).as_fields(0)
    ss = E.polygon_swaths(work, 0.0, C.SCENE_W)
    ring = E.polygon_inset([HOLED_SQUARE], [C.SCENE_RING])
    loops = tuple(E.headland_paths(ring, C.SCENE_R, C.SCENE_SPACING, direction=d) for d in (1, -1))
    plain = E.field_paths(ss, C.SCENE_R, C.SCENE_SPACING, clear_of=[HOLED_SQUARE])
    det = E.field_paths(ss, C.SCENE_R, C.SCENE_SPACING, clear_of=[HOLED_SQUARE], loops=loops)
    return ss, loops, plain, det


def test_field_paths_without_loops_are_unchanged(engine_scene):
    ss, _, plain, _ = engine_scene
    assert plain.detoured is None and plain.leg_transit is None and plain.transits is None
    cut = cut_with_angle([C.HostInset([HOLED_SQUARE], [C.SCENE_INSET]).rings(0, 0)], 0.0, C.SCENE_W)
    want = host_paths_clear(cut, [HOLED_SQUARE], radius=E._chord_radius(C.SCENE_R, C.SCENE_SPACING), spacing=C.SCENE_SPACING, mode=0)
    assert np.array_equal(plain.offsets_host, want['offsets']) and np.array_equal(plain.leg_offsets.cpu().numpy(), want['leg_offsets'])
    for k in SAMPLE_KEYS:
        assert np.array_equal(getattr(plain, k).cpu().numpy().view(np.uint8), want[k].view(np.uint8)), k
    assert np.array_equal(plain.blocked.cpu().numpy(), want['blocked']) and np.array_equal(plain.leg_rank.cpu().numpy(), want['leg_rank'])


def test_field_paths_with_loops_splice_the_transits(engine_scene):
    import torch
    ss, loops, plain, det = engine_scene
    lt = det.transits
    detoured, blocked0 = int(det.detoured[0]), int(plain.blocked[0])
    assert blocked0 >= 1 and detoured >= 1 and int(det.blocked[0]) == blocked0 - detoured == int((lt.found == 0).sum())
    # the transits are the twin's, on the loop set the engine arranged and the pairs of the rank -1 legs
    R = E._chord_radius(C.SCENE_R, C.SCENE_SPACING)
    frm, to, lf, slot = E._leg_pairs(ss, None, None, None)
    g = (2 * ss.offsets[lf] + lf + slot).cpu().numpy()
    rank = plain.leg_rank.cpu().numpy()
    sel = np.flatnonzero(rank[g] < 0)
    ls = {k: lt.loop_set[k].cpu().numpy() for k in C.LOOP_KEYS}
    ls.update(off=lt.loop_set['offsets_host'], field_loops=lt.loop_set['field_loops_host'])
    want = C.host_transits(0, frm.cpu().numpy()[sel], to.cpu().numpy()[sel], R, 0, [HOLED_SQUARE], ls, lt.stride, spacing=C.SCENE_SPACING)
    got = dict(found=lt.found, loop=lt.loop, st_i=lt.st_i, st_j=lt.st_j, in_word=lt.in_word, in_seg=lt.in_seg, in_len=lt.in_length, in_rank=lt.in_rank,
               out_word=lt.out_word, out_seg=lt.out_seg, out_len=lt.out_length, out_rank=lt.out_rank, ride=lt.ride, total=lt.total, status=lt.status)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    tp = lt.paths(C.SCENE_SPACING)
    got['offsets'] = tp.offsets_host
    got.update({'p_' + k: getattr(tp, k).cpu().numpy() for k, _ in C.PATH_OUTS})
    same(got, want)
    # the splice: a detoured slot holds its transit's samples, every other slot the plain path's
    leg_transit = det.leg_transit.cpu().numpy()
    assert np.array_equal(np.flatnonzero(leg_transit >= 0), g[sel][want['found'] == 1])
    lo0, lo1 = plain.leg_offsets.cpu().numpy(), det.leg_offsets.cpu().numpy()
    assert lo1[-1] == det.x.numel() == det.offsets_host[-1] and det.offsets_host[0] == 0
    for p in range(len(leg_transit)):
        tr = leg_transit[p]
        for k, _ in C.PATH_OUTS:
            new = getattr(det, k)[lo1[p]:lo1[p + 1]].cpu().numpy()
            old = want['p_' + k][want['offsets'][tr]:want['offsets'][tr + 1]] if tr >= 0 else getattr(plain, k)[lo0[p]:lo0[p + 1]].cpu().numpy()
            assert np.array_equal(new.view(np.uint8), old.view(np.uint8)), (k, p)
        assert np.all(det.leg[lo1[p]:lo1[p + 1]].cpu().numpy() == p)          # (one field: the slot is the global slot)
    assert (det.part == L.PART_LOOP_RIDE).any()
    old_len = plain.leg_total.cpu().numpy()
    new_len = old_len.copy()
    new_len[g[sel][want['found'] == 1]] = want['total'][want['found'] == 1]
    assert abs(float(det.transit_length[0]) - new_len[0::2].sum()) < 1e-9 * new_len.sum()
    # the spliced CSR goes to the path operators as it is
    veh = E.make_vehicle()
    v = torch.full_like(det.x, 2.0)
    kap = E.curvature(det.x, det.y, offsets=det.offsets)
    sp, _ = E.speed_plan(det.x, det.y, v, veh, offsets=det.offsets)
    s, t, h, totals = E.trajectory(det.x, det.y, sp, offsets=det.offsets)
    val = E.validate(det.x, det.y, sp, veh, offsets=det.offsets)
    assert kap.numel() == sp.numel() == s.numel() == det.x.numel() and bool(torch.isfinite(kap).all()) and bool(torch.isfinite(s).all())
    assert bool((s[1:] >= s[:-1]).all()) and totals.shape[0] == 1 and val is not None


def test_engine_loop_transits_is_what_field_paths_uses(engine_scene):
    import torch
    ss, loops, plain, det = engine_scene
    R = E._chord_radius(C.SCENE_R, C.SCENE_SPACING)
    frm, to, lf, slot = E._leg_pairs(ss, None, None, None)
    sel = torch.nonzero(plain.leg_rank[2 * ss.offsets[lf] + lf + slot] < 0).reshape(-1)
    lt = E.loop_transits(frm[sel], to[sel], [HOLED_SQUARE], 0, loops, R)          # (station_step: the radius, as field_paths takes it)
    ref = det.transits
    assert lt.stride == ref.stride == max(1, round(R / C.SCENE_SPACING)) and lt.radius == ref.radius
    for k in ('found', 'loop', 'st_i', 'st_j', 'in_word', 'out_word', 'in_rank', 'out_rank', 'status'):
        assert torch.equal(getattr(lt, k), getattr(ref, k)), k
    for k in ('in_seg', 'out_seg', 'in_length', 'out_length', 'ride', 'total'):
        assert torch.equal(getattr(lt, k).view(torch.int64), getattr(ref, k).view(torch.int64)), k
    tp = lt.paths(C.SCENE_SPACING)
    assert int(tp.offsets_host[-1]) == tp.x.numel() > 0 and set(tp.part.unique().tolist()) <= {1, L.PART_LOOP_RIDE}
    wide = E.loop_transits(frm[sel], to[sel], [HOLED_SQUARE], 0, loops[0], R, station_step=4 * R)
    assert wide.stride == max(1, round(4 * R / C.SCENE_SPACING)) and bool((wide.total >= lt.total).all())
    with pytest.raises(ValueError):
        E.loop_transits(frm[sel], to[sel][:1], [HOLED_SQUARE], 0, loops, R)


def test_plan_polygon_fields_detours():
    plan = E.plan_polygon_fields([HOLED_SQUARE], 4.0, 1.5, 0.5, [0.0], clear_of='boundary', reshape=True, headland_paths=True, detour=True)
    base = E.plan_polygon_fields([HOLED_SQUARE], 4.0, 1.5, 0.5, [0.0], clear_of='boundary', reshape=True, headland_paths=True)
    assert base.transits is None and base.paths.detoured is None
    assert plan.transits is plan.paths.transits
    assert np.array_equal((base.paths.blocked - plan.paths.detoured).cpu().numpy(), plan.paths.blocked.cpu().numpy())
    assert int(plan.transits.found.sum()) == int(plan.paths.detoured.sum())
