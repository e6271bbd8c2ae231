"""The path speeds on the device (run with -m gpu on an MI355X): fcpp_path_speeds against the host twin fcpp_debug_path_speeds on the path
sets of tests/path_speed_cases.py -- status and cap bit for bit (cap is pointwise), the stops exactly 0, v to the derived bound
(n_p + 4) 2^-52 (the kernels compose the same non-negative terms in other groupings than the sweeps) -- at every path length around the
tile size, with doubled cusps and junctions on every tile seam, on ramps that cross several tiles, across path boundaries in the spine and
in its second block; then engine.path_speeds through plan_polygon_fields on a planned holed square."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import path_speed_cases as S

pytestmark = pytest.mark.gpu

HOLED = [[(0, 0), (30, 0), (30, 30), (0, 30)], [(12, 12), (18, 12), (18, 18), (12, 18)]]


def against_twin(ps, prm, what):
    v, cap, status = S.device_speeds(ps, prm)
    hv, hcap, hstatus = S.host_speeds(ps, prm)
    assert np.array_equal(status, hstatus), what
    assert np.array_equal(cap.view(np.int64), hcap.view(np.int64)), what
    S.assert_within_bound(ps, v, hv, what)
    off = ps['offsets']
    for p in np.flatnonzero(status == 0):
        st = S.stops(ps['gear'][off[p]:off[p + 1]], prm.flags)
        assert (v[off[p]:off[p + 1]][st] == 0.0).all(), (what, p)
    return v, cap, status


def two_piece(n):
    return S.path([(n // 2, 0.0, 0, 1), (n - n // 2, 0.2, 1, 1)]) if n >= 3 else S.path([(n, 0.0, 0, 1)])


def test_fixed_and_random_sets():
    for name, kw in (('default', {}), ('asym', dict(a_acc=0.3, a_dec=0.9)), ('free', dict(flags=0, turn_kmh=np.inf))):
        against_twin(S.fixed_set(), S.params(**kw), name)
        against_twin(S.random_set(np.random.default_rng(7), n_paths=60, max_n=300), S.params(**kw), name)


def test_path_lengths_around_the_tile():
    ps = S.pack([two_piece(n) for n in (0, 1, 2, 3, 511, 512, 513, 1023, 1024, 1025)])
    assert np.diff(ps['offsets']).tolist() == [0, 1, 2, 3, 511, 512, 513, 1023, 1024, 1025]
    for kw in ({}, dict(flags=0), dict(a_acc=0.05, a_dec=0.08)):
        against_twin(ps, S.params(**kw), kw)


def test_doubled_pairs_on_every_tile_seam():
    """every length 500 .. 530 and 1020 .. 1030, a doubled cusp and a doubled junction at L/2 - 2 .. L/2 + 2: wherever the tiling cuts
    a path of two or three tiles, some pairs straddle the cut"""
    paths = [S.seam_path(n, n // 2 + k, cusp) for n in list(range(500, 531)) + list(range(1020, 1031)) for k in range(-2, 3) for cusp in (True, False)]
    ps = S.pack(paths)
    v, cap, status = against_twin(ps, S.params(a_acc=0.4, a_dec=0.7), 'seams')
    S.check_properties(ps, S.params(a_acc=0.4, a_dec=0.7), v, cap, status, slack=lambda n: n + 4)


def test_long_ramps_cross_tiles():
    """0.05 m steps at a_acc = 0.05: 1250 steps from rest to 9 km/h; a_dec = 0.08: 781 steps back to rest.  Swapped limits show."""
    ps = S.pack([S.path([(3000, 0.0, 0, 1)], spacing=0.05)])
    prm = S.params(a_acc=0.05, a_dec=0.08)
    v, cap, _ = against_twin(ps, prm, 'ramp')
    assert v[0] == 0.0 and v[-1] == 0.0
    assert (v[1:1250] < cap[1:1250]).all() and (v[1252:2210] == cap[1252:2210]).all() and (v[2222:-1] < cap[2222:-1]).all()
    s = 0.05 * np.arange(1, 1200)
    assert np.allclose(v[1:1200], np.sqrt(2 * 0.05 * s) * 3.6, rtol=1e-10)
    assert (np.diff(v[:1250]) > 0).all() and (np.diff(v[2222:]) < 0).all()


def test_many_short_paths():
    """3000 paths of 3 samples with different caps: the spine's resets between paths"""
    rng = np.random.default_rng(11)
    paths = [S.path([(3, float(rng.choice([0.0, 0.05, 0.4, -1.0])), int(rng.integers(0, 7)), int(rng.choice([1, -1])))], spacing=float(rng.choice([0.02, 0.3])))
             for _ in range(3000)]
    ps = S.pack(paths)
    for kw in (dict(flags=0, nominal=[9.0, 15.0, 12.0, 11.0, 7.0, 5.0, 3.0, 1.0]), dict(nominal=[9.0, 15.0, 12.0, 11.0, 7.0, 5.0, 3.0, 1.0])):
        against_twin(ps, S.params(**kw), 'short')


def test_second_spine_block():
    """more tiles than one block of the spine (2048 tiles): one path of 300 000 samples and 1600 of 500"""
    rng = np.random.default_rng(3)
    long = S.path([(5000, 0.0, 0, 1), (400, 0.2, 1, 1), (300, -0.2, 1, -1), (4300, 0.0, 0, 1)] * 30)
    short = [S.path([(250 + int(rng.integers(0, 10)), 0.0, 0, 1), (240, float(rng.choice([0.1, 0.5])), 1, int(rng.choice([1, -1])))]) for _ in range(40)]
    ps = S.pack(short * 20 + [long] + short * 20)
    assert len(ps['x']) > 1.05e6 and sum(-(-int(n) // 512) for n in np.diff(ps['offsets'])) > 2048
    against_twin(ps, S.params(a_acc=0.3, a_dec=0.5), 'second block')


def test_a_path_alone_and_inside_a_batch():
    """The spine counts tiles from the batch's first, so a path's sums are grouped by where it lies: alone and embedded both meet the
    bound against the twin (and each other to twice the bound); they need not be the same bits"""
    one = S.path([(700, 0.0, 0, 1), (90, 0.25, 1, 1), (60, -0.25, 1, -1), (800, 0.0, 0, 1)])
    filler = [S.straight_arc_straight(300 + 7 * k, 50, 200) for k in range(9)]
    prm = S.params(a_acc=0.2, a_dec=0.35)
    alone = against_twin(S.pack([one]), prm, 'alone')[0]
    ps = S.pack(filler[:5] + [one] + filler[5:])
    inside = against_twin(ps, prm, 'inside')[0][ps['offsets'][5]:ps['offsets'][6]]
    n = len(alone)
    assert (np.abs(alone - inside) <= 2 * (n + 4) * S.EPS * alone).all()
    print('alone and embedded: %d of %d samples differ in bits' % (int((alone != inside).sum()), n))


def test_failing_paths_and_null_outputs():
    import torch
    ps = S.fixed_set()
    off = ps['offsets']
    ps['kappa'][off[1] + 3] = np.nan
    ps['gear'][off[7] + 600] = 0
    v, cap, status = against_twin(ps, S.params(), 'failing')
    assert status.tolist() == [0, L.EINVAL, 0, 0, 0, 0, 0, L.EINVAL, 0, 0]
    assert np.isnan(v[off[1]:off[2]]).all() and np.isnan(cap[off[7]:off[8]]).all()
    # the engine on a tuple, every column as numpy
    veh = E.make_vehicle()
    sp = E.path_speeds((off, ps['x'], ps['y'], ps['kappa'], ps['part'], ps['gear']), veh, a_dec=0.9, turn_kmh=5.0)
    prm = S.params(a_acc=veh.max_longitudinal_accel, a_dec=0.9, turn_kmh=5.0, a_lat=veh.max_lateral_accel, safety_factor=veh.safety_factor)
    hv, hcap, hstatus = S.host_speeds(ps, prm)
    assert np.array_equal(sp.status.cpu().numpy(), hstatus) and np.array_equal(sp.cap.cpu().numpy().view(np.int64), hcap.view(np.int64))
    S.assert_within_bound(ps, sp.v.cpu().numpy(), hv, 'engine')
    assert isinstance(sp.v, torch.Tensor) and sp.offsets_host is not None


def test_on_a_planned_holed_square():
    import torch
    veh = E.make_vehicle()
    kw = dict(width=4.0, radius=2.0, spacing=0.5, angles=[0.0, 0.5], passes=1, headland_paths=True, reversing=True, mission='headland_first')
    plan = E.plan_polygon_fields([HOLED], speeds=veh, **kw)
    m, sp = plan.mission, plan.speeds
    assert isinstance(sp, E.PathSpeeds) and m.status.tolist() == [0] and sp.status.tolist() == [0] and sp.v.shape == m.x.shape
    ps = dict(offsets=m.offsets_host, x=m.x.cpu().numpy(), y=m.y.cpu().numpy(), kappa=m.kappa.cpu().numpy(), part=m.part.cpu().numpy(),
              gear=m.gear.cpu().numpy())
    prm = sp.params
    v, cap = sp.v.cpu().numpy(), sp.cap.cpu().numpy()
    hv, hcap, hstatus = S.host_speeds(ps, prm)
    assert np.array_equal(cap.view(np.int64), hcap.view(np.int64)) and (hstatus == 0).all()
    S.assert_within_bound(ps, v, hv, 'plan')
    S.check_properties(ps, prm, v, cap, sp.status.cpu().numpy(), slack=lambda n: n + 4)
    gear = ps['gear']
    flip = np.flatnonzero(gear[1:] != gear[:-1])
    assert flip.size > 0 and (v[flip] == 0.0).all() and (v[flip + 1] == 0.0).all()          # every cusp stands, both samples
    assert v[0] == 0.0 and v[-1] == 0.0
    s, t, h, totals = sp.trajectory()
    t = t.cpu().numpy()
    length, time = (float(a) for a in totals[0])
    assert np.isfinite(t).all() and (np.diff(t) >= 0).all() and t[0] == 0.0
    top = max(prm.nominal_kmh) / 3.6
    print('mission: %d samples, %.1f m in %.1f s (at top speed %.1f s), %d cusps' % (len(v), length, time, length / top, flip.size))
    assert time >= length / top
    # headings with the reverse flags agree with the stored ones away from zero steps
    dh = np.abs(np.angle(np.exp(1j * (h.cpu().numpy() - m.heading.cpu().numpy()))))
    moving = np.concatenate([S.steps(ps['x'], ps['y']) > 0, [False]])
    assert np.median(dh[moving]) < 0.3
    assert (moving & (gear < 0)).sum() > 0 and np.median(dh[moving & (gear < 0)]) < 0.3
    flags, _ = E.validate(m.x, m.y, sp.v, veh, offsets=m.offsets_host)
    alat = (flags.cpu().numpy().view(np.uint32) & L.FLAG_ALAT) != 0
    curved = np.abs(ps['kappa']) > prm.kappa_eps
    for i in np.flatnonzero(alat & curved):
        print('FCPP_FLAG_ALAT on sample %d: stored kappa %.6f, v %.3f km/h, part %d' % (i, ps['kappa'][i], v[i], ps['part'][i]))
    assert not (alat & curved).any()
    # speeds=None: exactly the plan without the argument
    bare = E.plan_polygon_fields([HOLED], **kw)
    none = E.plan_polygon_fields([HOLED], speeds=None, **kw)
    assert bare.speeds is None and none.speeds is None
    for other in (bare, none):
        for k in ('x', 'y', 'heading', 'kappa'):
            assert torch.equal(getattr(other.mission, k).view(torch.int64), getattr(m, k).view(torch.int64))
            assert torch.equal(getattr(other.paths, k).view(torch.int64), getattr(plan.paths, k).view(torch.int64))
        for k in ('part', 'gear', 'offsets', 'slot', 'src'):
            assert torch.equal(getattr(other.mission, k), getattr(m, k))
    # without a mission the speeds are the field paths'
    fp_plan = E.plan_polygon_fields([HOLED], speeds=veh, **{**kw, 'mission': None})
    assert fp_plan.mission is None and fp_plan.speeds.v.shape == fp_plan.paths.x.shape and fp_plan.speeds.status.tolist() == [0]
