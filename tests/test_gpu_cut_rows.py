"""The ROW form of a direct setup's counting pass (k_tile_rows_direct): two fields per wavefront, a row of 32 lanes each, for the fields the
closed-form cut takes; every other field of the wavefront goes through the wave form's pass inside the same kernel.  FCPP_CUT_ROWS=0 (read
per call) keeps the form of a wavefront per field and is the checker: every batch is planned twice through Batch.plan, the first call
asserted to have taken the row form, and the pair compared on the five output arrays and the statistics bit for bit, on fcpp_field_info
and on all 23 tables byte for byte (reading them fills a direct batch's tables on demand).

A row has a lane per primitive, and the closed-form cut takes fields of up to 32.  How many a field has is mostly a property of the batch:
the number of headland loops is ceil(R / W) of the VEHICLE (three for the default one: the headline's fields have 27 primitives), and a
field has 8 primitives per loop plus a reverse fill for each of the three turned corners of 60 degrees or more -- a convex quadrilateral
has at most two corners below 60 degrees, so at least one of the three gets its fill: 8 n + 1 to 8 n + 3 primitives for n loops.  A batch
therefore cannot hold fields of three loops beside fields of four, and a field of EXACTLY 32 primitives would need four loops without any
reverse fill: the fills are dropped only when the corner arc's band of width W covers the corner's square of side 2 R to within 0.1 m^2,
and for R > W that band has less than half the square's area.  No vehicle of test_gpu_devplan.py (or any other) gives one.
What CAN share a wavefront with eligible rows, and does below: fields that fail in the planner, and fields of one pass (no span, so no
closed-form cut) -- in row 0 beside an ordinary field, in row 1 beside one, and in both rows.  The vehicle of four loops makes every row
of every wavefront ineligible (33 to 35 primitives)."""
import os
import sys

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from field_coverage_path_planning_amd import workloads as WL

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_devplan import _random_quads                                  # noqa: E402
from test_gpu_direct_step import _cfg1, _cfg2, _record, _same, _with_one_pass_fields      # noqa: E402

pytestmark = pytest.mark.gpu

ROWS_MIN_FIELDS = 16          # (fcpp_devplan.h; the smallest batch the device takes has sixteen fields, so there is no size below it to test)
FIELD_BYTES, PRIM_COUNT_AT = 312, 200       # DevField: its size, and where its prim_count lies


def _prime():
    """any qualifying speculative setup makes the context's last verdict one that lets the next call's direct step begin"""
    os.environ['FCPP_DIRECT'] = '0'
    try:
        b0, _ = E.Batch.plan(_cfg1(16), E.make_vehicle(), E.make_options())
    finally:
        del os.environ['FCPP_DIRECT']
    b0.close()


def _plan(table, veh=None, opt=None, rows=True, prime=True):
    """one plan call with a direct setup -> (batch, result, row passes this call added)"""
    ctx = E.get_context()
    env = {} if rows else {'FCPP_CUT_ROWS': '0'}
    if prime:
        _prime()
    before, steps = ctx.cut_rows_passes(), ctx.direct_steps()
    os.environ.update(env)
    try:
        b, r = E.Batch.plan(table, veh or E.make_vehicle(), opt or E.make_options())
    finally:
        for k in env:
            del os.environ[k]
    assert b.setup_path() == 'device'
    assert ctx.direct_steps() == steps + 1, 'a direct setup: the counting pass is the direct one'
    return b, r, ctx.cut_rows_passes() - before


def _pair(make, what, veh=None, opt=None):
    """the batch through the row form (asserted) and through the checker, compared; -> the row form's record"""
    b, r, passes = _plan(make(), veh, opt)
    assert passes == 1, (what, 'the row form was taken')
    got = _record(b, r)
    b.close()
    b, r, passes = _plan(make(), veh, opt, rows=False)
    assert passes == 0, (what, 'FCPP_CUT_ROWS=0 keeps the wave form')
    want = _record(b, r)
    b.close()
    _same(got, want, what)
    return got


def _info(rec):
    return np.frombuffer(rec['info'], dtype=np.dtype(L.FieldInfo))


def _prim_counts(rec):
    f = rec['tables'][0].view(np.uint8).reshape(-1, FIELD_BYTES)
    return f[:, PRIM_COUNT_AT:PRIM_COUNT_AT + 4].copy().view(np.int32).ravel()


# 16 ... 19: batches whose last wavefront has two live rows and one; 63, 64, 65: the edge of a block of the two-level offsets; 257: several blocks
@pytest.mark.parametrize('n', [16, 17, 18, 19, 63, 64, 65, 257])
def test_batch_sizes(n):
    rec = _pair(lambda: _cfg1(n), f'cfg1 x {n}')
    pc = _prim_counts(rec)
    assert pc.size == n and (pc >= 25).all() and (pc <= 27).all(), 'three headland loops: every row eligible'


@pytest.mark.parametrize('turn_model,ring', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_random_quadrilaterals(turn_model, ring):
    V = _random_quads(np.random.default_rng(20), 67)
    V[::13] *= 0.01                                    # (too small to plan: status < 0)
    rec = _pair(lambda: E.FieldTable.from_vertices(V), f'quads, turn model {turn_model}, ring {ring}', opt=E.make_options(turn_model, 0.0, ring_order=ring))
    st = _info(rec)['status']
    assert (st != 0).any() and (st == 0).any()


def _rect_vertices(n):
    LH = WL.cfg1_batch(n)
    V = np.zeros((n, 4, 2))
    V[:, 1, 0] = V[:, 2, 0] = LH[:, 0]
    V[:, 2, 1] = V[:, 3, 1] = LH[:, 1]
    return V


# row 0 of wavefront 0 and row 1 of wavefront 1 (the other row ordinary), both rows of wavefronts 2 and 3, row 1 of wavefront 4, row 0 of
# wavefront 5, a block's last field, and the batch's last, alone in its wavefront
SPECIAL = (0, 3, 4, 5, 6, 7, 9, 10, 63, 66)


def test_fields_that_fail_in_the_planner_share_wavefronts_with_ordinary_ones():
    def make():
        V = _rect_vertices(67)
        for k in SPECIAL:
            V[k, 2] = 0.3 * V[k, 2]                    # vertex 2 pulled inside: not convex
        return E.FieldTable.from_vertices(V)
    st = _info(_pair(make, 'non-convex fields'))['status']
    assert (st[list(SPECIAL)] != 0).all() and (np.delete(st, SPECIAL) == 0).all()


def test_fields_without_a_span_share_wavefronts_with_ordinary_ones():
    def make():
        LH = WL.cfg1_batch(67).copy()
        for k in SPECIAL:
            LH[k] = (500.0, 18.0)                      # one swath: a field of field work without a span
        return E.FieldTable.from_rectangles(LH)
    info = _info(_pair(make, 'one-pass fields'))
    assert (info['status'] == 0).all() and (info['n_swaths'][list(SPECIAL)] == 1).all() and (np.delete(info['n_swaths'], SPECIAL) > 1).all()
    _pair(lambda: _with_one_pass_fields(129), 'one-pass fields of the direct-step tests')


@pytest.mark.parametrize('width,radius,loops,prims', [(3.0, 5.0, 2, (17, 19)), (2.0, 5.0, 3, (25, 27)), (1.0, 4.0, 4, (33, 35))])
def test_the_edge_of_a_row_of_primitives(width, radius, loops, prims):
    """two and three headland loops: rows; four: every row ineligible, wavefronts of two fields for the wave form's pass inside the row kernel
    (see the module's docstring for why no batch mixes the two kinds and why no field has exactly 32 primitives)"""
    veh = E.make_vehicle(working_width=width, min_turn_radius=radius)
    V = _random_quads(np.random.default_rng(21), 35)
    rec = _pair(lambda: E.FieldTable.from_vertices(V), f'{loops} loops', veh=veh)
    info, pc = _info(rec), _prim_counts(rec)
    ok = info['status'] == 0
    assert ok.any() and (info['n_loops'][ok] == loops).all()
    assert (pc[ok] >= prims[0]).all() and (pc[ok] <= prims[1]).all()


def test_a_batch_the_direct_step_declines():
    _pair(_cfg2, 'cfg2 x 200')


def test_row_form_wave_form_row_form_on_one_slot():
    """three plan calls in a row, the earlier batches still open (each setup takes the plan slot and swaps the slot's two buffers of aggregates)"""
    a, ra, pa = _plan(_cfg1(129))
    b, rb, pb = _plan(_cfg1(65), rows=False, prime=False)         # (a taken call leaves a qualifying verdict)
    c, rc, pc = _plan(_cfg1(129), prime=False)
    assert (pa, pb, pc) == (1, 0, 1)
    got_a, got_b, got_c = _record(a, ra), _record(b, rb), _record(c, rc)
    for q in (a, b, c):
        q.close()
    w, rw, _ = _plan(_cfg1(129), rows=False)
    want_129 = _record(w, rw)
    w.close()
    w, rw, _ = _plan(_cfg1(65))
    want_65 = _record(w, rw)
    w.close()
    _same(got_a, want_129, 'first row-form call')
    _same(got_c, want_129, 'second row-form call')
    _same(got_b, want_65, 'the wave-form call between them')
