"""The loop transits through the guarded arena (tests/guarded.py; run with -m gpu on an MI355X): fcpp_loop_transit_solve, _counts and _fill
on slots carved out of ONE uint8 CUDA tensor -- 256 bytes of 0xA5 in front of and behind every slot, outputs pre-filled with 0x5A, every
pointer only naturally aligned.  The scene's rank -1 pairs (all found: no NaN among the expected values, bit equality is value equality),
n = 3 and n = 1, both modes, every output NULL in turn.  After each call the guards are intact, the inputs have the bits that were put
in, and every output element has the bits the host twin gives on ordinary arrays.  The test inspects memory afterwards; nothing in it
provokes a fault."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import loop_transit_cases as C
from tests.guarded import Arena
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu

REC = ('found', 'loop', 'st_i', 'st_j', 'in_word', 'in_seg', 'out_word', 'out_seg')
LOOP_IN = ('x', 'y', 'heading', 'kappa', 's', 'part', 'gear')


@pytest.fixture
def gpu():
    import torch
    ctx = E.get_context(None)
    ctx.bind_stream()
    return ctx, torch.device('cuda', ctx.device)


def case(mode, n):
    sc = C.scene(mode)
    b = sc['blocked'][:n]
    frm, to = sc['frm'][b], sc['to'][b]
    want = C.host_transits(mode, frm, to, C.SCENE_R, 0, sc['region'], sc['ls'], C.SCENE_STRIDE, spacing=C.SCENE_SPACING)
    assert np.all(want['found'] == 1) and not any(np.isnan(want[k]).any() for k in ('in_seg', 'out_seg', 'ride', 'total'))
    return frm, to, np.zeros(len(b), np.int64), pack(sc['region']), sc['ls'], want


def inputs(A, frm, to, pf, region, ls):
    ro, vo, x, y = region
    for name, a in (('fx', frm[:, 0]), ('fy', frm[:, 1]), ('fh', frm[:, 2]), ('tx', to[:, 0]), ('ty', to[:, 1]), ('th', to[:, 2]), ('pair_field', pf),
                    ('ro', ro), ('vo', vo), ('rx', x), ('ry', y), ('loff', ls['off']), ('field_loops', ls['field_loops'])):
        A.input(name, a)
    for k in LOOP_IN:
        A.input('loop_' + k, ls[k])


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [3, 1])
def test_solve_stays_in_bounds(gpu, mode, n):
    ctx, dev = gpu
    frm, to, pf, region, ls, want = case(mode, n)
    ro, vo, x, y = region
    names = [k for k, _ in C.SOLVE_OUTS]
    for outs in [tuple(names)] + [tuple(k for k in names if k != drop) for drop in names]:
        A = Arena()
        inputs(A, frm, to, pf, region, ls)
        for k, dt in C.SOLVE_OUTS:
            if k in outs:
                A.output(k, dt, want[k].size)
        A.build(dev)
        rc = ctx.lib.fcpp_loop_transit_solve(ctx.handle, mode, n, A.ptr('fx'), A.ptr('fy'), A.ptr('fh'), A.ptr('tx'), A.ptr('ty'), A.ptr('th'), C.SCENE_R,
                                             A.ptr('pair_field'), len(ro) - 1, A.ptr('ro'), len(vo) - 1, A.ptr('vo'), len(x), A.ptr('rx'), A.ptr('ry'),
                                             len(ls['off']) - 1, A.ptr('loff'), None, len(ls['x']), A.ptr('loop_x'), A.ptr('loop_y'), A.ptr('loop_heading'),
                                             A.ptr('loop_s'), A.ptr('loop_part'), A.ptr('loop_gear'), A.ptr('field_loops'), None, C.SCENE_STRIDE,
                                             *[A.ptr(k) for k in names])
        assert rc == L.OK, ctx.lib.fcpp_last_error()
        A.check({k: want[k].reshape(-1) for k in outs})


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [3, 1])
def test_counts_and_fill_stay_in_bounds(gpu, mode, n):
    ctx, dev = gpu
    frm, to, pf, region, ls, want = case(mode, n)
    total = int(want['offsets'][-1])
    paths = [k for k, _ in C.PATH_OUTS]
    A = Arena()
    inputs(A, frm, to, pf, region, ls)
    for k in REC:
        A.input(k, want[k])
    A.output('offsets', np.int64, n + 1)
    A.build(dev)
    rec = [A.ptr(k) for k in REC]
    rc = ctx.lib.fcpp_loop_transit_counts(ctx.handle, mode, n, *rec, len(ls['off']) - 1, A.ptr('loff'), None, len(ls['x']), C.SCENE_SPACING,
                                          A.ptr('offsets'), None)
    assert rc == L.OK, ctx.lib.fcpp_last_error()
    A.check({'offsets': want['offsets']})
    for outs in [tuple(paths)] + [tuple(k for k in paths if k != drop) for drop in paths]:
        A = Arena()
        inputs(A, frm, to, pf, region, ls)
        for k in REC:
            A.input(k, want[k])
        A.input('offsets', want['offsets'])
        for k, dt in C.PATH_OUTS:
            if k in outs:
                A.output('p_' + k, dt, total)
        A.build(dev)
        rec = [A.ptr(k) for k in REC]
        rc = ctx.lib.fcpp_loop_transit_fill(ctx.handle, mode, n, A.ptr('fx'), A.ptr('fy'), A.ptr('fh'), C.SCENE_R, *rec, len(ls['off']) - 1, A.ptr('loff'),
                                            None, len(ls['x']), A.ptr('loop_x'), A.ptr('loop_y'), A.ptr('loop_heading'), A.ptr('loop_kappa'),
                                            A.ptr('loop_gear'), C.SCENE_SPACING, A.ptr('offsets'), None, total, *[A.ptr('p_' + k) for k in paths])
        assert rc == L.OK, ctx.lib.fcpp_last_error()
        A.check({'p_' + k: want['p_' + k] for k in outs})
