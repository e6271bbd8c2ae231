"""The path speeds through the guarded arena (tests/guarded.py; run with -m gpu on an MI355X): fcpp_path_speeds on slots carved out of ONE
uint8 CUDA tensor -- 256 bytes of 0xA5 in front of and behind every slot, outputs pre-filled with 0x5A, every pointer only naturally
aligned (the int8 columns at odd addresses).  After each call the guards are intact, the inputs have the bits that were put in, and every
element of v, cap and status is written.  cap and status are the host twin's bits; v is compared with the same call on ordinary tensors
(the same tiling, hence the same bits), which in turn meets the twin to the derived bound.  With v NULL, with cap NULL, and with a failing
path in the middle.  The test inspects memory afterwards; nothing in it provokes a fault."""
import ctypes as C

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import path_speed_cases as S
from tests.guarded import Arena

pytestmark = pytest.mark.gpu

COLS = ('x', 'y', 'kappa', 'part', 'gear')


@pytest.fixture
def gpu():
    import torch
    ctx = E.get_context(None)
    ctx.bind_stream()
    return ctx, torch.device('cuda', ctx.device)


def scene(failing):
    """paths of 0, 1, 3, 511, 513 and 1025 samples and the fixed shapes; a tile's last thread pair, odd counts, two and three tiles"""
    paths = [S.path([(n // 2, 0.0, 0, 1), (n - n // 2, 0.2, 1, -1)]) for n in (0, 1, 3, 511, 513, 1025)]
    ps = S.pack(paths[:3] + [S.reeds_shepp_like(57, 33, 140), S.straight_arc_straight(300, 90, 211)] + paths[3:])
    if failing:
        ps['x'][ps['offsets'][4] + 100] = np.inf
    return ps


@pytest.mark.parametrize('failing', [False, True])
def test_every_element_written_nothing_beside(gpu, failing):
    ctx, dev = gpu
    ps, prm = scene(failing), S.params(a_acc=0.4, a_dec=0.7)
    v, cap, status = S.device_speeds(ps, prm)
    hv, hcap, hstatus = S.host_speeds(ps, prm)
    assert np.array_equal(status, hstatus) and np.array_equal(cap.view(np.int64), hcap.view(np.int64)) and int((status != 0).sum()) == int(failing)
    S.assert_within_bound(ps, v, hv, 'ordinary tensors')
    total, n = len(ps['x']), len(ps['offsets']) - 1
    for outs in (('v', 'cap'), ('cap',), ('v',)):
        A = Arena()
        A.input('offsets', ps['offsets'])
        for k in COLS:
            A.input(k, ps[k])
        for k in outs:
            A.output(k, np.float64, total)
        A.output('status', np.int32, n)
        A.build(dev)
        rc = ctx.lib.fcpp_path_speeds(ctx.handle, C.byref(prm), n, A.ptr('offsets'), total, *[A.ptr(k) for k in COLS], A.ptr('v'), A.ptr('cap'),
                                      A.ptr('status'), None)
        assert rc == L.OK, ctx.lib.fcpp_last_error()
        A.check({**{k: {'v': v, 'cap': hcap}[k] for k in outs}, 'status': hstatus})
