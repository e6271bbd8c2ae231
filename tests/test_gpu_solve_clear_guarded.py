"""The clear connectors through the guarded arena (tests/guarded.py; run with -m gpu on an MI355X): fcpp_conn_solve_clear on slots carved
out of ONE uint8 CUDA tensor, and its host twin on a numpy arena -- 256 bytes of 0xA5 in front of and behind every slot, outputs pre-filled
with 0x5A, every pointer only naturally aligned.  n = 65 and n = 1, both modes, every output NULL in turn.  After each call the guards are
intact, the inputs have the bits that were put in, and every output element has the bits the host twin gives on ordinary arrays.  The
test inspects memory afterwards; nothing in it provokes a fault."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from tests.guarded import Arena
from tests.support import Gpu
from tests.test_gpu_solve_clear import FIELDS, random_pairs
from tests.test_solve_clear_host import host_solve_clear
from tests.test_swaths_host import pack

pytestmark = pytest.mark.gpu

R = 4.0
OUTS = (('word', np.int32), ('seg', np.float64), ('len', np.float64), ('rank', np.int32), ('crossings', np.int32), ('field_status', np.int32))
SUBSETS = [tuple(k for k, _ in OUTS)] + [tuple(k for k, _ in OUTS if k != drop) for drop, _ in OUTS]
CASE_FIELDS = [FIELDS[0], FIELDS[4], FIELDS[6]]          # 3 edges, a square with a hole, 257 edges: all valid


@pytest.fixture
def gpu():
    g = Gpu()
    g.ctx.bind_stream()
    return g


def case(mode, n):
    """n solved pairs against valid fields or none: no NaN among the expected values (bit equality is value equality)"""
    frm, to = random_pairs(21 + mode, 65)
    pair_field = ((np.arange(65) * 7) % 4 - 1).astype(np.int64)
    if n == 1:
        want = host_solve_clear(mode, frm, to, R, pair_field, CASE_FIELDS)
        i = int(np.flatnonzero(want['rank'] >= 1)[0])                    # a pair that goes through both passes
        frm, to, pair_field = frm[i:i + 1], to[i:i + 1], pair_field[i:i + 1]
    want = host_solve_clear(mode, frm, to, R, pair_field, CASE_FIELDS)
    want = {k: np.ascontiguousarray(want[k]).reshape(-1) for k, _ in OUTS}
    assert not np.isnan(want['seg']).any() and (want['rank'] >= 1).any()
    assert n == 1 or ((want['rank'] == -1).any() and (want['rank'] == 0).any())
    return frm, to, pair_field, pack(CASE_FIELDS), want


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [65, 1])
@pytest.mark.parametrize('where', ['device', 'host'])
def test_conn_solve_clear_stays_in_bounds(gpu, mode, n, where):
    frm, to, pair_field, (ro, vo, x, y), want = case(mode, n)
    for outs in SUBSETS:
        A = Arena()
        for name, a in (('fx', frm[:, 0]), ('fy', frm[:, 1]), ('fh', frm[:, 2]), ('tx', to[:, 0]), ('ty', to[:, 1]), ('th', to[:, 2]),
                        ('pair_field', pair_field), ('ro', ro), ('vo', vo), ('x', x), ('y', y)):
            A.input(name, a)
        for k, dt in OUTS:
            if k in outs:
                A.output(k, dt, want[k].size)
        A.build(gpu.dev if where == 'device' else None)
        args = (mode, n, A.ptr('fx'), A.ptr('fy'), A.ptr('fh'), A.ptr('tx'), A.ptr('ty'), A.ptr('th'), R, A.ptr('pair_field'), len(ro) - 1, A.ptr('ro'),
                len(vo) - 1, A.ptr('vo'), len(x), A.ptr('x'), A.ptr('y'), *[A.ptr(k) for k, _ in OUTS])
        rc = gpu.lib.fcpp_conn_solve_clear(gpu.h, *args) if where == 'device' else gpu.lib.fcpp_debug_conn_solve_clear(*args)
        assert rc == L.OK, gpu.lib.fcpp_last_error()
        A.check({k: want[k] for k in outs})
