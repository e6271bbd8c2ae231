"""CPU-side tests of the guarded arena (tests/guarded.py) and, through it, of the host twins.

First the harness proves itself: deliberately wrong writers written in numpy -- one element past the end, one in front of the start, the
last element left out, a bit of an input flipped -- must each fail the check with a message that names the slot, for every element size the
device tests use.  That is what shows tests/test_gpu_guarded.py would fail on such a kernel.  In-out slots (a buffer the call reads and
rewrites, as fcpp_ga_evolve's population) are proved the same way: left untouched where a change was expected, or written beside.  So is an
output the call may write only in part (a mask of the elements it must leave alone: fcpp_batch_connectors' rows, fcpp_corner_turns' row
tails): a write into a masked element is caught, a skipped unmasked one is, a correct partial write passes.

Then fcpp_debug_dubins, fcpp_debug_rs, fcpp_debug_swaths, fcpp_debug_route_transit and fcpp_debug_route run through a numpy arena on the
batches the device tests use (defined here, imported there): the twins stay inside their buffers, leave their inputs alone and give the
values of a plain call -- and the shapes are what they claim to be (vertex counts on the chunk edges, 71 rings, 64 crossings, more than 64
lines, 255 / 256 / 257 swaths) before a GPU is involved."""
import os
import re

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from tests.guarded import FILL_BYTE, GUARD, GUARD_BYTE, Arena, GuardError
from tests.support import REPO
from tests.test_dubins_host import host_solve as dubins_host
from tests.test_dubins_host import random_pairs
from tests.test_route_host import MIN_GAIN, cut_with_angle, ends, host_route, host_transit
from tests.test_route_host import R as R_ROUTE
from tests.test_rs_host import host_solve as rs_host
from tests.test_swaths_host import comb, host_cut, host_scores, pack, rings_of, star

CSRC = os.path.join(REPO, 'field_coverage_path_planning_amd', 'csrc')


# ---- the batches (shared with the device tests) ---------------------------------------------------------------------------------------
R_CONN, SPACING = 2.0, 0.5
SOLVE_N = (1, 255, 257)
SAMPLE_N = 257


def solve_pairs(n, reversing=False):
    """n near pairs of tests/test_dubins_host.py's generator (the goal within 4 R of the start: every word family occurs)"""
    return random_pairs(np.random.default_rng(9000 + 2 * n + int(reversing)), n, R_CONN, True)


def tile_rows(reversing=False):
    """the row-tile constant of the matrix kernel (one for both connector kinds), from the header the kernel is compiled with"""
    return int(re.search(r'\bCONN_ROWS = (\d+)', open(os.path.join(CSRC, 'fcpp_conn.h')).read()).group(1))


def matrix_shapes(reversing=False):
    return [(1, 1), (3, 255), (tile_rows(reversing) + 1, 257)]


def matrix_poses(nf, nt):
    """two pose lists inside a box of 6 R, so near pairs (three-arc words, reversing words) occur across the lists"""
    rng = np.random.default_rng(100 * nf + nt)
    make = lambda n: np.column_stack([rng.uniform(0.0, 6 * R_CONN, n), rng.uniform(0.0, 6 * R_CONN, n), rng.uniform(-np.pi, np.pi, n)])
    return make(nf), make(nt)


def cols(poses):
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    return [np.ascontiguousarray(p[:, k]) for k in range(3)]


# swaths: W = 3.2, first = 1.6, an oblique angle per field
SW_W, SW_FIRST = 3.2, 1.6
STAR_SIZES = (62, 63, 64, 65, 125, 126, 127, 189, 190)      # a ring that ends on a 63-edge chunk (63, 126, 189), a one-edge chunk (64, 127)


def ring(n, radius, phase, centre=(0.0, 0.0)):
    a = phase + 2.0 * np.pi * np.arange(n) / n
    return np.column_stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)])


RING63_HOLE64 = [ring(63, 100.0, 0.05), ring(64, 30.0, 0.02)]      # a chunk edge ON the ring boundary, then a hole that ends in a one-edge chunk


def grid_field():
    """a 200 m square with a 7 x 10 grid of 4 m square holes: 71 rings, more than the 64 lanes that stride them"""
    sq = lambda x, y, s: np.array([(x, y), (x + s, y), (x + s, y + s), (x, y + s)], dtype=np.float64)
    return [sq(0.0, 0.0, 200.0)] + [sq(15.0 + 25.0 * i, 10.0 + 19.0 * j, 4.0) for j in range(10) for i in range(7)]


GRID71 = grid_field()
GRID71_SHORT = [r[:2] if k == 66 else r for k, r in enumerate(grid_field())]          # ring 66 has two vertices
GRID71_NAN = grid_field()
GRID71_NAN[68][2, 1] = np.nan                                                          # a NaN vertex in ring 68
EDGE_KINDS = [('star%d' % m, star(m, m)) for m in STAR_SIZES] + [('ring63_hole64', RING63_HOLE64), ('grid71', GRID71),
                                                                 ('grid71_short', GRID71_SHORT), ('grid71_nan', GRID71_NAN)]
EDGE_STATUS = {'grid71_short': L.EINVAL, 'grid71_nan': L.EINVAL}
# exactly at the cap: comb(32) has 64 crossings on a line through its teeth, comb(33) 66
CAP_FIELDS = [comb(32), comb(33)]


def edge_batch():
    """-> names, fields, angles: the block-edge fields with an oblique angle of their own each"""
    rng = np.random.default_rng(2024)
    return [k for k, _ in EDGE_KINDS], [rings_of(f) for _, f in EDGE_KINDS], rng.uniform(0.1, 1.4, len(EDGE_KINDS)) * rng.choice([-1.0, 1.0], len(EDGE_KINDS))


SCORE_ANGLES = np.array([0.0, 0.37, -1.2])


def assert_edge_shapes(names, fields, cut):
    """the block-edge fields are what they claim to be"""
    for i, (name, f) in enumerate(zip(names, fields)):
        if name.startswith('star'):
            assert len(f) == 1 and len(f[0]) == int(name[4:])
        if name == 'ring63_hole64':
            assert [len(r) for r in f] == [63, 64]
        if name.startswith('grid71'):
            assert len(f) == 71
        assert cut['status'][i] == EDGE_STATUS.get(name, 0), name
        if name in EDGE_STATUS:
            assert cut['n_swaths'][i] == 0 and cut['n_lines'][i] == 0 and cut['offsets'][i + 1] == cut['offsets'][i], name
        else:
            assert cut['n_swaths'][i] > 20 and cut['n_lines'][i] > 20, name
    assert len(GRID71_SHORT[66]) == 2 and np.isnan(GRID71_NAN[68]).any()


# the router: R = 6, W = 3.2, strips of k working widths (k swaths at angle 0)
ROUTE_W, ROUTE_S = 3.2, 5
ROUTE_STRIPS = (255, 256, 257, 511, 512)      # a tour that ends on the 256-thread stride, one over, one under; the cap and one under
GUARDED_STRIPS = ROUTE_STRIPS[:3]


def strip(k):
    return np.array([(0, 0), (30, 0), (30, ROUTE_W * k), (0, ROUTE_W * k)], dtype=np.float64)


def route_cut(strips):
    cut = cut_with_angle([strip(k) for k in strips], 0.0, ROUTE_W)
    assert list(np.diff(cut['offsets'])) == list(strips)
    return cut


def assert_permutations(tours, soff):
    """every candidate's tour holds every swath of its field once"""
    for c in range(tours.shape[0]):
        for i in range(len(soff) - 1):
            t = tours[c, soff[i]:soff[i + 1]]
            assert np.array_equal(np.sort(t >> 1), np.arange(len(t))), (c, i)


# ---- 1: the harness catches wrong writers ---------------------------------------------------------------------------------------------
X_IN = np.arange(1.0, 8.0)
RIGHT = {'word': np.arange(1, 8, dtype=np.int8), 'idx': 1000 + np.arange(7, dtype=np.int32), 'y': 2.0 * X_IN}


def _toy():
    A = Arena().input('x', X_IN).output('word', np.int8, 7).output('idx', np.int32, 7).output('y', np.float64, 7).build()
    for name, v in RIGHT.items():
        A.view(name)[:] = v
    return A


def test_layout_alignment_and_fill():
    A = Arena().input('x', X_IN).output('word', np.int8, 7).output('idx', np.int32, 7).output('y', np.float64, 7).output('none', np.float64, 0).build()
    spans = [A.span(n) for n in ('x', 'word', 'idx', 'y', 'none')]
    assert spans[0][0] >= GUARD and len(A.raw) - spans[-1][1] >= GUARD
    for (_, e), (s, _) in zip(spans[:-1], spans[1:]):
        assert s - e >= GUARD
    assert A.address('x') % 16 == 8 and A.address('y') % 16 == 8 and A.address('idx') % 8 == 4 and A.address('word') % 2 == 1
    assert (A.view('y').view(np.uint8) == FILL_BYTE).all() and np.array_equal(A.view('x'), X_IN)
    mask = np.ones(len(A.raw), dtype=bool)
    for s, e in spans:
        mask[s:e] = False
    assert (A.raw[mask] == GUARD_BYTE).all()
    assert A.ptr('missing') is None and A.ptr('y').value == A.address('y')


def test_a_right_writer_passes():
    got = _toy().check(RIGHT)
    assert all(np.array_equal(got[k], RIGHT[k]) for k in RIGHT)


@pytest.mark.parametrize('name', ['word', 'idx', 'y'])
def test_one_element_past_the_end_is_caught(name):
    A = _toy()
    s, e = A.span(name)
    size = A.view(name).itemsize
    A.raw[e:e + size] = A.raw[e - size:e]
    with pytest.raises(GuardError, match=r'guard bytes were written.*behind the end of slot %r' % name):
        A.check(RIGHT)


@pytest.mark.parametrize('name', ['word', 'idx', 'y'])
def test_one_element_before_the_start_is_caught(name):
    A = _toy()
    s, e = A.span(name)
    size = A.view(name).itemsize
    A.raw[s - size:s] = A.raw[s:s + size]
    with pytest.raises(GuardError, match=r'guard bytes were written.*in front of slot %r' % name):
        A.check(RIGHT)


@pytest.mark.parametrize('name', ['word', 'idx', 'y'])
def test_a_last_element_left_unwritten_is_caught(name):
    A = _toy()
    A.view(name).view(np.uint8)[-A.view(name).itemsize:] = FILL_BYTE
    with pytest.raises(GuardError, match=r'output slot %r: 1 of 7 elements differ \(1 of them still pre-filled\), the first element 6' % name):
        A.check(RIGHT)


def test_a_flipped_input_bit_is_caught():
    A = _toy()
    A.view('x').view(np.uint8)[8 * 3] ^= 1
    with pytest.raises(GuardError, match=r"input slot 'x' was written: 1 bytes differ, the first in element 3"):
        A.check(RIGHT)


def test_wrong_values_prefill_values_and_forbidden_slots_are_caught():
    A = _toy()
    A.view('idx')[2] += 1
    with pytest.raises(GuardError, match=r"output slot 'idx': 1 of 7 elements differ \(0 of them still pre-filled\), the first element 2"):
        A.check(RIGHT)
    # an expected value that IS the pre-fill pattern could pass unwritten: refused
    A = _toy()
    A.view('word')[4] = FILL_BYTE
    with pytest.raises(GuardError, match=r"expected\['word'\]\[4\] is the pre-fill pattern"):
        A.check(dict(RIGHT, word=A.view('word').copy()))
    # a slot the call must leave alone
    A = Arena().output('y', np.float64, 3).output('quiet', np.int32, 3, written=False).build()
    A.view('y')[:] = 1.0
    A.check({'y': np.ones(3)})
    A.view('quiet')[1] = 0
    with pytest.raises(GuardError, match=r"slot 'quiet' must not be written"):
        A.check({'y': np.ones(3)})
    # the expected values name exactly the written outputs, with their type and size
    for bad in ({}, dict(RIGHT, quiet=np.zeros(1)), dict(RIGHT, y=RIGHT['y'][:6]), dict(RIGHT, idx=RIGHT['idx'].astype(np.int64))):
        with pytest.raises(GuardError):
            _toy().check(bad)


def _toy_inout():
    """x is read, `state` is read and rewritten (every element but the third changes), y is written"""
    state = 10 + np.arange(5, dtype=np.int32)
    want = {'state': np.array([20, 21, 12, 23, 24], dtype=np.int32), 'y': np.ones(5)}
    A = Arena().input('x', X_IN).inout('state', state).output('y', np.float64, 5).build()
    assert A.address('state') % 8 == 4 and np.array_equal(A.view('state'), state)          # pre-filled with the input
    return A, state, want


def test_inout_slots_are_checked_like_outputs():
    A, state, want = _toy_inout()
    A.view('y')[:] = 1.0
    # left untouched when a change was expected
    with pytest.raises(GuardError, match=r"in-out slot 'state': 4 of 5 elements differ \(4 of them still the input\), the first element 0"):
        A.check(want)
    # the expected values must name it
    with pytest.raises(GuardError, match='expected values for'):
        A.check({'y': want['y']})
    A.view('state')[:] = want['state']
    got = A.check(want)
    assert np.array_equal(got['state'], want['state']) and np.array_equal(got['y'], want['y'])
    # one wrong element
    A.view('state')[1] = 7
    with pytest.raises(GuardError, match=r"in-out slot 'state': 1 of 5 elements differ \(0 of them still the input\), the first element 1"):
        A.check(want)


@pytest.mark.parametrize('side', ['behind', 'in front'])
def test_a_write_beside_an_inout_slot_is_caught(side):
    A, state, want = _toy_inout()
    A.view('y')[:] = 1.0
    A.view('state')[:] = want['state']
    s, e = A.span('state')
    if side == 'behind':
        A.raw[e:e + 4] = A.raw[e - 4:e]
    else:
        A.raw[s - 4:s] = A.raw[s:s + 4]
    with pytest.raises(GuardError, match=r"guard bytes were written.*%s" % ("behind the end of slot 'state'" if side == 'behind' else "in front of slot 'state'")):
        A.check(want)


def test_inout_prefill_pattern_rule():
    """an expected element that IS the 0x5A pattern is refused -- unless the input element already was that value (the call may leave it)"""
    fill = np.frombuffer(bytes([FILL_BYTE] * 4), dtype=np.int32)[0]
    A = Arena().inout('state', np.array([1, fill, 3], dtype=np.int32)).build()
    A.view('state')[:] = [5, fill, 6]
    A.check({'state': np.array([5, fill, 6], dtype=np.int32)})
    A = Arena().inout('state', np.array([1, 2, 3], dtype=np.int32)).build()
    A.view('state')[:] = [5, fill, 6]
    with pytest.raises(GuardError, match=r"expected\['state'\]\[1\] is the pre-fill pattern"):
        A.check({'state': np.array([5, fill, 6], dtype=np.int32)})


def _toy_masked(at_check):
    """rows of 3: the call writes rows 0 and 2 and the first element of row 1 -- the rest of row 1 it must leave alone"""
    keep = np.zeros(9, dtype=bool)
    keep[4:6] = True
    want = {'rows': 100.0 + np.arange(9), 'n': np.array([3, 1, 3], dtype=np.int32)}
    A = Arena().input('x', X_IN).output('rows', np.float64, 9, keep=None if at_check else keep).output('n', np.int32, 3).build()
    A.view('n')[:] = want['n']
    A.view('rows')[~keep] = want['rows'][~keep]
    return A, want, ({'rows': keep} if at_check else None)


@pytest.mark.parametrize('at_check', [False, True], ids=['mask at output()', 'mask at check()'])
def test_a_partly_written_output(at_check):
    # a correct partial write passes, whatever the expected values say where the mask is set -- the pre-fill pattern included
    A, want, keep = _toy_masked(at_check)
    got = A.check(want, keep=keep)
    assert np.array_equal(got['rows'][:4], want['rows'][:4]) and (got['rows'][4:6].view(np.uint8) == FILL_BYTE).all()
    A.check(dict(want, rows=np.where(np.arange(9) == 4, A.view('rows')[4], want['rows'])), keep=keep)
    # a write into a masked element is caught, the right value too
    A, want, keep = _toy_masked(at_check)
    A.view('rows')[5] = want['rows'][5]
    with pytest.raises(GuardError, match=r"output slot 'rows': 1 of the 2 elements the call must leave alone were written, the first element 5"):
        A.check(want, keep=keep)
    # one byte of a masked element
    A, want, keep = _toy_masked(at_check)
    A.view('rows').view(np.uint8)[8 * 4 + 7] ^= 0x80
    with pytest.raises(GuardError, match=r"must leave alone were written, the first element 4"):
        A.check(want, keep=keep)
    # a skipped unmasked element is caught as ever
    A, want, keep = _toy_masked(at_check)
    A.view('rows').view(np.uint8)[8 * 3:8 * 4] = FILL_BYTE
    with pytest.raises(GuardError, match=r"output slot 'rows': 1 of 9 elements differ \(1 of them still pre-filled\), the first element 3"):
        A.check(want, keep=keep)
    # ... and so are a wrong value, an unmasked expected element that is the pre-fill pattern, and a write beside the slot
    A, want, keep = _toy_masked(at_check)
    A.view('rows')[8] += 1.0
    with pytest.raises(GuardError, match=r"output slot 'rows': 1 of 9 elements differ \(0 of them still pre-filled\), the first element 8"):
        A.check(want, keep=keep)
    A, want, keep = _toy_masked(at_check)
    fill = np.frombuffer(bytes([FILL_BYTE] * 8), dtype=np.float64)[0]
    A.view('rows')[6] = fill
    with pytest.raises(GuardError, match=r"expected\['rows'\]\[6\] is the pre-fill pattern"):
        A.check(dict(want, rows=np.where(np.arange(9) == 6, fill, want['rows'])), keep=keep)
    A, want, keep = _toy_masked(at_check)
    s, e = A.span('rows')
    A.raw[e:e + 8] = A.raw[e - 8:e]
    with pytest.raises(GuardError, match=r"guard bytes were written.*behind the end of slot 'rows'"):
        A.check(want, keep=keep)


def test_masks_are_for_written_outputs_of_their_size():
    keep = np.zeros(9, dtype=bool)
    with pytest.raises(ValueError, match='mask'):
        Arena().output('rows', np.float64, 9, keep=keep[:8])
    with pytest.raises(ValueError, match='mask'):
        Arena().output('rows', np.float64, 9, keep=keep.astype(np.int8))
    A, want, _ = _toy_masked(True)
    for bad in ({'x': np.zeros(7, dtype=bool)}, {'missing': keep}):
        with pytest.raises(GuardError, match='no written output slot'):
            A.check(want, keep=bad)
    with pytest.raises(ValueError, match='mask'):
        A.check(want, keep={'rows': keep[:8]})
    # without a mask the untouched elements of row 1 fail as skipped elements
    with pytest.raises(GuardError, match=r"output slot 'rows': 2 of 9 elements differ \(2 of them still pre-filled\), the first element 4"):
        A.check(want)


# ---- 2: the host twins through a numpy arena ------------------------------------------------------------------------------------------
def solve_arena(frm, to, n_seg, outs, device=None):
    """the slots of fcpp_*_solve / fcpp_debug_dubins / _rs -> (arena, the argument list behind n)"""
    n = len(frm)
    A = Arena()
    for name, a in zip(('fx', 'fy', 'fh', 'tx', 'ty', 'th'), cols(frm) + cols(to)):
        A.input(name, a)
    for name, dtype, count in (('word', np.int32, n), ('seg', np.float64, n_seg * n), ('len', np.float64, n)):
        if name in outs:
            A.output(name, dtype, count)
    A.build(device)
    return A, [A.ptr(k) for k in ('fx', 'fy', 'fh', 'tx', 'ty', 'th')] + [R_CONN] + [A.ptr(k) for k in ('word', 'seg', 'len')]


SOLVE_SUBSETS = [('word', 'seg', 'len'), ('word',), ('seg',), ('len',)]


@pytest.mark.parametrize('reversing', [False, True], ids=['dubins', 'rs'])
@pytest.mark.parametrize('n', SOLVE_N)
def test_host_solve_stays_in_bounds(n, reversing):
    lib = L.load()
    frm, to = solve_pairs(n, reversing)
    word, seg, tot = (rs_host if reversing else dubins_host)(frm, to, R_CONN)
    want = {'word': word, 'seg': seg.reshape(-1), 'len': tot}
    assert (word >= 0).all() and (n < 255 or len(np.unique(word)) >= 4)
    for outs in SOLVE_SUBSETS:
        A, args = solve_arena(frm, to, 5 if reversing else 3, outs)
        assert (lib.fcpp_debug_rs if reversing else lib.fcpp_debug_dubins)(n, *args) == 0
        A.check({k: want[k] for k in outs})


def swath_inputs(A, fields, angles):
    ro, vo, x, y = pack(fields)
    for name, a in (('ring_offsets', ro), ('vert_offsets', vo), ('x', x), ('y', y), ('angles', np.ascontiguousarray(angles, dtype=np.float64))):
        A.input(name, a)
    return len(ro) - 1, len(vo) - 1, len(x)


def swath_head(A, n, nr, nv):
    return [n, A.ptr('ring_offsets'), nr, A.ptr('vert_offsets'), nv, A.ptr('x'), A.ptr('y')]


PAIR_OUTS = (('n_swaths', np.int32), ('n_lines', np.int32), ('length', np.float64), ('status', np.int32))
RECORD_OUTS = (('ax', np.float64), ('ay', np.float64), ('bx', np.float64), ('by', np.float64), ('line', np.int32), ('rec_length', np.float64))


def swath_cases():
    names, fields, angles = edge_batch()
    return [('edges', fields, angles, SW_W, SW_FIRST), ('cap', CAP_FIELDS, np.zeros(2), 5.0, 0.0), ('cap_late', CAP_FIELDS, np.zeros(2), 0.5, 0.0)]


def record_values(cut):
    return {'ax': cut['ax'], 'ay': cut['ay'], 'bx': cut['bx'], 'by': cut['by'], 'line': cut['line'], 'rec_length': cut['length']}


@pytest.mark.parametrize('case', swath_cases(), ids=lambda c: c[0])
def test_host_swaths_stay_in_bounds(case):
    lib = L.load()
    what, fields, angles, W, first = case
    # the scores, three angles shared
    sc = host_scores(fields, SCORE_ANGLES, W, first)
    for outs in (tuple(k for k, _ in PAIR_OUTS), ('status',), ('length',)):
        A = Arena()
        n, nr, nv = swath_inputs(A, fields, SCORE_ANGLES)
        for k, dt in PAIR_OUTS:
            if k in outs:
                A.output(k, dt, n * 3)
        A.build()
        assert lib.fcpp_debug_swaths(*swath_head(A, n, nr, nv), 3, A.ptr('angles'), 0, W, first, 0.0, *[A.ptr(k) for k, _ in PAIR_OUTS], None, 0,
                                     *[None] * 6) == 0
        A.check({k: sc[k].reshape(-1) for k in outs})
    # the cut, an angle per field: the counts, then the records
    cut = host_cut(fields, angles, W, first)
    m = int(cut['offsets'][-1])
    pair = {'n_swaths': cut['n_swaths'], 'n_lines': cut['n_lines'], 'length': cut['total'], 'status': cut['status'], 'offsets': cut['offsets']}
    rec = record_values(cut)
    for outs in (tuple(rec), ('line',), ('ax',)):
        A = Arena()
        n, nr, nv = swath_inputs(A, fields, angles)
        for k, dt in PAIR_OUTS:
            A.output(k, dt, n)
        A.output('offsets', np.int64, n + 1)
        for k, dt in RECORD_OUTS:
            if k in outs:
                A.output(k, dt, m)
        A.build()
        assert lib.fcpp_debug_swaths(*swath_head(A, n, nr, nv), 1, A.ptr('angles'), 1, W, first, 0.0, *[A.ptr(k) for k, _ in PAIR_OUTS],
                                     A.ptr('offsets'), m, *[A.ptr(k) for k, _ in RECORD_OUTS]) == 0
        A.check(dict(pair, **{k: rec[k] for k in outs}))
    # the shapes are what they claim to be
    if what == 'edges':
        assert_edge_shapes(edge_batch()[0], fields, cut)
    else:
        assert cut['status'].tolist() == [0, L.EUNSUPPORTED] and cut['offsets'][2] == cut['offsets'][1]
        per_line = np.bincount(cut['line'], minlength=cut['n_lines'][0])
        assert per_line.max() == 32                                  # 64 crossings: exactly the cap
        if what == 'cap':
            assert cut['n_swaths'][0] == 2 + 6 * 32
        else:
            assert cut['n_lines'][0] > 64 and (per_line[64:] == 32).any()      # capped lines in the second block of 64 lines


def route_transit_arena(cut, toff, device=None):
    A = Arena()
    for name, a in (('soff', cut['offsets']), ('ax', cut['ax']), ('ay', cut['ay']), ('bx', cut['bx']), ('by', cut['by']), ('angle', cut['angle']),
                    ('toff', toff)):
        A.input(name, a)
    A.output('T', np.float64, int(toff[-1]))
    return A.build(device)


ROUTE_OUTS = (('tours', np.int32), ('costs', np.float64), ('route', np.int32), ('cost', np.float64), ('winner', np.int32), ('sweeps', np.int32),
              ('status', np.int32), ('stored', np.float64))
ROUTE_SUBSETS = [tuple(k for k, _ in ROUTE_OUTS), ('winner',), ('costs',), ('route', 'sweeps')]


def route_solve_arena(soff, toff, T, En, Xn, outs, device=None):
    n, nt = len(soff) - 1, int(soff[-1])
    sizes = {'tours': ROUTE_S * nt, 'costs': n * ROUTE_S, 'route': nt}
    A = Arena().input('soff', soff).input('toff', toff).input('T', T)
    if En is not None:
        A.input('E', En).input('X', Xn)
    for k, dt in ROUTE_OUTS:
        if k in outs:
            A.output(k, dt, sizes.get(k, n))
    return A.build(device)


def route_values(res):
    out = {k: np.ascontiguousarray(res[k]).reshape(-1) for k, _ in ROUTE_OUTS}
    # a NaN-free, finite result: nothing equals the pre-fill pattern by accident, and bit equality is value equality
    assert all(np.isfinite(out[k]).all() for k in ('costs', 'cost', 'stored'))
    return out


@pytest.fixture(scope='module')
def guarded_route():
    """the cut of the three strips and per mode the transit blocks and E / X of plain calls -- computed once, left unchanged"""
    cut = route_cut(GUARDED_STRIPS)
    return cut, {mode: host_transit(cut, R_ROUTE, mode) + ends(cut, mode) for mode in (0, 1)}


@pytest.mark.parametrize('mode', [0, 1])
def test_host_route_stays_in_bounds(guarded_route, mode):
    lib = L.load()
    cut, per_mode = guarded_route
    T, toff, En, Xn = per_mode[mode]
    soff = cut['offsets']
    n, nt, tt = len(soff) - 1, int(soff[-1]), int(toff[-1])
    A = route_transit_arena(cut, toff)
    assert lib.fcpp_debug_route_transit(n, A.ptr('soff'), nt, A.ptr('ax'), A.ptr('ay'), A.ptr('bx'), A.ptr('by'), A.ptr('angle'), R_ROUTE, mode,
                                        A.ptr('toff'), tt, A.ptr('T')) == 0
    A.check({'T': T})
    for with_ends in (True, False):
        E_, X_ = (En, Xn) if with_ends else (None, None)
        res = host_route(soff, T, toff, E_, X_, S=ROUTE_S, max_sweeps=3)
        want = route_values(res)
        assert np.all(res['status'] == 0) and res['sweeps'].max() >= 1
        assert_permutations(res['tours'], soff)
        for outs in ROUTE_SUBSETS if with_ends else ROUTE_SUBSETS[:1]:
            A = route_solve_arena(soff, toff, T, E_, X_, outs)
            assert lib.fcpp_debug_route(n, A.ptr('soff'), nt, A.ptr('toff'), tt, A.ptr('T'), A.ptr('E'), A.ptr('X'), ROUTE_S, MIN_GAIN, 3,
                                        *[A.ptr(k) for k, _ in ROUTE_OUTS]) == 0
            A.check({k: want[k] for k in outs})
