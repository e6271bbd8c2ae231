"""fcpp_patch_sizes, fcpp_patch_counts and fcpp_patch_fill on guarded buffers (tests/guarded.py): every output element is written and
nothing beside it, the inputs keep their bits, every pointer is only naturally aligned (the 64-byte records, the 32-byte dims, the frame
and the bitmap at 8 mod 16, the labels and `line` at 4 mod 8), the optional host copies are NULL, and the bitmap and the line counts are
handed over full of garbage.  Once, at the second-round sizes: a line of three rounds of bitmap words, more lines than one launch of the
runs kernel covers, more regions than one round of the scan, fields of several numbering blocks, an empty field and a field of one cell
between them, labels of -2 and a label that never occurs.  The expected values are the host twin's."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import engine as E
from tests import patch_cases as P
from tests.guarded import Arena

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('join', P.JOINS)
def test_sizes_counts_and_fill_on_guarded_buffers(join):
    import torch
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    shapes = P.shapes()
    grids = [P.many_lines(n_cu), np.zeros((0, 0), np.int32), P.lab((1, 1)), P.long_sliver(), shapes['minus_two'][0][0], shapes['absent_label'][0][0],
             P.blobs(8, 150, 200, 50, 0.7), P.two_labels_two_words(), P.ring()]
    n_reg = [int(g.max(initial=-1)) + 1 for g in grids]
    n_reg[5] += 2
    packed = P.pack(grids, n_reg)
    dims, off, flat, roff = packed
    n, k = len(grids), int(roff[-1])
    th = np.array([0.3, 0.0, -1.1, 0.0, 0.3, np.pi / 2, -1.1, 0.0, 0.0])
    host = P.twin(packed, th, join=join)
    nl, nw, ms = (int(v) for v in host['totals'])
    assert nl > P.runs_round_lines(n_cu) and k > 256 and host['records']['B'].max() == 9000 and ms > P.runs_round_lines(n_cu)
    rule = (P.W, P.RES / 2, float(join))

    a = Arena().input('dims', dims).input('cell_offsets', off).input('labels', flat).input('region_offsets', roff).input('angle', th)
    a.output('frame', np.float64, 2 * n).output('records', np.int64, 8 * k)
    a.build(dev)
    totals = np.full(2, -7, np.int64)
    ctx.bind_stream()
    rc = ctx.lib.fcpp_patch_sizes(ctx.handle, n, a.ptr('dims'), a.ptr('cell_offsets'), None, P.RES, a.ptr('labels'), a.ptr('region_offsets'), None, k,
                                  a.ptr('angle'), *rule, a.ptr('frame'), a.ptr('records'), totals.ctypes.data)
    assert rc == 0, ctx.lib.fcpp_last_error()
    a.check({'frame': host['frame'].reshape(-1), 'records': host['records'].view(np.int64)})
    assert totals.tolist() == [nl, nw]

    b = Arena().input('dims', dims).input('cell_offsets', off).input('labels', flat).input('region_offsets', roff)
    b.input('frame', host['frame'].reshape(-1)).input('records', host['records'].view(np.int64))
    b.output('bitmap', np.uint64, nw).output('line_counts', np.int64, nl).output('line_offsets', np.int64, nl + 1).output('swath_offsets', np.int64, n + 1)
    b.build(dev)          # (the outputs' pre-fill 0x5A5A.. is the garbage the bitmap and the counts start from)
    rc = ctx.lib.fcpp_patch_counts(ctx.handle, n, b.ptr('dims'), b.ptr('cell_offsets'), None, P.RES, b.ptr('labels'), b.ptr('region_offsets'), None, k,
                                   b.ptr('frame'), *rule, b.ptr('records'), nl, nw, b.ptr('bitmap'), b.ptr('line_counts'), b.ptr('line_offsets'),
                                   b.ptr('swath_offsets'), None)
    assert rc == 0, ctx.lib.fcpp_last_error()
    b.check({'bitmap': host['bitmap'], 'line_counts': host['line_counts'], 'line_offsets': host['line_offsets'], 'swath_offsets': host['swath_offsets']})

    c = Arena().input('dims', dims).input('region_offsets', roff).input('frame', host['frame'].reshape(-1)).input('records', host['records'].view(np.int64))
    c.input('bitmap', host['bitmap']).input('line_offsets', host['line_offsets'])
    for name in ('ax', 'ay', 'bx', 'by', 'length'):
        c.output(name, np.float64, ms)
    c.output('line', np.int32, ms).output('region', np.int64, ms)
    c.build(dev)
    rc = ctx.lib.fcpp_patch_fill(ctx.handle, n, c.ptr('dims'), P.RES, c.ptr('region_offsets'), None, k, c.ptr('frame'), *rule, c.ptr('records'), nl, nw,
                                 c.ptr('bitmap'), c.ptr('line_offsets'), ms, c.ptr('ax'), c.ptr('ay'), c.ptr('bx'), c.ptr('by'), c.ptr('line'),
                                 c.ptr('length'), c.ptr('region'))
    assert rc == 0, ctx.lib.fcpp_last_error()
    c.check({name: host[name] for name in P.SWATH_KEYS})
