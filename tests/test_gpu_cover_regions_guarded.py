"""fcpp_cover_regions_counts and fcpp_cover_regions_fill on guarded buffers (tests/guarded.py): every output element is written and nothing
beside it, the inputs keep their bits, every pointer is only naturally aligned (the 48-byte records and the 32-byte dims at 8 mod 16, the
labels at 4 mod 8, the grid at an odd address), the optional host copies are NULL.  Once, at the second-round sizes: more tiles than one
launch of the seam kernel covers, more numbering blocks than one round of the scan, 3 x 3 tiles with last tiles 2 cells wide, blocks of
roots only, an empty field and a field of one cell between them.  The expected values are the host twin's."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import engine as E
from tests import cover_region_cases as C
from tests.guarded import Arena

pytestmark = pytest.mark.gpu


def test_counts_and_fill_on_guarded_buffers():
    import torch
    ctx = E.get_context(None)
    dev = torch.device('cuda', ctx.device)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    rng = np.random.default_rng(4)
    ii = np.arange(130)
    grids = [C.members((130, 130), (ii[:, None] + ii[None, :]) % 2 == 0), np.zeros((0, 0), np.uint8), C.members((1, 1), np.ones((1, 1), bool))]
    grids += C.seam_batch(n_cu)
    grids.append(rng.integers(0, 8, (70, 131), dtype=np.uint8))
    dims, off, flat = C.pack(grids)
    n, total = len(grids), len(flat)
    assert C.tiles_of(grids) > C.seam_round_tiles(n_cu) and C.blocks_of(grids) > 256
    connectivity = 8
    host = C.twin(grids, 3, 1, connectivity)
    k = int(host['offsets'][-1])

    a = Arena().input('dims', dims).input('cell_offsets', off).input('grid', flat)
    a.output('labels', np.int32, total).output('region_offsets', np.int64, n + 1)
    a.build(dev)
    ctx.bind_stream()
    rc = ctx.lib.fcpp_cover_regions_counts(ctx.handle, n, a.ptr('dims'), a.ptr('cell_offsets'), None, a.ptr('grid'), 3, 1, connectivity, a.ptr('labels'),
                                           a.ptr('region_offsets'), None)
    assert rc == 0, ctx.lib.fcpp_last_error()
    a.check({'labels': host['keys'], 'region_offsets': host['offsets']})

    b = Arena().input('dims', dims).input('cell_offsets', off).input('region_offsets', host['offsets']).inout('labels', host['keys'])
    b.output('records', np.int64, 6 * k)
    b.build(dev)
    rc = ctx.lib.fcpp_cover_regions_fill(ctx.handle, n, b.ptr('dims'), b.ptr('cell_offsets'), None, b.ptr('labels'), b.ptr('region_offsets'), None, k,
                                         b.ptr('records'))
    assert rc == 0, ctx.lib.fcpp_last_error()
    b.check({'labels': host['index'], 'records': host['records'].view(np.int64)})
