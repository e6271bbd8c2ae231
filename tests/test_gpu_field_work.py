"""k_plan_sparse_fields (a workgroup plans the wave tiles of a field and reduces the field) against the path it replaced for such fields
(k_plan_sparse + k_reduce_stats): the points must be identical bit for bit -- the same tile function plans them --, the statistics equal
up to the order of their sums, the counts exactly; a second step into the same arrays gives the same (the flag counts the streaming
kernels leave in the runs' slots are reset by whoever reduces).  The switch (FCPP_FIELD_WORK=0: the replaced path) is read when a batch is
created and is the host tiler's: both batches are set up by the host."""
import numpy as np
import pytest
import torch

from field_coverage_path_planning_amd import engine as E
from tests import test_gpu_parity as T

pytestmark = pytest.mark.gpu


def _plan(specs, field_work, monkeypatch):
    """-> ([two steps' outputs into the same arrays], reduction classes) of the batch planned under FCPP_FIELD_WORK=field_work"""
    monkeypatch.setenv('FCPP_FIELD_WORK', field_work)
    b = E.Batch(specs, E.make_vehicle(), E.make_options())
    bufs = b.alloc()
    steps = []
    for _ in range(2):
        rr = b.run(bufs)
        torch.cuda.synchronize()
        steps.append({'x': rr.x.cpu().numpy(), 'y': rr.y.cpu().numpy(), 'k': rr.kappa.cpu().numpy(), 'v': rr.v.cpu().numpy(),
                      'f': rr.flagseg.cpu().numpy(), 's': rr.stats_raw.cpu().numpy()})
    classes = np.array(b.reduce_classes(), dtype=np.int64)
    b.close()
    return steps, classes


def test_field_work_equals_open_path(monkeypatch):
    rng = np.random.default_rng(77)
    specs = [E.FieldSpec(field_length=float(a), field_width=float(b)) for a, b in rng.uniform(90.0, 700.0, size=(300, 2))]
    more, _ = T._random_fields(4242, 60, para=True, with_obstacles=True)       # skewed fields (points outside), obstacles
    specs += more
    ctx = E.get_context()
    ctx.set_setup('host')
    try:
        work, work_classes = _plan(specs, '1', monkeypatch)
        opened, open_classes = _plan(specs, '0', monkeypatch)
    finally:
        ctx.set_setup('auto')
    # the default sends most of these fields to k_plan_sparse_fields, the switch none
    assert work_classes.sum() < open_classes.sum() and open_classes.sum() == 360
    for steps in (work, opened):
        for k in 'xykvfs':
            assert np.array_equal(steps[0][k], steps[1][k]), k          # a re-run is bit-identical
    for k in 'xykvf':
        assert np.array_equal(work[0][k], opened[0][k]), k
    sw, so = work[0]['s'], opened[0]['s']                  # (n_fields, 13) int64 words: nine doubles, four counters
    assert np.array_equal(sw[:, 9:], so[:, 9:])
    assert int(so[:, 10].sum()) > 0                        # some skewed field does leave its polygon: the flag counts are exercised
    fw, fo = sw[:, :9].view(np.float64), so[:, :9].view(np.float64)
    np.testing.assert_allclose(fw[:, :6], fo[:, :6], rtol=1e-13, atol=0.0)
    assert np.array_equal(fw[:, 6:], fo[:, 6:])            # maxima do not depend on the order
