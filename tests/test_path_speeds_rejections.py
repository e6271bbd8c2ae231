"""The argument checks of fcpp_path_speeds itself (run with -m gpu on an MI355X; tiny): every case is a call the glue refuses ON THE HOST,
before any kernel launch -- the status it returns, and that the outputs keep what they held.  The same checks of the host twin run
without a device in tests/test_path_speeds_host.py."""
import ctypes as C

import numpy as np
import pytest

from field_coverage_path_planning_amd import _lib as L
from field_coverage_path_planning_amd import engine as E
from tests import path_speed_cases as S

pytestmark = pytest.mark.gpu


def test_refused_on_the_host():
    import torch
    ctx = E.get_context(None)
    ctx.bind_stream()
    dev = torch.device('cuda', ctx.device)
    ps = S.pack([S.straight_arc_straight(20, 9, 11), S.reeds_shepp_like(7, 5, 9)])
    total, n = len(ps['x']), len(ps['offsets']) - 1
    t = {k: torch.as_tensor(ps[k], device=dev) for k in ('offsets', 'x', 'y', 'kappa', 'part', 'gear')}
    v, cap = torch.full((total,), 7.0, dtype=torch.float64, device=dev), torch.full((total,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((n,), 99, dtype=torch.int32, device=dev)

    def call(prm=S.params(), handle=ctx.handle, n_paths=n, total=total, host=None, **null):
        ptr = lambda k, a: None if k in null else a.data_ptr()
        return ctx.lib.fcpp_path_speeds(handle, C.byref(prm) if prm is not None else None, n_paths, ptr('offsets', t['offsets']), total,
                                        *[ptr(k, t[k]) for k in ('x', 'y', 'kappa', 'part', 'gear')], ptr('v', v), ptr('cap', cap),
                                        ptr('status', status), None if host is None else host.ctypes.data)

    assert call(handle=None) == L.EINVAL and b'context' in ctx.lib.fcpp_last_error()
    assert call(prm=None) == L.EINVAL
    for k in ('x', 'y', 'kappa', 'part', 'gear', 'status'):
        assert call(**{k: None}) == L.EINVAL, k
    assert call(offsets=None) == L.EINVAL                                      # neither the device table nor a host copy
    for kw in (dict(a_acc=0.0), dict(a_dec=np.nan), dict(a_lat=np.inf), dict(reverse_kmh=-2.5), dict(turn_kmh=0.0), dict(safety_factor=0.0),
               dict(kappa_eps=0.0), dict(flags=16), dict(nominal=[np.nan] * 8), dict(nominal=[-1.0] * 8)):
        assert call(prm=S.params(**kw)) == L.EINVAL, kw
        assert b'positive and finite' in ctx.lib.fcpp_last_error()
    assert call(n_paths=-1) == L.ESIZE and call(total=-1) == L.ESIZE
    assert call(total=total - 1) == L.ESIZE and b'offsets' in ctx.lib.fcpp_last_error()          # read back from the device
    off = ps['offsets']
    for bad in (off + 1, np.array([0, off[1] + 50, off[1], off[2]])[[0, 1, 3]], np.array([0, total + 1, total])):
        assert call(host=np.ascontiguousarray(bad, dtype=np.int64)) == L.ESIZE
    torch.cuda.synchronize()
    assert bool((v == 7.0).all()) and bool((cap == 7.0).all()) and bool((status == 99).all())          # nothing was launched
    # and the call itself, with the host copy alone and both outputs NULL: only the status is written
    assert call(offsets=None, host=off, v=None, cap=None) == L.OK
    assert status.tolist() == [0, 0] and bool((v == 7.0).all())
