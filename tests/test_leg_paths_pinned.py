"""The field paths and the headland paths pinned against a RECORDING (tests/golden/leg_paths_pinned.npz, written by
tools/record_leg_paths.py; the commit that produced it is stored in the file): what fcpp_debug_field_paths and fcpp_debug_headland_paths
returned before the two operators were given one fill kernel, one group kernel and one entry skeleton.  The other tests compare the device
with the host twin, and a change of both sides alike would pass them; this file holds still.

28 cases, a sizing call plus a filling call each.
  field paths (9): the batch of tests/test_field_paths_host.py's three cuts (the strips of 0, 1, 2, 3 and 5 swaths, the square with a
    hole, the L with its hole: 7 fields), Dubins and Reeds-Shepp, with and without entry / exit poses, at spacing 0.5 with the stored
    order (4); with poses and an explicit order (2); with poses at spacing 7 (2); and that file's three-field batch with a swath named
    twice in field 1 (1).  Planned at _chord_radius(R, spacing), as field_paths plans.
  headland paths (19): batch_rings(7) of tests/test_headland_paths_host.py under its eight CASES at spacing 0.5 and at 7 (16), the FAILED
    rings in both modes (2), a call without rings (1).
Per case the per-group and per-slot arrays are stored in full and compared as raw bytes (NaN totals count): the path offsets, the slot
offsets, the status, the totals, leg_word, leg_total (and leg_kind, which only the headland twin returns); leg_seg and the seven
per-sample columns as the SHA-256 of their bytes.  The GPU tests run the device entries on the same cases (tests/test_gpu_field_paths.py,
tests/test_gpu_headland_paths.py) against what the device returns of this: everything but leg_kind, leg_word, leg_total and leg_seg."""
import functools
import hashlib
import os

import numpy as np
import pytest

from field_coverage_path_planning_amd import engine as E
from tests.test_field_paths_host import ENTRY, EXIT, FIELD_CASES, SAMPLE_KEYS, host_paths, stored_order
from tests.test_guarded_host import strip
from tests.test_headland_paths_host import CASES, FAILED, R_BRIDGE, batch_rings, host_hpaths, raw_rings
from tests.test_route_host import HOLED_SQUARE, R, cut_with_angle
from tests.test_swaths_host import ELL, HOLE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'leg_paths_pinned.npz')
FIELD_FULL = ('offsets', 'leg_offsets', 'status', 'work', 'transit')                    # what the device entries return too
RING_FULL = ('offsets', 'leg_offsets', 'status', 'work', 'transit', 'skipped')
FIELD_HOST_FULL, RING_HOST_FULL = ('leg_word', 'leg_total'), ('leg_kind', 'leg_word', 'leg_total')
DIGESTS = SAMPLE_KEYS
HOST_DIGESTS = ('leg_seg',)
FIELD_NAMES = ['field/m%d-%s' % (mode, k) for mode in (0, 1) for k in ('open', 'ends', 'ends-order', 'ends-s7')] + ['field/failed']
RING_NAMES = (['ring/R%g-m%d-d%+d-s%g' % (c + (s,)) for s in (0.5, 7.0) for c in CASES] + ['ring/failed-m0', 'ring/failed-m1', 'ring/none'])


@functools.lru_cache(maxsize=None)
def field_batch():
    """the three cuts of tests/test_field_paths_host.py as ONE batch of 7 fields (each cut at its own width and angle)"""
    cuts = [cut_with_angle(f, a, W) for f, a, W in FIELD_CASES.values()]
    out = {k: np.ascontiguousarray(np.concatenate([c[k] for c in cuts])) for k in ('a', 'b', 'ax', 'ay', 'bx', 'by', 'line', 'length', 'angle')}
    sizes = np.concatenate([np.diff(c['offsets']) for c in cuts])
    out['offsets'] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert list(sizes) == [0, 1, 2, 3, 5, 14, int(cuts[2]['offsets'][1])]
    return out


@functools.lru_cache(maxsize=None)
def failed_field_batch():
    """tests/test_field_paths_host.py's three fields, swath 0 of field 1 named twice -> (cut, order)"""
    cut = cut_with_angle([HOLED_SQUARE, strip(3), [ELL, HOLE]], [0.0, 0.0, 0.3], 4.0)
    order = stored_order(cut['offsets'])
    s1 = int(cut['offsets'][1])
    order[s1 + 1] = order[s1] ^ 1
    return cut, order


def field_cases():
    """name -> (cut, dict(spacing, mode, order, entry, exit)); the radius of a case is _chord_radius(R, spacing)"""
    cut = field_batch()
    n = len(cut['offsets']) - 1
    entry, exit = np.tile(ENTRY, (n, 1)), np.tile(EXIT, (n, 1))
    out = {}
    for mode in (0, 1):
        out['field/m%d-open' % mode] = (cut, dict(spacing=0.5, mode=mode, order=None, entry=None, exit=None))
        out['field/m%d-ends' % mode] = (cut, dict(spacing=0.5, mode=mode, order=None, entry=entry, exit=exit))
        out['field/m%d-ends-order' % mode] = (cut, dict(spacing=0.5, mode=mode, order=stored_order(cut['offsets']), entry=entry, exit=exit))
        out['field/m%d-ends-s7' % mode] = (cut, dict(spacing=7.0, mode=mode, order=None, entry=entry, exit=exit))
    bad, order = failed_field_batch()
    out['field/failed'] = (bad, dict(spacing=0.5, mode=0, order=order, entry=np.tile(ENTRY, (3, 1)), exit=np.tile(EXIT, (3, 1))))
    assert sorted(out) == sorted(FIELD_NAMES) and len(out) == 9
    return out


def headland_cases():
    """name -> (ring set, dict(radius, mode, spacing, direction))"""
    out = {}
    for spacing in (0.5, 7.0):
        for radius, mode, direction in CASES:
            out['ring/R%g-m%d-d%+d-s%g' % (radius, mode, direction, spacing)] = (batch_rings(7), dict(radius=radius, mode=mode, spacing=spacing,
                                                                                                   direction=direction))
    for mode in (0, 1):
        out['ring/failed-m%d' % mode] = (raw_rings(FAILED), dict(radius=R_BRIDGE, mode=mode, spacing=0.5, direction=1))
    out['ring/none'] = (raw_rings([]), dict(radius=R_BRIDGE, mode=0, spacing=0.5, direction=1))
    assert sorted(out) == sorted(RING_NAMES) and len(out) == 19
    return out


def host_field_case(cut, kw):
    return host_paths(cut, E._chord_radius(R, kw['spacing']), kw['spacing'], kw['mode'], order=kw['order'], entry=kw['entry'], exit=kw['exit'])


def host_headland_case(rg, kw):
    return host_hpaths(rg, kw['radius'], kw['mode'], kw['spacing'], kw['direction'])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def recording(name, res, full, digests):
    """a case's share of the file"""
    out = {'%s/%s' % (name, k): np.ascontiguousarray(res[k]) for k in full}
    out['%s/sha256' % name] = np.array(['%s=%s' % (k, digest(res[k])) for k in digests])
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def assert_pinned(name, res, full, digests):
    """res[k] holds the recorded bytes for every k of `full`, the recorded digest for every k of `digests`"""
    g = golden()
    for k in full:
        want, got = g['%s/%s' % (name, k)], np.ascontiguousarray(res[k])
        assert got.dtype == want.dtype and got.shape == want.shape, (name, k)
        assert np.array_equal(got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)), (name, k)
    sha = dict(s.split('=') for s in g['%s/sha256' % name].tolist())
    for k in digests:
        assert digest(res[k]) == sha[k], (name, k)


def test_the_recording_holds_every_case():
    g = golden()
    names = {k.rsplit('/', 1)[0] for k in g if k != 'commit'}
    assert names == set(FIELD_NAMES) | set(RING_NAMES) and len(names) == 28
    assert len(str(g['commit'])) == 40


@pytest.mark.parametrize('name', FIELD_NAMES)
def test_host_field_paths_are_the_recorded_ones(name):
    cut, kw = field_cases()[name]
    res = host_field_case(cut, kw)
    assert res['total'] > 100 and (name != 'field/failed' or res['status'].tolist() == [0, -1, 0])
    assert_pinned(name, res, FIELD_FULL + FIELD_HOST_FULL, DIGESTS + HOST_DIGESTS)


@pytest.mark.parametrize('name', RING_NAMES)
def test_host_headland_paths_are_the_recorded_ones(name):
    rg, kw = headland_cases()[name]
    res = host_headland_case(rg, kw)
    assert res['total'] > 100 or name == 'ring/none'
    assert_pinned(name, res, RING_FULL + RING_HOST_FULL, DIGESTS + HOST_DIGESTS)
