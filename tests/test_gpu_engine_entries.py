"""The library entries plan_polygon_fields calls, in order, on the GPU (run with -m gpu on an MI355X): once with every option of the chain
on, once with every option off.  engine's docstrings promise of each option "nothing changes, down to the entries called" without it; this
pins that for the whole chain at once, and pins the chain's calls themselves against a change of the binding layer.  The two lists were
recorded at the commit before the binding layer was rebuilt on PathSet and the CSR toolkit: what is listed is every LOOK-UP of an entry on
the context's library handle, so an entry handed to a helper before the one called first is listed first (fcpp_field_path_fill_clear)."""
import numpy as np
import pytest

from field_coverage_path_planning_amd import engine as E
from tests.test_route_host import HOLED_SQUARE

pytestmark = pytest.mark.gpu

FIELDS = [HOLED_SQUARE, [(60, 0), (100, 0), (100, 40), (60, 40)]]
ENTRY = np.array([[-5.0, -5.0, 0.0], [55.0, -5.0, 0.0]])
EXIT = np.array([[45.0, 45.0, np.pi], [105.0, 45.0, np.pi]])

HEAD = ['fcpp_inset_counts', 'fcpp_inset_fill', 'fcpp_inset_counts', 'fcpp_inset_fill',                    # headland(): the passes, the work area
        'fcpp_swath_scores', 'fcpp_swath_counts', 'fcpp_swath_fill']                                        # best_swath_angle, polygon_swaths

BARE = HEAD + ['fcpp_route_transit', 'fcpp_route_solve',                                                    # route_swaths
               'fcpp_field_path_counts', 'fcpp_field_path_fill']                                            # field_paths

FULL = HEAD + [
    'fcpp_rs_solve', 'fcpp_conn_solve_clear', 'fcpp_rs_solve', 'fcpp_conn_solve_clear',                     # route_swaths: entry and exit connectors, priced
    'fcpp_route_transit_priced', 'fcpp_route_solve',
    'fcpp_rs_solve', 'fcpp_conn_clear', 'fcpp_rs_solve', 'fcpp_conn_clear',                                 # the legs as routed and as stored, tested
    'fcpp_rs_solve', 'fcpp_conn_solve_clear',                                                               # the legs' clear words
    'fcpp_headland_path_counts', 'fcpp_headland_path_fill', 'fcpp_headland_path_counts', 'fcpp_headland_path_fill',       # the loops, both ways round
    'fcpp_field_path_fill_clear', 'fcpp_field_path_counts_clear',                                           # field_paths(clear_of=...)
    'fcpp_trajectory', 'fcpp_trajectory', 'fcpp_loop_transit_solve', 'fcpp_loop_transit_counts', 'fcpp_loop_transit_fill',  # the detour
    'fcpp_polygon_cover_sizes', 'fcpp_polygon_cover', 'fcpp_cover_regions_counts', 'fcpp_cover_regions_fill',
    'fcpp_patch_sizes', 'fcpp_patch_counts', 'fcpp_patch_fill',
    'fcpp_route_transit', 'fcpp_route_solve', 'fcpp_field_path_counts', 'fcpp_field_path_fill',             # the patch passes routed and driven
    'fcpp_polygon_cover_sizes', 'fcpp_polygon_cover',                                                       # coverage_after
    'fcpp_mission_solve', 'fcpp_mission_counts', 'fcpp_mission_fill', 'fcpp_rs_solve', 'fcpp_conn_solve_clear',         # the mission, its joints tested
    'fcpp_path_speeds']


class _Recorder:
    """stands in for the context's library handle: notes the name of every entry looked up on it"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def _entries(**options):
    ctx = E.get_context()
    ctx.bind_stream()                  # (so that no call below has a stream to hand to the library first)
    lib = ctx.lib
    ctx.lib = rec = _Recorder(lib)
    try:
        plan = E.plan_polygon_fields(FIELDS, 4.0, 3.0, 0.5, [0.0], **options)
    finally:
        ctx.lib = lib
    return rec.names, plan


def test_every_option_on():
    names, plan = _entries(passes=1, reversing=True, headland_paths=True, clear_of='boundary', reshape=True, price_clear=True, detour=True,
                           coverage_resolution=0.5, missed_min_area=1.0, patch=True, mission='headland_first', speeds=E.make_vehicle(),
                           entry=ENTRY, exit=EXIT)
    assert names == FULL
    assert plan.mission.status.tolist() == [0, 0] and plan.speeds.status.tolist() == [0, 0] and plan.paths.status.tolist() == [0, 0]
    assert int(plan.mission.x.numel()) == int(plan.speeds.v.numel()) > 0 and plan.coverage_after is not None and plan.transits is plan.paths.transits


def test_every_option_off():
    names, plan = _entries()
    assert names == BARE
    assert plan.paths.status.tolist() == [0, 0] and int(plan.paths.x.numel()) > 0
    assert all(getattr(plan, k) is None for k in ('headland_paths', 'coverage', 'clearance', 'transits', 'missed', 'patch', 'patch_info', 'patch_paths',
                                                  'coverage_after', 'mission', 'speeds'))
