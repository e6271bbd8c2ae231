"""The clearance rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_route_sanitizers.py):
tests/native/clear_sanitize_driver.cpp drives csrc/fcpp_clearfn.h -- the expressions fcpp_debug_conn_clear / fcpp_debug_route_transit_clear
run on the host and the kernels run on the device -- over random fields (no ring, 3 edges, FCPP_CLEAR_EDGE_CHUNK - 1 / + 0 / + 1 edges, a
hole, a ring of 2 vertices, NaN vertices), both modes, unsolved paths, no region, a field index outside the list, and the transit blocks of
m = 0 .. 40 and 513 swaths; any sanitizer report aborts the driver, which is a stand-alone program: nothing is loaded into python.
Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('clear_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_clearance_rule_clean_under_asan_ubsan(driver, seed):
    out = word_counts(run_sanitized(driver, seed, 44))
    # every outcome occurred: paths without a region, unsolved, against a bad field, clear, crossed from inside, started outside; blocked and
    # free entries of the transit blocks; the field over the cap
    assert out['no_region'] >= 100 and out['unsolved'] >= 50 and out['bad_field'] >= 200 and out['clear'] >= 100 and out['crossed'] >= 100
    assert out['outside'] >= 20 and out['blocked'] >= 1000 and out['free'] >= 1000 and out['unsupported'] == 1
