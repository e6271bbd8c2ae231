"""The coverage-region rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_loop_transit_sanitizers.py): tests/native/cover_regions_sanitize_driver.cpp drives csrc/fcpp_regionfn.h -- the member, neighbour
and run functions the kernels run, and the per-field twin behind fcpp_debug_cover_regions -- over the shapes of the host tests, zero-sized
fields, grids one cell wide or high and random grids of garbage bytes, every named kind and random (mask, value) pairs, both
connectivities, and checks every result against a brute-force relabelling.  Any sanitizer report aborts the driver, which is a stand-alone
program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

N = 60


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('cover_regions_sanitize_driver')


def test_cover_region_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, N))
    print(out)
    # 15 fixed grids under 8 (kind, connectivity) pairs, N random grids under 10, 40 runs on every random grid
    assert out['fields'] == 15 * 8 + N * 10 and out['regions'] > 10000 and out['runs'] == 40 * N
