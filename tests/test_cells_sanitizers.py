"""The field cell rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_patch_sanitizers.py):
tests/native/cells_sanitize_driver.cpp drives csrc/fcpp_cellfn.h -- the functions the kernels run, in the host's order of work behind
fcpp_debug_cells, on working arrays of their exact sizes -- over the named shapes of the host tests, fields of every status, a field at the
edge cap and seeded random stars with ponds at random cut angles, in both modes, and checks every result against the definition: the
count 1 + cuts - holes, the areas' sum and the partition of random points.  Any sanitizer report aborts the driver, which is a stand-alone
program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

N = 40


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('cells_sanitize_driver')


def test_cell_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, N))
    print(out)
    # 10 named shapes x 2 modes x 4 runs, 11 status fields x 2 modes, N random fields x 2 modes x 2 min_area
    assert out['fields'] >= 80 + 20 + 4 * N and out['cells'] > 5000 and out['cuts'] > 5000
