"""The vehicle shares' rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_trips_sanitizers.py):
tests/native/fleet_driver.cpp drives csrc/fcpp_fleetfn.h -- the tables, both stages, the pick, the backtrack, the very functions the kernel
runs -- over random fields of 0 to 10 swaths and fields of 17 to 513 (both sides of the cap), 1 to 64 candidates, both directions and one,
K from 0 to 17, rows of the per-share outputs as short as K, whole-number tables (ties), and every way a field can be invalid, and checks
the result against every composition into at most K shares where a field is small.  Any sanitizer report aborts the driver, which is a
stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

N = 400


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('fleet_driver')


def test_fleet_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, N))
    print(out)
    # every kind of result occurred, the cap was met from above once, and most fields were small enough for the brute force
    assert out['ok'] > 250 and out['invalid'] > 20 and out['unsupported'] > 5 and out['empty'] > 0, out
    assert out['brute'] > 250 and out['backwards'] > 20 and out['fewer'] > 20, out
