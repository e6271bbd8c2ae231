"""The path-speed rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_patch_sanitizers.py):
tests/native/path_speeds_sanitize_driver.cpp drives csrc/fcpp_speedfn.h -- the parameter and sample checks, caps, stops and the host twin's
order of work behind fcpp_debug_path_speeds -- over fixed shapes (empty, one-sample, two-equal-sample paths, runs of zero steps, doubled
junctions and cusps, failing samples) under every flag word, and over random paths of random pieces, and checks every sample against a
brute-force O(n^2) minimum summed in long double.  Any sanitizer report aborts the driver, which is a stand-alone program: nothing is
loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

N = 400


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('path_speeds_sanitize_driver')


def test_path_speed_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, N))
    print(out)
    # 10 fixed paths under 8 flag words, 4 of them failing; N random paths, about one in ten failing
    assert out['paths'] == 80 + N and out['failed'] >= 32 + N // 20 and out['samples'] > 20000
    assert out['stops'] > 500 and out['at_cap'] > 2000 and out['zero_steps'] > 500
