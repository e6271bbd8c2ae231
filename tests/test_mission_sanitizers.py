"""The mission-path rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_patch_sanitizers.py):
tests/native/mission_sanitize_driver.cpp drives csrc/fcpp_missionfn.h -- the station list, the layers, the finish, the slot counts and
mission_eval, the very functions the kernels run -- over random fields of random items (loops of 0 to 40 samples, loops without a station,
lines, empty paths, NaN poses, a loop beyond the station limit), with and without entry and exit, in both modes, and checks the chosen
stations against every combination of stations where there are few.  Any sanitizer report aborts the driver, which is a stand-alone
program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

N = 600


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('mission_sanitize_driver')


def test_mission_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, N))
    print(out)
    # every kind of result occurred in both modes, and most fields were small enough for the brute-force comparison
    for m in '01':
        assert out['ok' + m] > 100 and out['einval' + m] > 0 and out['cap' + m] > 0 and out['empty' + m] > 0 and out['brute' + m] > 100, out
    assert out['samples'] > 10000
