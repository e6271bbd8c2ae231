"""The cell tour's rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_mission_sanitizers.py):
tests/native/tour_sanitize_driver.cpp drives csrc/fcpp_tourfn.h -- the joint block, the layers, the candidates, the sweeps, the pick, the
very functions the kernels run -- over random fields of 0 to 7 cells of 0 to 4 variants in both modes, with and without gates and stored
nodes, NaN poses, stored nodes outside their cell, and both sides of each of the three caps, and checks the result against every order and
every node combination where a field is small.  Any sanitizer report aborts the driver, which is a stand-alone program: nothing is loaded
into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

N = 400


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('tour_sanitize_driver')


def test_tour_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, N))
    print(out)
    # every kind of result occurred, the three caps were met from above, and many fields were small enough for the brute force
    assert out['ok'] > 200 and out['invalid'] > 0 and out['unsupported'] == 3 and out['empty'] > 0 and out['improved'] > 50, out
    assert out['brute'] > 50 and out['optimal'] > 0 and out['moves'] > 50 and out['solved'] > 10000, out
