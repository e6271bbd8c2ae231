"""The polygon swath rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_rs_sanitizers.py):
tests/native/swath_sanitize_driver.cpp drives csrc/fcpp_swathfn.h -- the expressions fcpp_debug_swaths runs on the host and the kernels
run on the device -- with the comb, the L with its hole, a 300-vertex star, the comb over the crossing cap, a field with a NaN vertex and
one with a two-vertex ring, at random angles, widths and offsets; any sanitizer report aborts the driver.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('swath_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_swath_rule_clean_under_asan_ubsan(driver, seed):
    words = run_sanitized(driver, seed, 600).split()
    # every outcome occurred: cut fields, invalid ones, the comb over the cap
    assert words[0] == 'ok' and int(words[1]) > 300 and int(words[3]) >= 200 and int(words[5]) > 10 and int(words[7]) > 10000
