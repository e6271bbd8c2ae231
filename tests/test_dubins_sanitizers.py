"""The Dubins solver under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_host_sanitizers.py, whose
driver is left as it is): tests/native/dubins_sanitize_driver.cpp drives csrc/fcpp_dubinsfn.h -- the function fcpp_debug_dubins runs on
the host and the kernels run on the device -- with random, degenerate and hostile pairs; any sanitizer report aborts the driver."""
import pytest

from tests.support import run_sanitized, sanitize_driver


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('dubins_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_dubins_function_clean_under_asan_ubsan(driver, seed):
    words = run_sanitized(driver, seed, 200000).split()
    assert words[0] == 'solved' and int(words[1]) > 100000 and int(words[3]) > 1000      # both outcomes exercised
