"""The Reeds-Shepp solver under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_dubins_sanitizers.py):
tests/native/rs_sanitize_driver.cpp drives csrc/fcpp_rsfn.h -- the function fcpp_debug_rs runs on the host and the kernels run on the
device -- with random, degenerate and hostile pairs, through the solve, the gear runs and the pose along them; any sanitizer report aborts
the driver.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('rs_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_rs_function_clean_under_asan_ubsan(driver, seed):
    words = run_sanitized(driver, seed, 200000).split()
    assert words[0] == 'solved' and int(words[1]) > 100000 and int(words[3]) > 1000 and int(words[7]) > 10000      # both outcomes, and cusps
