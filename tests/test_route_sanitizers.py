"""The swath router's rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_swaths_sanitizers.py):
tests/native/route_sanitize_driver.cpp drives csrc/fcpp_routefn.h -- the expressions fcpp_debug_route runs on the host and the kernels run
on the device -- over random transit blocks, bit-symmetric under (p, q) <-> (q ^ 1, p ^ 1) with an infinite same-swath diagonal: m = 0 .. 40
and both sides of the cap (512, 513), 1 .. 64 candidates, with and without E / X, some with NaN or infinite entries; any sanitizer report
aborts the driver, which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('route_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_route_rule_clean_under_asan_ubsan(driver, seed):
    out = word_counts(run_sanitized(driver, seed, 60))
    # every outcome occurred: routed fields, some of them improved, invalid ones, the field over the cap, poisoned blocks, applied moves
    assert out['ok'] >= 30 and out['improved'] >= 20 and out['invalid'] >= 1 and out['unsupported'] == 1 and out['poisoned'] >= 5
    assert out['moves'] > 100
