"""The priced transit block's rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_solve_clear_sanitizers.py): tests/native/route_priced_sanitize_driver.cpp drives priced_transit of csrc/fcpp_solveclearfn.h --
the expressions fcpp_debug_route_transit_priced runs on the host and the kernels run on the device -- over random fields of swaths and
random regions in both modes: fields of 0 and 1 swaths, ponds over swath ends, regions without a ring and with a NaN vertex, penalty 0.
Any sanitizer report aborts the driver, which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

KINDS = ('own', 'clear', 'rescued', 'blocked', 'outside', 'bad_field')


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('route_priced_sanitize_driver')


def test_priced_transit_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, 140))
    print(out)
    # every kind of entry occurred, in both modes
    for mode in (0, 1):
        for kind in KINDS:
            assert out[f'{kind}{mode}'] >= 5, (kind, mode, out)
