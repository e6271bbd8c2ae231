"""The loop-transit rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_solve_clear_sanitizers.py): tests/native/loop_transit_sanitize_driver.cpp drives csrc/fcpp_transitfn.h -- the expressions
fcpp_debug_loop_transits runs on the host and the kernels run on the device -- over loops of 1, 7, 64, 200 and more samples than the station
cap, fields without loops or stations, a NaN vertex, a NaN arc length, NaN poses and field indices outside the list, both modes; it picks
every pair twice (the twin's pick, and a second look at every candidate) and samples every found transit.  Any sanitizer report aborts
the driver, which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

N = 360


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('loop_transit_sanitize_driver')


def test_loop_transit_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, N))
    print(out)
    for mode in (0, 1):
        for kind in ('einval', 'cap', 'none', 'via'):
            assert out[f'{kind}{mode}'] >= 1, (kind, mode, out)
        assert out[f'ride{mode}'] + out[f'wrap{mode}'] >= 1, out
    assert sum(out.values()) == N
