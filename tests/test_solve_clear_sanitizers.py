"""The clear-connector rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_clearance_sanitizers.py): tests/native/solve_clear_sanitize_driver.cpp drives csrc/fcpp_solveclearfn.h -- the expressions
fcpp_debug_conn_solve_clear runs on the host and the kernels run on the device -- over fields of 0, 3, 255, 256 and 257 edges, a hole, a
NaN vertex, both modes, NaN poses, no region and field indices outside the list; any sanitizer report aborts the driver, which is a
stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

KINDS = ('unsolved', 'no_region', 'bad_field', 'rank0', 'rescued', 'outside', 'blocked')


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('solve_clear_sanitize_driver')


def test_clear_connector_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, 6000))
    print(out)
    # every kind of result occurred, in both modes
    for mode in (0, 1):
        for kind in KINDS:
            assert out[f'{kind}{mode}'] >= 5, (kind, mode, out)
    assert sum(out.values()) == 6000
