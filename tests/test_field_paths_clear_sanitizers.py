"""The clear field-path rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_solve_clear_sanitizers.py): tests/native/field_paths_clear_sanitize_driver.cpp drives csrc/fcpp_fpathfn.h over
csrc/fcpp_solveclearfn.h -- the expressions fcpp_debug_field_paths_clear runs on the host and the kernels run on the device -- over fields of
0, 1 and 14 swaths, regions of 0, 3 and 257 edges, a NaN vertex, NaN poses, a bad order, both modes; any sanitizer report aborts the driver,
which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

KINDS = ('rank0', 'reshaped', 'blocked', 'outside', 'bad_region', 'ok_field', 'failed_field', 'empty_field')


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('field_paths_clear_sanitize_driver')


def test_clear_field_path_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, 240))
    print(out)
    # every kind of result occurred, in both modes
    for mode in (0, 1):
        for kind in KINDS:
            assert out[f'{kind}{mode}'] >= 5, (kind, mode, out)
    assert sum(out[f'{k}{mode}'] for k in KINDS[5:] for mode in (0, 1)) == 3 * 240
