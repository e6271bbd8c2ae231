"""The patch-pass rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_cover_regions_sanitizers.py): tests/native/patch_sanitize_driver.cpp drives csrc/fcpp_patchfn.h -- the key, layout, line, bin
and run functions the kernels run, and the host's order of work behind fcpp_debug_patch_swaths -- over the fixed shapes of the host tests,
zero-sized fields, labels of -2, a label that never occurs and random label grids at random angles, widths, margins and joins, and checks
every result against a brute-force pass.  Any sanitizer report aborts the driver, which is a stand-alone program: nothing is loaded into
python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts

N = 60


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('patch_sanitize_driver')


def test_patch_rule_clean_under_asan_ubsan(driver):
    out = word_counts(run_sanitized(driver, 1, N))
    print(out)
    # 14 fixed fields under 16 (angle, join, margin) triples, in one batch and alone; N random batches of 1 .. 4 fields
    assert out['fields'] >= 14 * 16 * 2 + N and out['regions'] > 10000 and out['swaths'] > 10000
