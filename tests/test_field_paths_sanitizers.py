"""The field-path rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_route_sanitizers.py):
tests/native/field_paths_sanitize_driver.cpp drives csrc/fcpp_fpathfn.h -- the expressions fcpp_debug_field_paths runs on the host and the
kernels run on the device -- over random swath sets: m = 0 .. 40, both modes, with and without an order, an entry and an exit pose, some
with a poisoned order or a NaN, negative or infinite length; every array has its exact size.  Any sanitizer report aborts the driver,
which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('field_paths_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_field_path_rule_clean_under_asan_ubsan(driver, seed):
    out = word_counts(run_sanitized(driver, seed, 140))
    # every outcome occurred: fields with paths, failed ones of both kinds, empty ones, every combination's ingredients, reversing cusps
    assert out['ok'] >= 100 and out['invalid'] >= 10 and out['bad_order'] >= 3 and out['bad_length'] >= 3 and out['empty'] >= 1
    assert out['ordered'] >= 50 and out['entry'] >= 40 and out['exit'] >= 40 and out['reversing'] >= 40
    assert out['samples'] > 100000 and out['cusps'] > 100
