"""The headland-path rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_field_paths_sanitizers.py):
tests/native/headland_paths_sanitize_driver.cpp drives csrc/fcpp_hpathfn.h -- the expressions fcpp_debug_headland_paths runs on the host and
the kernels run on the device -- over the rings csrc/fcpp_insetfn.h cuts from the inset driver's shapes at the distances 2, 6, 8, 60 and
random ones, and over hand-made rings (arcs only, a NaN vertex, one vertex, none, a negative src, an arc of radius 0, an infinite
distance): both modes, both directions, R = 1.5, 6 and random, spacing 0.5 and 7; every array has its exact size.  Any sanitizer report
aborts the driver, which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('headland_paths_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_headland_path_rule_clean_under_asan_ubsan(driver, seed):
    out = word_counts(run_sanitized(driver, seed, 140))
    # every outcome occurred: closed loops, empty insets, failed rings of both kinds, every kind of leg, both directions and modes
    assert out['ok'] >= 150 and out['empty'] >= 20 and out['invalid'] >= 40 and out['unsupported'] >= 8
    assert out['straight'] >= 1000 and out['followed'] >= 300 and out['skipped'] >= 100 and out['connectors'] >= 1000 and out['smooth'] >= 300
    assert out['reversed'] >= 50 and out['reversing'] >= 50 and out['samples'] > 50000 and out['cusps'] > 500
