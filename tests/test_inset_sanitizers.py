"""The polygon inset rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_swaths_sanitizers.py):
tests/native/inset_sanitize_driver.cpp drives csrc/fcpp_insetfn.h -- the expressions fcpp_debug_inset runs on the host and the kernels run
on the device -- with the hand-made shapes, a 300-vertex star, a field of 1025 edges, a field with a NaN vertex and one with a two-vertex
ring, at random distances (some of which empty the field) and arc steps; any sanitizer report aborts the driver.  Sanitizers stay on host
builds: nothing loaded into Python runs under one."""
import pytest

from tests.support import run_sanitized, sanitize_driver


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('inset_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_inset_rule_clean_under_asan_ubsan(driver, seed):
    words = run_sanitized(driver, seed, 180).split()
    # every outcome occurred: insets with rings, empty ones, invalid fields, the field over the edge cap; straights and arcs
    assert words[0] == 'ok' and int(words[1]) >= 60 and int(words[3]) >= 20 and int(words[5]) >= 40 and int(words[7]) >= 20
    assert int(words[9]) > int(words[1]) and int(words[11]) > 5000 and int(words[13]) > 1000
