"""The polygon inset rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_swaths_sanitizers.py):
tests/native/inset_sanitize_driver.cpp drives csrc/fcpp_insetfn.h -- the expressions fcpp_debug_inset runs on the host and the kernels run
on the device -- with the hand-made shapes, a 300-vertex star, a field of 1025 edges, a field with a NaN vertex and one with a two-vertex
ring, at random distances (some of which empty the field) and arc steps; any sanitizer report aborts the driver.  Sanitizers stay on host
builds: nothing loaded into Python runs under one."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def driver():
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    out = os.path.join(REPO, 'build', 'inset_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'inset_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize('seed', [1, 2])
def test_inset_rule_clean_under_asan_ubsan(driver, seed):
    r = subprocess.run([driver, str(seed), '180'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    # every outcome occurred: insets with rings, empty ones, invalid fields, the field over the edge cap; straights and arcs
    assert words[0] == 'ok' and int(words[1]) >= 60 and int(words[3]) >= 20 and int(words[5]) >= 40 and int(words[7]) >= 20
    assert int(words[9]) > int(words[1]) and int(words[11]) > 5000 and int(words[13]) > 1000
