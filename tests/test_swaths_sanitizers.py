"""The polygon swath rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_rs_sanitizers.py):
tests/native/swath_sanitize_driver.cpp drives csrc/fcpp_swathfn.h -- the expressions fcpp_debug_swaths runs on the host and the kernels
run on the device -- with the comb, the L with its hole, a 300-vertex star, the comb over the crossing cap, a field with a NaN vertex and
one with a two-vertex ring, at random angles, widths and offsets; any sanitizer report aborts the driver.  Sanitizers stay on host builds."""
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
    out = os.path.join(REPO, 'build', 'swath_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'swath_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize('seed', [1, 2])
def test_swath_rule_clean_under_asan_ubsan(driver, seed):
    r = subprocess.run([driver, str(seed), '600'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    # every outcome occurred: cut fields, invalid ones, the comb over the cap
    assert words[0] == 'ok' and int(words[1]) > 300 and int(words[3]) >= 200 and int(words[5]) > 10 and int(words[7]) > 10000
