"""The path-speed rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_patch_sanitizers.py):
tests/native/path_speeds_sanitize_driver.cpp drives csrc/fcpp_speedfn.h -- the parameter and sample checks, caps, stops and the host twin's
order of work behind fcpp_debug_path_speeds -- over fixed shapes (empty, one-sample, two-equal-sample paths, runs of zero steps, doubled
junctions and cusps, failing samples) under every flag word, and over random paths of random pieces, and checks every sample against a
brute-force O(n^2) minimum summed in long double.  Any sanitizer report aborts the driver, which is a stand-alone program: nothing is
loaded into python.  Sanitizers stay on host builds."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 400


@pytest.fixture(scope='module')
def driver():
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    out = os.path.join(REPO, 'build', 'path_speeds_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'path_speeds_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_path_speed_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', str(N)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    # 10 fixed paths under 8 flag words, 4 of them failing; N random paths, about one in ten failing
    assert out['paths'] == 80 + N and out['failed'] >= 32 + N // 20 and out['samples'] > 20000
    assert out['stops'] > 500 and out['at_cap'] > 2000 and out['zero_steps'] > 500
