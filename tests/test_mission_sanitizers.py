"""The mission-path rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_patch_sanitizers.py):
tests/native/mission_sanitize_driver.cpp drives csrc/fcpp_missionfn.h -- the station list, the layers, the finish, the slot counts and
mission_eval, the very functions the kernels run -- over random fields of random items (loops of 0 to 40 samples, loops without a station,
lines, empty paths, NaN poses, a loop beyond the station limit), with and without entry and exit, in both modes, and checks the chosen
stations against every combination of stations where there are few.  Any sanitizer report aborts the driver, which is a stand-alone
program: nothing is loaded into python.  Sanitizers stay on host builds."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 600


@pytest.fixture(scope='module')
def driver():
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    out = os.path.join(REPO, 'build', 'mission_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'mission_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_mission_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', str(N)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    # every kind of result occurred in both modes, and most fields were small enough for the brute-force comparison
    for m in '01':
        assert out['ok' + m] > 100 and out['einval' + m] > 0 and out['cap' + m] > 0 and out['empty' + m] > 0 and out['brute' + m] > 100, out
    assert out['samples'] > 10000
