"""The cell tour's rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_mission_sanitizers.py):
tests/native/tour_sanitize_driver.cpp drives csrc/fcpp_tourfn.h -- the joint block, the layers, the candidates, the sweeps, the pick, the
very functions the kernels run -- over random fields of 0 to 7 cells of 0 to 4 variants in both modes, with and without gates and stored
nodes, NaN poses, stored nodes outside their cell, and both sides of each of the three caps, and checks the result against every order and
every node combination where a field is small.  Any sanitizer report aborts the driver, which is a stand-alone program: nothing is loaded
into python.  Sanitizers stay on host builds."""
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
    out = os.path.join(REPO, 'build', 'tour_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'tour_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_tour_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', str(N)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    # every kind of result occurred, the three caps were met from above, and many fields were small enough for the brute force
    assert out['ok'] > 200 and out['invalid'] > 0 and out['unsupported'] == 3 and out['empty'] > 0 and out['improved'] > 50, out
    assert out['brute'] > 50 and out['optimal'] > 0 and out['moves'] > 50 and out['solved'] > 10000, out
