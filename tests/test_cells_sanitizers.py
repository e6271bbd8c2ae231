"""The field cell rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_patch_sanitizers.py):
tests/native/cells_sanitize_driver.cpp drives csrc/fcpp_cellfn.h -- the functions the kernels run, in the host's order of work behind
fcpp_debug_cells, on working arrays of their exact sizes -- over the named shapes of the host tests, fields of every status, a field at the
edge cap and seeded random stars with ponds at random cut angles, in both modes, and checks every result against the definition: the
count 1 + cuts - holes, the areas' sum and the partition of random points.  Any sanitizer report aborts the driver, which is a stand-alone
program: nothing is loaded into python.  Sanitizers stay on host builds."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 40


@pytest.fixture(scope='module')
def driver():
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    out = os.path.join(REPO, 'build', 'cells_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'cells_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_cell_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', str(N)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    # 10 named shapes x 2 modes x 4 runs, 11 status fields x 2 modes, N random fields x 2 modes x 2 min_area
    assert out['fields'] >= 80 + 20 + 4 * N and out['cells'] > 5000 and out['cuts'] > 5000
