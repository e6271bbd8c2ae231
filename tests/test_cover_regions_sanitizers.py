"""The coverage-region rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_loop_transit_sanitizers.py): tests/native/cover_regions_sanitize_driver.cpp drives csrc/fcpp_regionfn.h -- the member, neighbour
and run functions the kernels run, and the per-field twin behind fcpp_debug_cover_regions -- over the shapes of the host tests, zero-sized
fields, grids one cell wide or high and random grids of garbage bytes, every named kind and random (mask, value) pairs, both
connectivities, and checks every result against a brute-force relabelling.  Any sanitizer report aborts the driver, which is a stand-alone
program: nothing is loaded into python.  Sanitizers stay on host builds."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 60


@pytest.fixture(scope='module')
def driver():
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    out = os.path.join(REPO, 'build', 'cover_regions_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'cover_regions_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_cover_region_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', str(N)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    # 15 fixed grids under 8 (kind, connectivity) pairs, N random grids under 10, 40 runs on every random grid
    assert out['fields'] == 15 * 8 + N * 10 and out['regions'] > 10000 and out['runs'] == 40 * N
