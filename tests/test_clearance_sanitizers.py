"""The clearance rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_route_sanitizers.py):
tests/native/clear_sanitize_driver.cpp drives csrc/fcpp_clearfn.h -- the expressions fcpp_debug_conn_clear / fcpp_debug_route_transit_clear
run on the host and the kernels run on the device -- over random fields (no ring, 3 edges, FCPP_CLEAR_EDGE_CHUNK - 1 / + 0 / + 1 edges, a
hole, a ring of 2 vertices, NaN vertices), both modes, unsolved paths, no region, a field index outside the list, and the transit blocks of
m = 0 .. 40 and 513 swaths; any sanitizer report aborts the driver, which is a stand-alone program: nothing is loaded into python.
Sanitizers stay on host builds."""
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
    out = os.path.join(REPO, 'build', 'clear_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'clear_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize('seed', [1, 2])
def test_clearance_rule_clean_under_asan_ubsan(driver, seed):
    r = subprocess.run([driver, str(seed), '44'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    # every outcome occurred: paths without a region, unsolved, against a bad field, clear, crossed from inside, started outside; blocked and
    # free entries of the transit blocks; the field over the cap
    assert out['no_region'] >= 100 and out['unsolved'] >= 50 and out['bad_field'] >= 200 and out['clear'] >= 100 and out['crossed'] >= 100
    assert out['outside'] >= 20 and out['blocked'] >= 1000 and out['free'] >= 1000 and out['unsupported'] == 1
