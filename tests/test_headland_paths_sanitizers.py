"""The headland-path rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_field_paths_sanitizers.py):
tests/native/headland_paths_sanitize_driver.cpp drives csrc/fcpp_hpathfn.h -- the expressions fcpp_debug_headland_paths runs on the host and
the kernels run on the device -- over the rings csrc/fcpp_insetfn.h cuts from the inset driver's shapes at the distances 2, 6, 8, 60 and
random ones, and over hand-made rings (arcs only, a NaN vertex, one vertex, none, a negative src, an arc of radius 0, an infinite
distance): both modes, both directions, R = 1.5, 6 and random, spacing 0.5 and 7; every array has its exact size.  Any sanitizer report
aborts the driver, which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
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
    out = os.path.join(REPO, 'build', 'headland_paths_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'headland_paths_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize('seed', [1, 2])
def test_headland_path_rule_clean_under_asan_ubsan(driver, seed):
    r = subprocess.run([driver, str(seed), '140'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    # every outcome occurred: closed loops, empty insets, failed rings of both kinds, every kind of leg, both directions and modes
    assert out['ok'] >= 150 and out['empty'] >= 20 and out['invalid'] >= 40 and out['unsupported'] >= 8
    assert out['straight'] >= 1000 and out['followed'] >= 300 and out['skipped'] >= 100 and out['connectors'] >= 1000 and out['smooth'] >= 300
    assert out['reversed'] >= 50 and out['reversing'] >= 50 and out['samples'] > 50000 and out['cusps'] > 500
