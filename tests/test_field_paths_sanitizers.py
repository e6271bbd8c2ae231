"""The field-path rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_route_sanitizers.py):
tests/native/field_paths_sanitize_driver.cpp drives csrc/fcpp_fpathfn.h -- the expressions fcpp_debug_field_paths runs on the host and the
kernels run on the device -- over random swath sets: m = 0 .. 40, both modes, with and without an order, an entry and an exit pose, some
with a poisoned order or a NaN, negative or infinite length; every array has its exact size.  Any sanitizer report aborts the driver,
which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
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
    out = os.path.join(REPO, 'build', 'field_paths_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'field_paths_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize('seed', [1, 2])
def test_field_path_rule_clean_under_asan_ubsan(driver, seed):
    r = subprocess.run([driver, str(seed), '140'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    # every outcome occurred: fields with paths, failed ones of both kinds, empty ones, every combination's ingredients, reversing cusps
    assert out['ok'] >= 100 and out['invalid'] >= 10 and out['bad_order'] >= 3 and out['bad_length'] >= 3 and out['empty'] >= 1
    assert out['ordered'] >= 50 and out['entry'] >= 40 and out['exit'] >= 40 and out['reversing'] >= 40
    assert out['samples'] > 100000 and out['cusps'] > 100
