"""The swath router's rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of tests/test_swaths_sanitizers.py):
tests/native/route_sanitize_driver.cpp drives csrc/fcpp_routefn.h -- the expressions fcpp_debug_route runs on the host and the kernels run
on the device -- over random transit blocks, bit-symmetric under (p, q) <-> (q ^ 1, p ^ 1) with an infinite same-swath diagonal: m = 0 .. 40
and both sides of the cap (512, 513), 1 .. 64 candidates, with and without E / X, some with NaN or infinite entries; any sanitizer report
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
    out = os.path.join(REPO, 'build', 'route_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'route_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize('seed', [1, 2])
def test_route_rule_clean_under_asan_ubsan(driver, seed):
    r = subprocess.run([driver, str(seed), '60'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    # every outcome occurred: routed fields, some of them improved, invalid ones, the field over the cap, poisoned blocks, applied moves
    assert out['ok'] >= 30 and out['improved'] >= 20 and out['invalid'] >= 1 and out['unsupported'] == 1 and out['poisoned'] >= 5
    assert out['moves'] > 100
