"""The loop-transit rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_solve_clear_sanitizers.py): tests/native/loop_transit_sanitize_driver.cpp drives csrc/fcpp_transitfn.h -- the expressions
fcpp_debug_loop_transits runs on the host and the kernels run on the device -- over loops of 1, 7, 64, 200 and more samples than the station
cap, fields without loops or stations, a NaN vertex, a NaN arc length, NaN poses and field indices outside the list, both modes; it picks
every pair twice (the twin's pick, and a second look at every candidate) and samples every found transit.  Any sanitizer report aborts
the driver, which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 360


@pytest.fixture(scope='module')
def driver():
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    out = os.path.join(REPO, 'build', 'loop_transit_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'loop_transit_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_loop_transit_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', str(N)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    for mode in (0, 1):
        for kind in ('einval', 'cap', 'none', 'via'):
            assert out[f'{kind}{mode}'] >= 1, (kind, mode, out)
        assert out[f'ride{mode}'] + out[f'wrap{mode}'] >= 1, out
    assert sum(out.values()) == N
