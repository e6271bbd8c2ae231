"""The priced transit block's rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_solve_clear_sanitizers.py): tests/native/route_priced_sanitize_driver.cpp drives priced_transit of csrc/fcpp_solveclearfn.h --
the expressions fcpp_debug_route_transit_priced runs on the host and the kernels run on the device -- over random fields of swaths and
random regions in both modes: fields of 0 and 1 swaths, ponds over swath ends, regions without a ring and with a NaN vertex, penalty 0.
Any sanitizer report aborts the driver, which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('own', 'clear', 'rescued', 'blocked', 'outside', 'bad_field')


@pytest.fixture(scope='module')
def driver():
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    out = os.path.join(REPO, 'build', 'route_priced_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'route_priced_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_priced_transit_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', '140'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    # every kind of entry occurred, in both modes
    for mode in (0, 1):
        for kind in KINDS:
            assert out[f'{kind}{mode}'] >= 5, (kind, mode, out)
