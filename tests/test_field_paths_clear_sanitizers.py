"""The clear field-path rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_solve_clear_sanitizers.py): tests/native/field_paths_clear_sanitize_driver.cpp drives csrc/fcpp_fpathfn.h over
csrc/fcpp_solveclearfn.h -- the expressions fcpp_debug_field_paths_clear runs on the host and the kernels run on the device -- over fields of
0, 1 and 14 swaths, regions of 0, 3 and 257 edges, a NaN vertex, NaN poses, a bad order, both modes; any sanitizer report aborts the driver,
which is a stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('rank0', 'reshaped', 'blocked', 'outside', 'bad_region', 'ok_field', 'failed_field', 'empty_field')


@pytest.fixture(scope='module')
def driver():
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    out = os.path.join(REPO, 'build', 'field_paths_clear_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'field_paths_clear_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_clear_field_path_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', '240'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    # every kind of result occurred, in both modes
    for mode in (0, 1):
        for kind in KINDS:
            assert out[f'{kind}{mode}'] >= 5, (kind, mode, out)
    assert sum(out[f'{k}{mode}'] for k in KINDS[5:] for mode in (0, 1)) == 3 * 240
