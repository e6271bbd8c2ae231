"""The patch-pass rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_cover_regions_sanitizers.py): tests/native/patch_sanitize_driver.cpp drives csrc/fcpp_patchfn.h -- the key, layout, line, bin
and run functions the kernels run, and the host's order of work behind fcpp_debug_patch_swaths -- over the fixed shapes of the host tests,
zero-sized fields, labels of -2, a label that never occurs and random label grids at random angles, widths, margins and joins, and checks
every result against a brute-force pass.  Any sanitizer report aborts the driver, which is a stand-alone program: nothing is loaded into
python.  Sanitizers stay on host builds."""
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
    out = os.path.join(REPO, 'build', 'patch_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'patch_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_patch_rule_clean_under_asan_ubsan(driver):
    r = subprocess.run([driver, '1', str(N)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    print(out)
    # 14 fixed fields under 16 (angle, join, margin) triples, in one batch and alone; N random batches of 1 .. 4 fields
    assert out['fields'] >= 14 * 16 * 2 + N and out['regions'] > 10000 and out['swaths'] > 10000
