"""The polygon-coverage rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_headland_paths_sanitizers.py): tests/native/polygon_cover_sanitize_driver.cpp drives csrc/fcpp_pcoverfn.h -- the expressions
fcpp_debug_polygon_cover runs on the host and the kernels run on the device -- over the rectangle, the L with its hole, a 300-vertex star,
grids of 64 and 65 columns, failed fields of every kind and random fields, under swaths, a run of more than 256 samples, an arc, masked
connectors, NaN and infinite samples, paths of no and of one sample and random zigzags; both caps, with and without the work and pass
arrays, the path table grouped and permuted; every array has its exact size.  Any sanitizer report aborts the driver, which is a
stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
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
    out = os.path.join(REPO, 'build', 'polygon_cover_sanitize_driver')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
           '-ffp-contract=off', '-o', out, os.path.join(REPO, 'tests', 'native', 'polygon_cover_sanitize_driver.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize('seed', [1, 2])
def test_polygon_cover_rule_clean_under_asan_ubsan(driver, seed):
    r = subprocess.run([driver, str(seed), '40'], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr and 'LeakSanitizer' not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    out = {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}
    # every outcome occurred: good fields with and without paths, failed fields of both kinds, every class of cell, segment and path
    assert out['ok'] >= 200 and out['invalid'] >= 40 and out['unsupported'] >= 10 and out['no_paths'] >= 25
    assert out['cells'] > 1000000 and out['inside'] > 100000 and out['covered'] > 50000 and out['overlapped'] > 1000 and out['spill'] > 10000
    assert out['flat_ends'] >= 500 and out['joints'] >= 10000 and out['masked'] >= 300 and out['nonfinite'] >= 100
    assert out['empty_paths'] >= 30 and out['single_paths'] >= 20 and out['permuted'] >= 50 and out['round_runs'] >= 50 and out['long_runs'] >= 20
