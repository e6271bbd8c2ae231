"""The polygon-coverage rule under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU (the pattern of
tests/test_headland_paths_sanitizers.py): tests/native/polygon_cover_sanitize_driver.cpp drives csrc/fcpp_pcoverfn.h -- the expressions
fcpp_debug_polygon_cover runs on the host and the kernels run on the device -- over the rectangle, the L with its hole, a 300-vertex star,
grids of 64 and 65 columns, failed fields of every kind and random fields, under swaths, a run of more than 256 samples, an arc, masked
connectors, NaN and infinite samples, paths of no and of one sample and random zigzags; both caps, with and without the work and pass
arrays, the path table grouped and permuted; every array has its exact size.  Any sanitizer report aborts the driver, which is a
stand-alone program: nothing is loaded into python.  Sanitizers stay on host builds."""
import pytest

from tests.support import run_sanitized, sanitize_driver, word_counts


@pytest.fixture(scope='module')
def driver():
    return sanitize_driver('polygon_cover_sanitize_driver')


@pytest.mark.parametrize('seed', [1, 2])
def test_polygon_cover_rule_clean_under_asan_ubsan(driver, seed):
    out = word_counts(run_sanitized(driver, seed, 40))
    # every outcome occurred: good fields with and without paths, failed fields of both kinds, every class of cell, segment and path
    assert out['ok'] >= 200 and out['invalid'] >= 40 and out['unsupported'] >= 10 and out['no_paths'] >= 25
    assert out['cells'] > 1000000 and out['inside'] > 100000 and out['covered'] > 50000 and out['overlapped'] > 1000 and out['spill'] > 10000
    assert out['flat_ends'] >= 500 and out['joints'] >= 10000 and out['masked'] >= 300 and out['nonfinite'] >= 100
    assert out['empty_paths'] >= 30 and out['single_paths'] >= 20 and out['permuted'] >= 50 and out['round_runs'] >= 50 and out['long_runs'] >= 20
