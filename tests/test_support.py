"""tests/support.py itself, on the CPU: the verdict on a sanitizer driver's run, the word parser, the bit view and the entry check each refuse
what they are there to refuse."""
import numpy as np
import pytest

from tests.support import bits, check_entries, judge_sanitized, word_counts

ENTRIES = {'fcpp_dubins_solve': 12}


def test_judge_rejects_a_failed_run_and_each_report_marker():
    judge_sanitized(0, 'ok 3', 'a warning that is no report')
    with pytest.raises(AssertionError):
        judge_sanitized(1, 'ok 3', '')
    for report in ('x.h:7:3: runtime error: signed integer overflow', '==12==ERROR: AddressSanitizer: heap-buffer-overflow',
                   '==12==ERROR: LeakSanitizer: detected memory leaks'):
        with pytest.raises(AssertionError):
            judge_sanitized(0, 'ok 3', 'before\n' + report + '\nafter')


def test_word_counts_round_trip():
    want = {'ok': 3, 'invalid': 0, 'samples': 123456789012}
    assert word_counts(' '.join('%s %d' % kv for kv in want.items()) + '\n') == want


@pytest.mark.parametrize('dtype', [np.int64, np.uint64])
def test_bits_tell_signed_zeros_apart_and_equate_equal_nans(dtype):
    assert bits(0.0, dtype).dtype == dtype and not np.array_equal(bits([0.0], dtype), bits([-0.0], dtype))
    nan = np.array([np.nan, -np.nan])
    assert np.array_equal(bits(nan, dtype), bits(nan.copy(), dtype)) and bits(nan, dtype)[0] != bits(nan, dtype)[1]


def test_check_entries_fails_on_a_missing_entry_and_a_count_off_by_one():
    check_entries(ENTRIES)
    for wrong in ({'fcpp_no_such_entry': 3}, {'fcpp_dubins_solve': 11}, {'fcpp_dubins_solve': 13}):
        with pytest.raises(AssertionError):
            check_entries(wrong)
