"""No GPU: the plain-numpy model of the segmented bit-range sort (tests/segmented_bits_cases.py) equals the reference on every
case the GPU tests run, every plantable fault changes some case -- so the cases can tell a kernel with that mistake from a
correct one -- and a whole-key segmented sort differs from the range sort wherever the case is not degenerate."""
import numpy as np
import pytest

import segmented_cases
from segmented_bits_cases import (BUILDERS, FAULTS, PASS_CASES, PASS_SIZES, RANGES, case_inputs, expected, non_degenerate,
                                  segmented_bits_model)


def pass_case(builder, rng_range, size):
    return case_inputs(builder, *rng_range, sizes=[size], tag=f"pass/{size}")


@pytest.mark.parametrize("builder", BUILDERS)
def test_model_equals_the_reference_on_the_size_class_cases(builder):
    for begin, end in RANGES:
        keys, values, offsets = case_inputs(builder, begin, end)
        want = expected(keys, values, offsets, len(keys), begin, end)
        got = segmented_bits_model(keys, values, offsets, begin, end)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (builder, begin, end)
        keys_only = segmented_bits_model(keys, None, offsets, begin, end)
        assert np.array_equal(keys_only[0], want[0]) and keys_only[1] is None


@pytest.mark.parametrize("size", PASS_SIZES)
def test_model_equals_the_reference_on_the_pass_cases(size):
    for builder, (begin, end) in PASS_CASES:
        keys, values, offsets = pass_case(builder, (begin, end), size)
        want = expected(keys, values, offsets, len(keys), begin, end)
        got = segmented_bits_model(keys, values, offsets, begin, end)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (builder, begin, end)


def test_model_leaves_bad_segments_alone():
    rng = np.random.default_rng(5)
    n = 50000
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    values = np.arange(n, dtype=np.uint32)
    offsets = np.array([100, 1100, 21100, 9000, 9000, n + 5000], np.uint32)
    want = expected(keys, values, offsets, n, 7, 24)
    got = segmented_bits_model(keys, values, offsets, 7, 24)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(want[0][21100:], keys[21100:]) and not np.array_equal(want[0][1100:21100], keys[1100:21100])


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_changes_some_case(fault):
    cases = [(pass_case(b, r, PASS_SIZES[0]), r) for b, r in PASS_CASES]
    cases += [(case_inputs("uniform", *r), r) for r in ((3, 12), (7, 24))]
    for (keys, values, offsets), (begin, end) in cases:
        want = expected(keys, values, offsets, len(keys), begin, end)
        got = segmented_bits_model(keys, values, offsets, begin, end, fault=fault)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            return
    raise AssertionError(f"no case tells a kernel with the fault {fault!r} from a correct one")


def test_a_whole_key_segmented_sort_is_another_sort():
    checked = 0
    for builder in BUILDERS:
        for begin, end in RANGES:
            if not non_degenerate("uniform" if builder == "const-middle" else builder, 4097, begin, end):
                continue
            keys, values, offsets = case_inputs(builder, begin, end)
            want = expected(keys, values, offsets, len(keys), begin, end)
            whole = segmented_cases.expected(keys, values, offsets, len(keys))
            assert not np.array_equal(want[0], whole[0]), (builder, begin, end)
            checked += 1
    assert checked >= 40
