"""Without a GPU: the numpy model of the bit-range sorts (tests/sort_bits_cases.py) equals the reference on the ranges and
builders the GPU tests use, every plantable fault changes the result of at least one of those cases, and a whole-key sort
differs from the range sort on every case that has bits outside the range -- which is what makes that fault visible."""
import numpy as np
import pytest

import sort_bits_cases as cases

ALL_RANGES = cases.RANGES + [cases.EMPTY_RANGE, cases.FULL_RANGE]
CASES = [(builder, n, begin, end) for builder in cases.BUILDERS for n in cases.BUILDER_SIZES for begin, end in ALL_RANGES]


@pytest.fixture(scope="module")
def results():
    """inputs and the reference of every case, computed once"""
    out = {}
    for case in CASES:
        builder, n, begin, end = case
        keys, values = cases.case_inputs(builder, n, begin, end)
        out[case] = (keys, values, cases.reference(keys, values, begin, end))
    return out


def test_the_model_equals_the_reference(results):
    for (builder, n, begin, end), (keys, values, (want_keys, want_values)) in results.items():
        got_keys, got_values = cases.sort_bits_model(keys, values, begin, end)
        assert np.array_equal(got_keys, want_keys) and np.array_equal(got_values, want_values), (builder, n, begin, end)
        only_keys, none = cases.sort_bits_model(keys, None, begin, end)
        assert none is None and np.array_equal(only_keys, want_keys), (builder, n, begin, end)


def test_a_count_leaves_the_tail_alone(results):
    keys, values, _ = results["uniform", 4097, 3, 12]
    for count in (0, 1, 4096, 4097, 5000):
        want = cases.reference(keys, values, 3, 12, count)
        got = cases.sort_bits_model(keys, values, 3, 12, count)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(want[0][min(count, 4097):], keys[min(count, 4097):])


@pytest.mark.parametrize("fault", cases.FAULTS)
def test_every_planted_fault_changes_some_case(results, fault):
    caught = []
    for (builder, n, begin, end), (keys, values, (want_keys, want_values)) in results.items():
        if n != cases.BUILDER_SIZES[0]:
            continue   # (one size is enough to catch every fault, and the model is the same at both)
        got_keys, got_values = cases.sort_bits_model(keys, values, begin, end, fault=fault)
        if not (np.array_equal(got_keys, want_keys) and np.array_equal(got_values, want_values)):
            caught.append((builder, begin, end))
    assert caught, fault
    # ... and the keys alone give the key faults away: the bits outside the range tell equal fields apart
    if fault != "values-stale":
        assert any(not np.array_equal(cases.sort_bits_model(results[b, cases.BUILDER_SIZES[0], lo, hi][0], None, lo, hi, fault=fault)[0],
                                      results[b, cases.BUILDER_SIZES[0], lo, hi][2][0]) for b, lo, hi in caught), fault


def test_a_whole_key_sort_differs_from_the_range_sort(results):
    seen = 0
    for (builder, n, begin, end), (keys, values, (want_keys, _)) in results.items():
        if not cases.non_degenerate(builder, n, begin, end):
            continue
        seen += 1
        assert not np.array_equal(np.sort(keys), want_keys), (builder, n, begin, end)
    # all but (1, 32) with fields that are as good as distinct (uniform, const-byte): there the two orders are one
    assert seen == len(cases.BUILDER_SIZES) * (len(cases.BUILDERS) * len(cases.RANGES) - 2)


def test_the_builders_build_what_they_say():
    for begin, end in cases.RANGES:
        width = end - begin
        for builder in cases.BUILDERS:
            keys, values = cases.case_inputs(builder, 4097, begin, end)
            f = cases.field(keys, begin, end)
            outside = keys & ~np.uint32(((1 << width) - 1) << begin)
            assert len(np.unique(outside)) > 1 or width == 32   # random bits outside the range
            if builder == "few":
                assert len(np.unique(f)) <= 3
            if builder == "const-byte":
                assert len(np.unique(f & np.uint32(0xFF))) == 1 and (width <= 8 or len(np.unique(f)) > 1)
            if builder == "equal":
                assert len(np.unique(f)) == 1
            if builder == "ones":
                assert (f == (1 << width) - 1).all()
            assert not np.array_equal(values, np.arange(4097, dtype=np.uint32))
