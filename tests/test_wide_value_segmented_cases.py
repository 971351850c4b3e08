"""No GPU: the reference and the numpy model of tests/wide_value_segmented_cases.py (vrdxHipCmdWideValueSortSegmented).  The
clean model equals the reference on every case of the GPU list and runs exactly one pass per varying byte; every planted
fault changes some case -- keys, values or the passes run -- in every class it can occur in, so the GPU tests, which hold the
device to the same reference on the same cases, would see each of them (the passes excepted, which only the traffic shows)."""
import numpy as np
import pytest

import wide_value_segmented_cases as cases

CLASSES = tuple(cases.SIZES)


@pytest.fixture(scope="module")
def outcomes():
    """(class, builder) -> (keys, values, offsets, expected keys, expected values, expected passes), computed once"""
    out = {}
    for size_class in CLASSES:
        for builder in cases.BUILDERS:
            keys, values, offsets = cases.class_case(size_class, builder)
            want_keys, want_values = cases.expected(keys, values, offsets)
            passes = sum(cases.varying_bytes(keys[b:e]) for b, e in cases.valid_segments(offsets, len(keys)) if e - b >= 2)
            out[size_class, builder] = (keys, values, offsets, want_keys, want_values, passes)
    return out


def test_the_reference_is_a_stable_sort_of_every_segment_and_leaves_the_rest():
    keys, values, offsets = cases.class_case("small", "two_valued")
    want_keys, want_values = cases.expected(keys, values, offsets)
    assert np.array_equal(want_keys[:5], keys[:5]) and np.array_equal(want_values[-7:], values[-7:])
    for b, e in cases.valid_segments(offsets, len(keys)):
        order = np.argsort(keys[b:e], kind="stable")
        assert np.array_equal(want_keys[b:e], keys[b:e][order]) and np.array_equal(want_values[b:e], values[b:e][order])
    # offsets that are not monotone: the valid segments one by one
    bad = np.array([20, 30, 0, 10], np.uint32)
    k, v = cases.expected(keys[:40], values[:40], bad)
    assert np.array_equal(k[:10], np.sort(keys[:10])) and np.array_equal(k[20:30], np.sort(keys[20:30]))
    assert np.array_equal(k[10:20], keys[10:20]) and np.array_equal(k[30:], keys[30:40])
    assert np.array_equal(np.sort(v), np.sort(values[:40]))


def test_the_cases_hold_what_the_issue_lists():
    assert cases.SIZES["small"] == (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096)
    assert cases.SIZES["mid"] == (4097, 4352, 8191, 8192) and cases.SIZES["large"] == (8193, 8448, 16384, 16385, 24577, 40000)
    rng = np.random.default_rng(1)
    for at in range(4):
        keys = cases.make_keys(f"byte{at}", 5000, rng)
        assert int(np.bitwise_or.reduce(keys ^ keys[0])) == 0xFF << (8 * at)
    assert cases.varying_bytes(cases.make_keys("equal", 100, rng)) == 0
    assert cases.varying_bytes(cases.make_keys("bytes02", 5000, rng)) == 2
    assert cases.varying_bytes(cases.make_keys("bytes012", 5000, rng)) == 3
    ones = cases.make_keys("ones_third", 3000, rng)
    assert 800 < int((ones == cases.ONES).sum()) < 1200
    assert len(np.unique(cases.make_keys("two_valued", 100, rng))) == 2
    assert np.all(np.diff(cases.make_keys("descending", 40000, rng).astype(np.int64)) < 0)
    values = cases.make_values(40000, rng)
    assert not np.array_equal(values, np.arange(40000)) and len(np.unique(values)) == 40000
    assert np.all((values >> cases.SHIFT) != (values & cases.LOW))


@pytest.mark.parametrize("size_class", CLASSES)
def test_the_clean_model_equals_the_reference(outcomes, size_class):
    for builder in cases.BUILDERS:
        keys, values, offsets, want_keys, want_values, want_passes = outcomes[size_class, builder]
        got_keys, got_values, passes = cases.segmented_model(keys, values, offsets)
        assert np.array_equal(got_keys, want_keys), builder
        assert np.array_equal(got_values, want_values), builder
        assert passes == want_passes, builder


@pytest.mark.parametrize("fault,size_class", [(f, c) for f, where in cases.FAULTS.items() for c in where])
def test_every_fault_changes_some_case_where_it_can_occur(outcomes, fault, size_class):
    changed = []
    for builder in cases.BUILDERS:
        keys, values, offsets, want_keys, want_values, want_passes = outcomes[size_class, builder]
        got_keys, got_values, passes = cases.segmented_model(keys, values, offsets, fault=fault)
        if not (np.array_equal(got_keys, want_keys) and np.array_equal(got_values, want_values) and passes == want_passes):
            changed.append(builder)
    assert changed, f"{fault} goes unseen in the {size_class} class"


def test_there_are_at_least_the_seven_faults_of_the_issue():
    assert len(cases.FAULTS) >= 7 and all(set(where) <= set(CLASSES) and where for where in cases.FAULTS.values())


def test_the_model_leaves_bad_segments_alone():
    rng = np.random.default_rng(3)
    keys, values = cases.make_keys("random", 300, rng), cases.make_values(300, rng)
    offsets = np.array([100, 200, 0, 90, 400], np.uint32)   # a decreasing pair, an end behind the bound
    got_keys, got_values, _ = cases.segmented_model(keys, values, offsets)
    want_keys, want_values = cases.expected(keys, values, offsets)
    assert np.array_equal(got_keys, want_keys) and np.array_equal(got_values, want_values)
    assert np.array_equal(got_keys[200:], keys[200:]) and np.array_equal(got_keys[90:100], keys[90:100])
    assert np.array_equal(got_keys[:90], np.sort(keys[:90])) and np.array_equal(got_keys[100:200], np.sort(keys[100:200]))
