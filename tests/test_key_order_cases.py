"""No GPU: the references of the key orders of the 64-bit sorts (tests/key_order_cases.py) agree with numpy's own orders, T
is a bijection with the inverse the kernels use, the plain-numpy model of both device forms equals the references on the
cases the GPU tests run, and every plantable fault changes some case -- so the cases can tell a kernel with that mistake
from a correct one."""
import numpy as np
import pytest

from key_order_cases import (BUILDERS, DIRECTIONS, FAULTS, FLOAT_EDGES, INT_EDGES, ONES, ORDERS, T, T_inverse, all_ones_key,
                             case_keys, expected, expected_segments, order_word, segment_case, segmented64_ordered_model,
                             sort64_ordered_model)

CASES = [(o, d) for o in ORDERS for d in DIRECTIONS]
SEGMENT_SIZES = [0, 1, 2, 255, 4096, 4097, 8192, 8193, 16384, 16385, 20001]


def same(got, want):
    return np.array_equal(got[0], want[0]) and (want[1] is None or np.array_equal(got[1], want[1]))


def test_the_order_word():
    assert [order_word(o) for o in ORDERS] == [0, 1, 2]
    assert order_word("float64", True) == 0x102


@pytest.mark.parametrize("order,descending", CASES)
def test_T_is_a_bijection_and_T_inverse_inverts_it(order, descending):
    rng = np.random.default_rng(1)
    keys = np.concatenate([rng.integers(0, 1 << 64, size=5000, dtype=np.uint64), INT_EDGES, FLOAT_EDGES])
    assert np.array_equal(T_inverse(T(keys, order, descending), order, descending), keys)
    assert np.array_equal(T(T_inverse(keys, order, descending), order, descending), keys)
    assert T(np.array([all_ones_key(order, descending)]), order, descending)[0] == ONES
    assert np.array_equal(T(keys, order, True), ~T(keys, order, False))


def test_the_keys_that_T_maps_to_all_ones():
    got = {(o, d): int(all_ones_key(o, d)) for o, d in CASES}
    assert got == {("uint64", False): (1 << 64) - 1, ("uint64", True): 0, ("int64", False): (1 << 63) - 1,
                   ("int64", True): 1 << 63, ("float64", False): 0x7FFFFFFFFFFFFFFF, ("float64", True): 0xFFFFFFFFFFFFFFFF}


def test_the_reference_is_numpys_order_of_int64():
    keys, values = case_keys("mixed-int", 20001, "int64", False)
    assert np.array_equal(expected(keys, values, "int64")[0].view(np.int64), np.sort(keys.view(np.int64)))
    assert np.array_equal(expected(keys, values, "uint64")[0], np.sort(keys))
    unique = np.unique(keys)   # no duplicates: descending is the reverse
    rng = np.random.default_rng(2)
    rng.shuffle(unique)
    assert np.array_equal(expected(unique, None, "int64", True)[0].view(np.int64), np.sort(unique.view(np.int64))[::-1])
    assert np.array_equal(expected(unique, None, "uint64", True)[0], np.sort(unique)[::-1])


def test_the_reference_is_numpys_order_of_float64_without_nans():
    keys, values = case_keys("float-values", 20001, "float64", False)
    keys = np.concatenate([keys, np.array([np.inf, -np.inf, 5e-324, -5e-324, 0.0]).view(np.uint64)])
    assert not np.isnan(keys.view(np.float64)).any()
    got = expected(keys, None, "float64")[0].view(np.float64)
    assert np.array_equal(got, np.sort(keys.view(np.float64)))   # compared as float values
    unique = np.unique(keys)
    assert np.array_equal(expected(unique, None, "float64", True)[0].view(np.float64), np.sort(unique.view(np.float64))[::-1])


def test_float64_is_totalOrder():
    """negative NaNs, -inf ... -0.0, +0.0 ... +inf, positive NaNs; NaN payloads as bits"""
    ordered = np.array([0xFFFFFFFFFFFFFFFF, 0xFFF8000000BEEF00, 0xFFF8000000000000, 0xFFF0000000000001], np.uint64)
    ordered = np.concatenate([ordered, np.array([-np.inf, -1e300, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, 1e300, np.inf]).view(np.uint64),
                              np.array([0x7FF0000000000001, 0x7FF8000000000000, 0x7FF8000000BEEF00, 0x7FFFFFFFFFFFFFFF], np.uint64)])
    shuffled = ordered.copy()
    np.random.default_rng(3).shuffle(shuffled)
    assert np.array_equal(expected(shuffled, None, "float64")[0], ordered)
    assert np.array_equal(expected(shuffled, None, "float64", True)[0], ordered[::-1])


@pytest.mark.parametrize("order,descending", CASES)
def test_equal_keys_keep_their_input_order_in_both_directions(order, descending):
    keys, values = case_keys("duplicates", 5000, order, descending)
    ek, ev = expected(keys, values, order, descending)
    index = np.arange(len(keys))[np.argsort(T(keys, order, descending), kind="stable")]
    for key in np.unique(keys):
        assert (np.diff(index[ek == key]) > 0).all()


@pytest.mark.parametrize("order,descending", CASES)
@pytest.mark.parametrize("builder", BUILDERS)
def test_the_composition_model_equals_the_reference(builder, order, descending):
    for n in (1, 5, 1025, 16385):
        keys, values = case_keys(builder, n, order, descending)
        want = expected(keys, values, order, descending)
        assert same(sort64_ordered_model(keys, values, order, descending), want), n
        assert same(sort64_ordered_model(keys, None, order, descending), (want[0], None)), n


@pytest.mark.parametrize("order,descending", CASES)
@pytest.mark.parametrize("builder", ["uniform", "float-specials", "duplicates", "ones-in-T", "plus-minus-x"])
def test_the_segmented_model_equals_the_reference(builder, order, descending):
    keys, values, offsets = segment_case(builder, SEGMENT_SIZES, order, descending)
    want = expected_segments(keys, values, offsets, len(keys), order, descending)
    assert same(segmented64_ordered_model(keys, values, offsets, order, descending), want)
    assert same(segmented64_ordered_model(keys, None, offsets, order, descending), (want[0], None))


def test_the_segmented_reference_leaves_bad_segments_alone():
    keys, values = case_keys("float-specials", 30000, "float64", True)
    offsets = np.array([100, 1100, 21100, 9000, 9000, 35000], np.uint32)
    ek, ev = expected_segments(keys, values, offsets, len(keys), "float64", True)
    assert np.array_equal(ek[21100:], keys[21100:]) and np.array_equal(ev[21100:], values[21100:])
    assert same(segmented64_ordered_model(keys, values, offsets, "float64", True), (ek, ev))
    assert not np.array_equal(ek[1100:21100], keys[1100:21100])


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_changes_some_case(fault):
    for order, descending in CASES:
        for builder in ("float-specials", "duplicates", "plus-minus-x", "ones-in-T"):
            keys, values = case_keys(builder, 1025, order, descending)
            want = expected(keys, values, order, descending)
            if not same(sort64_ordered_model(keys, values, order, descending, fault=fault), want):
                return
            if not same(sort64_ordered_model(keys, None, order, descending, fault=fault), (want[0], None)):
                return
            keys, values, offsets = segment_case(builder, [1000, 4097, 16385], order, descending)
            want = expected_segments(keys, values, offsets, len(keys), order, descending)
            if not same(segmented64_ordered_model(keys, values, offsets, order, descending, fault=fault), want):
                return
    raise AssertionError(f"no case tells a kernel with the fault {fault!r} from a correct one")


def test_the_unsigned_ascending_order_is_the_existing_sort():
    keys, values = case_keys("uniform", 5000, "uint64", False)
    perm = np.argsort(keys, kind="stable")
    assert same(expected(keys, values, "uint64"), (keys[perm], values[perm]))
