"""Without a GPU: the references of the ordered 32-bit sorts (tests/key_order32_cases.py) against numpy's own typed sorts, T
against its inverse, the numpy model of the three device forms against the references, and every plantable fault of the model
against some case -- so that the GPU suites, which hold the device to the same references on the same keys, can tell each of
those mistakes from a correct kernel."""
import numpy as np
import pytest

import key_order32_cases as cases

SIZES = (1, 2, 255, 257, 4097, 16384)
FLAT_SIZES = (16385, 16387, 40000)
LARGE = 3 * cases.TILE + 1234   # three full tiles of the large kernel and a partial one


@pytest.mark.parametrize("descending", cases.DIRECTIONS)
@pytest.mark.parametrize("order", cases.ORDERS)
def test_T_is_a_bijection_with_the_stated_inverse(order, descending):
    rng = np.random.default_rng(1)
    keys = np.concatenate([cases.INT_EDGES, cases.FLOAT_EDGES, cases.make_keys("uniform", 100000, rng)])
    t = cases.T(keys, order, descending)
    assert np.array_equal(cases.T_inverse(t, order, descending), keys)
    assert len(np.unique(t)) == len(np.unique(keys))
    assert cases.T(np.array([cases.all_ones_key(order, descending)]), order, descending)[0] == cases.ONES
    assert np.array_equal(cases.T(keys, "uint32"), keys)   # order word 0: the identity


@pytest.mark.parametrize("descending", cases.DIRECTIONS)
def test_the_reference_is_numpys_sort_of_the_typed_view(descending):
    for builder in ("uniform", "mixed-int", "duplicates"):
        keys, values = cases.case_keys(builder, 5000, "int32", descending)
        ek, ev = cases.expected(keys, values, "int32", descending)
        want = np.sort(keys.view(np.int32))
        assert np.array_equal(ek.view(np.int32), want[::-1] if descending else want), builder
        # equal keys in input order, in both directions: the values of one key ascend wherever payload() ascends
        perm = np.argsort(-keys.view(np.int32).astype(np.int64) if descending else keys.view(np.int32), kind="stable")
        assert np.array_equal(ev, values[perm]), builder
    keys, values = cases.case_keys("float-values", 5000, "float32", descending)
    assert not np.isnan(keys.view(np.float32)).any() and (keys.view(np.float32) != 0).all()
    ek, ev = cases.expected(keys, values, "float32", descending)
    want = np.sort(keys.view(np.float32))
    assert np.array_equal(ek, (want[::-1] if descending else want).view(np.uint32))
    perm = np.argsort(-keys.view(np.float32).astype(np.float64) if descending else keys.view(np.float32), kind="stable")
    assert np.array_equal(ev, values[perm])


def test_float32_is_total_order():
    keys = cases.FLOAT_EDGES.copy()
    ek, _ = cases.expected(keys, None, "float32")
    f = ek.view(np.float32)
    nan = np.isnan(f)
    negative = (ek >> np.uint32(31)) != 0
    first, last = np.flatnonzero(nan & negative), np.flatnonzero(nan & ~negative)
    assert len(first) == 4 and len(last) == 4
    assert first.max() == 3 and last.min() == len(keys) - 4           # NaNs with the sign bit set first, the others last
    assert np.array_equal(ek[first], np.sort(ek[first])[::-1])        # among themselves by payload: the larger, the further out
    assert np.array_equal(ek[last], np.sort(ek[last]))
    body = f[4:-4]
    assert body[0] == -np.inf and body[-1] == np.inf and (np.diff(body) >= 0).all()
    zeros = np.flatnonzero(body == 0)
    assert np.array_equal(ek[4:-4][zeros], np.array([0x80000000, 0], np.uint32))   # -0.0 in front of +0.0


@pytest.mark.parametrize("descending", cases.DIRECTIONS)
@pytest.mark.parametrize("order", cases.ORDERS)
def test_the_model_of_the_flat_sorts_gives_the_reference(order, descending):
    for builder in cases.BUILDERS:
        for n in SIZES + FLAT_SIZES[:2]:
            keys, values = cases.case_keys(builder, n, order, descending)
            for v in (None, values):
                cases.assert_same(*cases.ordered_sort_model(keys, v, order, descending), cases.expected(keys, v, order, descending),
                                  f"{builder} {n}")
    for bound, counts in ((16384, (0, 1, 5, 16383, 16384, 16391)), (40000, (0, 1, 5, 16384, 16385, 39999, 40000, 40007))):
        keys, values = cases.case_keys("float-specials", bound, order, descending)
        for count in counts:
            cases.assert_same(*cases.ordered_sort_model(keys, values, order, descending, count=count),
                              cases.expected(keys, values, order, descending, count=count), f"count {count} of {bound}")


@pytest.mark.parametrize("descending", cases.DIRECTIONS)
@pytest.mark.parametrize("order", cases.ORDERS)
def test_the_model_of_the_segmented_sorts_gives_the_reference(order, descending):
    for builder in cases.BUILDERS:
        keys, values, offsets = cases.segment_case(builder, [0, 1, 2, 4095, 4097, 16385, LARGE], order, descending)
        for v in (None, values):
            cases.assert_same(*cases.segmented_ordered_model(keys, v, offsets, order, descending),
                              cases.expected_segments(keys, v, offsets, len(keys), order, descending), builder)


def _changed(fault):
    """the cases (form, builder, order, descending) whose model output the fault changes"""
    out = []
    for order in cases.ORDERS:
        for descending in cases.DIRECTIONS:
            for builder in ("float-specials", "duplicates", "one-byte", "three-bytes", "plus-minus-x", "ones-in-T"):
                keys, values = cases.case_keys(builder, 1000, order, descending)
                good = cases.ordered_sort_model(keys, values, order, descending)
                bad = cases.ordered_sort_model(keys, values, order, descending, fault=fault)
                if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
                    out.append(("one workgroup", builder, order, descending))
                keys, values = cases.case_keys(builder, 20000, order, descending)
                good = cases.ordered_sort_model(keys, values, order, descending, count=17000)
                bad = cases.ordered_sort_model(keys, values, order, descending, count=17000, fault=fault)
                if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
                    out.append(("flat under a count", builder, order, descending))
                keys, values, offsets = cases.segment_case(builder, [1000, LARGE], order, descending)
                good = cases.segmented_ordered_model(keys, values, offsets, order, descending)
                bad = cases.segmented_ordered_model(keys, values, offsets, order, descending, fault=fault)
                if not np.array_equal(good[0], bad[0]):
                    out.append(("segmented, keys", builder, order, descending))
                elif not np.array_equal(good[1], bad[1]):
                    out.append(("segmented, values only", builder, order, descending))
    return out


@pytest.mark.parametrize("fault", cases.FAULTS)
def test_every_fault_changes_some_case(fault):
    changed = _changed(fault)
    assert changed, fault
    forms = {form for form, *_ in changed}
    if fault in ("histogram-from-raw-keys", "no-inverse-before-copy-back"):
        assert forms == {"segmented, keys"}, forms                     # the large class only
        if fault == "histogram-from-raw-keys":
            assert ("segmented, keys", "plus-minus-x", "float32", False) in changed
        else:
            assert {b for _, b, *_ in changed} <= {"one-byte", "three-bytes", "plus-minus-x"}   # an odd number of passes
    if fault == "transform-up-to-the-bound":
        assert forms == {"flat under a count"}, forms
    if fault == "descending-by-reversal":
        assert all(descending for *_, descending in changed)
        # seen through the values: the keys of a reversed ascending sort are those of the descending one
        assert ("segmented, values only", "duplicates", "uint32", True) in changed
    if fault in ("float-mask-flips-sign", "neg-from-untransformed-word"):
        assert {order for _, _, order, _ in changed} == {"float32"}
    if fault == "pads-transformed":
        assert not any(order == "uint32" and not descending for _, _, order, descending in changed)   # T is the identity there
        assert "one workgroup" in forms and "segmented, keys" in forms
