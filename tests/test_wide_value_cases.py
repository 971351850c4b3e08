"""Without a GPU: the numpy model of the three forms of the sort of 32-bit keys with 64-bit values (tests/wide_value_cases.py)
against the reference on every case, and every plantable fault of the model against some case -- so that the GPU suite, which
holds the device to the same reference on the same kinds of keys and values, can tell each of those mistakes from a correct
kernel."""
import numpy as np
import pytest

import wide_value_cases as cases

TWO_SORTS_FROM = 20000   # (the model takes the constant as an argument: small here, so that all three forms are cheap)
ONE_WORKGROUP_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)
GATHER_SIZES = (8193, 8194, 8195, 8196, 9215, 9216, 9217, 16384, 16385)
TWO_SORTS_SIZES = (TWO_SORTS_FROM, TWO_SORTS_FROM + 1, TWO_SORTS_FROM + 2, TWO_SORTS_FROM + 3)


def _cases():
    """(builder, bound, count, total): direct calls at every size, indirect ones either side of the bound"""
    for builder in cases.BUILDERS:
        for n in ONE_WORKGROUP_SIZES + GATHER_SIZES + TWO_SORTS_SIZES:
            yield builder, n, None, n
    for bound in (8192, TWO_SORTS_FROM - 1, TWO_SORTS_FROM):
        for count in (0, 1, 8193, bound - 1, bound, bound + 7):
            yield "uniform", bound, count, bound + 16
            yield "three", bound, count, bound + 16


def _arrays(builder, total, seed):
    rng = np.random.default_rng(seed)
    return cases.make_keys(builder, total, rng), cases.make_values(total, rng)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_the_forms_by_size():
    assert cases.form_of(0, TWO_SORTS_FROM) == "none"
    assert [cases.form_of(n, TWO_SORTS_FROM) for n in (1, 8192, 8193, TWO_SORTS_FROM - 1, TWO_SORTS_FROM)] == \
        ["one-workgroup", "one-workgroup", "gather", "gather", "two-sorts"]
    assert cases.form_of(8192, TWO_SORTS_FROM, small_sort=False) == "gather"


def test_the_values_show_a_dropped_or_swapped_word():
    v = cases.make_values(5000, np.random.default_rng(0))
    lo, hi = v & cases.LOW, v >> cases.SHIFT
    assert (lo != hi).all() and len(np.unique(v)) > 4990
    assert (lo == 0).any() and (hi == 0).any() and (lo == 0xFFFFFFFF).any() and (hi == 0xFFFFFFFF).any()
    assert not np.array_equal(v, np.arange(5000))


def test_the_clean_forms_equal_the_reference_on_all_cases():
    for seed, (builder, bound, count, total) in enumerate(_cases()):
        keys, values = _arrays(builder, total, seed)
        n = bound if count is None else min(count, bound)
        got = cases.wide_value_model(keys, values, bound, count, TWO_SORTS_FROM)
        assert _same(got, cases.expected(keys, values, n)), (builder, bound, count)
    # smallSort off: n <= 8192 through the gather form
    keys, values = _arrays("three", 5000, 1)
    assert _same(cases.wide_value_model(keys, values, two_sorts_from=TWO_SORTS_FROM, small_sort=False), cases.expected(keys, values))


@pytest.mark.parametrize("fault", cases.FAULTS)
def test_every_fault_changes_the_result_of_some_case(fault):
    caught = []
    for seed, (builder, bound, count, total) in enumerate(_cases()):
        keys, values = _arrays(builder, total, seed)
        n = bound if count is None else min(count, bound)
        got = cases.wide_value_model(keys, values, bound, count, TWO_SORTS_FROM, fault=fault)
        if not _same(got, cases.expected(keys, values, n)):
            caught.append((cases.form_of(bound, TWO_SORTS_FROM), builder, bound, count))
    assert caught, fault
    forms = {form for form, *_ in caught}
    # a fault shows in every form it can occur in
    where = {"gather-by-position": {"gather"}, "second-sort-on-sorted-copy": {"two-sorts"}, "scalar-tail-dropped": {"gather", "two-sorts"},
             "pad-stored": {"one-workgroup"}, "constant-byte-from-all-slots": {"one-workgroup"}}
    assert forms == where.get(fault, {"one-workgroup", "gather", "two-sorts"}), (fault, forms)


def test_a_pad_stored_shows_only_behind_the_count():
    """the fault the guard bytes and the untouched tail are for: an indirect count below the bound"""
    keys, values = _arrays("uniform", 8192 + 16, 3)
    got = cases.wide_value_model(keys, values, 8192, 1000, TWO_SORTS_FROM, fault="pad-stored")
    want = cases.expected(keys, values, 1000)
    assert np.array_equal(got[0][:1000], want[0][:1000]) and not np.array_equal(got[0][1000:1024], want[0][1000:1024])
