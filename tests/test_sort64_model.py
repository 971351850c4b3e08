"""The model of the 64-bit sorts (tests/sort64_model.py) on every input the GPU tests of tests/test_sort64_edges_gpu.py run
at n <= 2049: the faithful composition is the sort numpy gives, every planted fault is turned down by check64 on an input
named here, and iota values -- what the suite carried before payload64 -- let a fault through (no GPU needed)."""
import numpy as np
import pytest

import plan_model
import sort64_model as model
from sort64_model import FAULTS, case_inputs, check64, expected64, payload64, small_cases, sort64_model

# one input that must tell each fault from the right sort: (pattern, n, key+value)
WITNESS = {
    "value-is-index": ("dup-high", 5, True),
    "low-from-high": ("dup-high", 5, True),
    "merge-swaps-lanes": ("dup-high", 1027, False),
    "tail-index": ("dup-high", 1027, True),
    "tail-values-stale": ("dup-high", 1027, True),
    "second-sort-unstable": ("dup-high", 1027, False),
}


def _passes(pattern, n, key_value, fault, values=None):
    keys, payload = case_inputs(pattern, n)
    values = (payload if values is None else values) if key_value else None
    got_keys, got_values = sort64_model(keys, values, fault=fault)
    try:
        check64(got_keys, got_values, keys, values)
    except AssertionError:
        return False
    return True


def test_the_cases_cover_every_tail_and_both_sides_of_a_workgroup():
    sizes = {n for _, n in small_cases()}
    assert {n % 4 for n in sizes} == {0, 1, 2, 3}
    assert {1021, 1022, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 2049} <= sizes and max(sizes) == 2049
    assert {p for p, _ in small_cases()} == set(model.VALUE_PATTERNS)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 1027, 100_003])
def test_payload_is_never_the_index(n):
    v = payload64(n)
    assert len(v) == n and v.dtype == np.uint32
    assert not (v == np.arange(n, dtype=np.uint32)).any()
    if n > 1:
        assert (v == 0xFFFFFFFF).sum() == 1 and (v == 0).sum() == 1
        rest = np.sort(v[(v != 0xFFFFFFFF) & (v != 0)] ^ np.uint32(0x80000000))
        assert len(np.unique(rest)) == n - 2 and (rest < n).all()   # what is left of a permutation of 0 ... n - 1


def test_dup_high_has_runs_of_high_words_and_exact_duplicates():
    keys, _ = case_inputs("dup-high", 1027)
    lo, hi = model.words_of(keys)
    assert len(np.unique(hi)) <= 37 and len(np.unique(lo)) > 700
    assert len(np.unique(keys)) < 1027 - 150   # about a fifth of the keys are copies


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_the_faithful_model_is_the_sort(key_value):
    for pattern, n in small_cases():
        keys, payload = case_inputs(pattern, n)
        values = payload if key_value else None
        got_keys, got_values = sort64_model(keys, values)
        want_keys, want_values = expected64(keys, values)
        assert np.array_equal(got_keys, want_keys), (pattern, n)
        assert not key_value or np.array_equal(got_values, want_values), (pattern, n)
        check64(got_keys, got_values, keys, values)
    assert sort64_model(np.zeros(0, np.uint64))[0].size == 0


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_is_turned_down(fault):
    pattern, n, key_value = WITNESS[fault]
    assert (pattern, n) in small_cases()
    assert not _passes(pattern, n, key_value, fault), f"{fault} passes check64 on {pattern} n={n}"
    caught = [(p, m, kv) for p, m in small_cases() for kv in (False, True) if not _passes(p, m, kv, fault)]
    print(f"{fault}: turned down on {len(caught)} of {2 * len(small_cases())} runs, first {caught[0]}")
    assert (pattern, n, key_value) in caught


def test_iota_values_hide_a_permute_that_writes_the_index():
    """values = arange(n) are their own index, so values[I[j]] == I[j]: the blind spot payload64 closes"""
    for pattern, n in small_cases():
        iota = np.arange(n, dtype=np.uint32)
        assert _passes(pattern, n, True, "value-is-index", values=iota), (pattern, n)
        if n >= 2:
            assert not _passes(pattern, n, True, "value-is-index"), (pattern, n)


def test_the_second_sort_meets_the_high_words_in_the_order_of_the_low_words():
    keys = np.array([0x0000000300000002, 0x0000000100000003, 0x0000000200000001, 0x0000000400000001], np.uint64)
    assert model.second_sort_keys(keys).tolist() == [2, 4, 3, 1]
    n = 300_001
    rng = np.random.default_rng(7)
    constant = model.make_keys64("high-constant", n, rng)
    assert model.second_sort_verdict(constant, "msd", 10, 18432) == plan_model.VERDICT_MSD_SORTED
    assert model.second_sort_verdict(constant, "hybrid-8") == plan_model.VERDICT_HYBRID_DECLINED   # no byte varies
    assert model.second_sort_verdict(model.make_keys64("low-constant", n, rng), "hybrid-8") == plan_model.VERDICT_HYBRID_RUNS
    assert model.second_sort_verdict(model.make_keys64("uniform", n, rng), "msd", 10, 18432) == plan_model.VERDICT_MSD_RUNS
    assert model.second_sort_verdict(model.make_keys64("8-distinct", n, rng), "msd", 10, 18432) == plan_model.VERDICT_NONE
