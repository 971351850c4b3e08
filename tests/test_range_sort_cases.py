"""Without a GPU: the numpy model of the chunked range sort (tests/range_sort_cases.py) on the cases the GPU tests run, for a
device of few CUs (the cases are functions of the CU count, and so are the model's chunks: base[] between the tiles of a
chunk only matters from cus * 16384 + 1 elements on).  The clean model equals np.argsort(field, kind="stable") on every case;
every planted fault changes the result of at least one of them -- but for the pad digit, which tiles of a multiple of 256
keys make harmless (test_the_pad_digit_only_matters_in_tiles_that_are_no_multiple_of_256 says why, and shows it)."""
import numpy as np
import pytest

import range_sort_cases as cases

CUS = 4   # the GPU tests take the device's; the model's work grows with it


def _inputs(n, builder, r):
    return cases.case_inputs(builder, n, *r)


@pytest.fixture(scope="module")
def clean():
    """every GPU parity case through the clean model: (case, keys, values, want, got, info)"""
    out = []
    for n, builder, r in cases.gpu_cases(CUS):
        keys, values = _inputs(n, builder, r)
        want = cases.reference(keys, values, *r)
        got_keys, got_values, info = cases.sort_range_model(keys, values, *r, CUS)
        out.append(((n, builder, r), keys, values, want, (got_keys, got_values), info))
    return out


def test_the_clean_model_is_the_stable_argsort_of_the_field(clean):
    for case, _, _, want, got, info in clean:
        assert info["form"] == "chunked", case
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case


def test_the_cases_reach_what_they_are_there_for(clean):
    seen = {(case, info["active"], info["copy_back"], info["chunks"], info["chunk_keys"], info["scratch_written"])
            for case, _, _, _, _, info in clean}
    # three digits of which the middle one is constant: two active passes, no copy back
    assert any(case[1] == "const-mid" and case[2] == (4, 28) and active == 0b101 and not copy for case, active, copy, *_ in seen)
    # two digits of which the low one is constant: one active pass, a copy back
    assert any(case[1] == "const-low" and case[2] == (8, 24) and active == 0b10 and copy for case, active, copy, *_ in seen)
    # an equal field: no active pass, and the scratch arrays are never written
    for case, active, copy, _, _, written in seen:
        if case[1] == "equal":
            assert active == 0 and not copy and not written, case
    # one, two and three tiles per chunk; a last chunk that is not full; more than one chunk everywhere
    tiles = {-(-keys // cases.TILE) for _, _, _, _, keys, _ in seen}
    assert {1, 2, 3} <= tiles
    assert all(chunks >= 2 for _, _, _, chunks, _, _ in seen)
    assert all(keys % 256 == 0 and keys >= cases.CHUNK_MIN for _, _, _, _, keys, _ in seen)


@pytest.mark.parametrize("fault", [f for f in cases.FAULTS if f not in ("pad-digit-255", "scan-by-bound")])
def test_every_fault_changes_a_case_the_gpu_tests_run(clean, fault):
    changed = []
    for case, keys, values, want, _, _ in clean:
        got_keys, got_values, _ = cases.sort_range_model(keys, values, *case[2], CUS, fault=fault)
        if not (np.array_equal(got_keys, want[0]) and np.array_equal(got_values, want[1])):
            changed.append(case)
    assert changed, fault
    if fault == "base-not-advanced":   # only chunks of two tiles and more: from cus * 16384 + 1 elements on
        assert min(n for n, _, _ in changed) > CUS * cases.TILE


def test_the_scan_chunking_by_the_bound_changes_an_indirect_case():
    """the indirect cases of the GPU tests: one bound, seven counts; a scan that takes the bound's chunks leaves the rows of the
    count's chunks as they were counted"""
    bound = cases.indirect_bound(CUS)
    begin, end = 5, 14
    keys, values = cases.case_inputs("uniform", bound + 8, begin, end)
    changed = []
    for name in cases.INDIRECT_COUNTS:
        count = cases.indirect_count(name, bound)
        want = cases.reference(keys, values, begin, end, min(count, bound))
        got = cases.sort_range_model(keys, values, begin, end, CUS, count=count, bound=bound)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        assert np.array_equal(got[0][min(count, bound):], keys[min(count, bound):]), name
        bad = cases.sort_range_model(keys, values, begin, end, CUS, count=count, bound=bound, fault="scan-by-bound")
        if not (np.array_equal(bad[0], want[0]) and np.array_equal(bad[1], want[1])):
            changed.append(name)
    assert "16385" in changed, changed   # two chunks by the count, one by the bound


def test_the_pad_digit_only_matters_in_tiles_that_are_no_multiple_of_256(clean):
    """A tile's pads are counted in one bin and taken out of it again before base[] advances; taken out of bin 255 of a digit
    of fewer than 8 bits they would stay in the bin of all ones and push base[] of that digit too far -- for the NEXT tile of
    the chunk.  Tiles hold a multiple of 256 keys, so the only tile of a chunk with pads is its last one, behind which base[]
    is never read (and chunks hold a multiple of 256 keys, so that tile is the array's last): the fault cannot show in the
    chunked form as built, on any input.  With tiles of any other length it does."""
    for case, keys, values, want, _, _ in clean:
        got_keys, got_values, _ = cases.sort_range_model(keys, values, *case[2], CUS, fault="pad-digit-255")
        assert np.array_equal(got_keys, want[0]) and np.array_equal(got_values, want[1]), case
    n, r = 2 * CUS * cases.TILE + 257, (5, 14)   # the last digit one bit wide
    keys, values = cases.case_inputs("uniform", n, *r)
    want = cases.reference(keys, values, *r)
    ragged = cases.sort_range_model(keys, values, *r, CUS, tile=5000)
    assert np.array_equal(ragged[0], want[0]) and np.array_equal(ragged[1], want[1])
    bad = cases.sort_range_model(keys, values, *r, CUS, fault="pad-digit-255", tile=5000)
    assert not np.array_equal(bad[0], want[0])


def test_small_counts_and_other_forms():
    keys, values = cases.case_inputs("uniform", 20000, 3, 12)
    for r, form in ((cases.EMPTY_RANGE, "none"), (cases.FULL_RANGE, "whole-key"), (cases.INVALID_RANGES[0], "none")):
        got = cases.sort_range_model(keys, values, *r, CUS)
        assert got[2]["form"] == form
        if form == "none":
            assert np.array_equal(got[0], keys) and np.array_equal(got[1], values)
    small = cases.sort_range_model(keys[:16384], values[:16384], 3, 12, CUS)
    assert small[2]["form"] == "one-workgroup" and np.array_equal(small[0], cases.reference(keys[:16384], None, 3, 12)[0])
    # the chunk formula: a count of 5 under a large bound is one short chunk
    assert cases.chunk_keys(5, 256) == 256 and cases.chunk_keys(16385, 256) == 8448 and cases.chunk_keys(1 << 23, 256) == 32768
