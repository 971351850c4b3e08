"""Without a GPU: the inputs of tests/storage_reuse_cases.py are what their names say.  Every call of CALLS is put through
tests/plan_model.py with the constants the host uses at its bound -- ten bits and msd_capacity() where the MSD plan is
recorded, hybrid_capacity() for the hybrid plan, the ballot sorter's capacity rule (HybridCapacity in vrdx_plan.h: no
bucket beyond 16384, and never the MSD plan) -- and the verdict must be the one the table of CALLS states.  A generator that
changes cannot turn a "declined" call into an "accepted" one, or the other way round, without this file noticing."""
import numpy as np
import pytest

import plan_model as model
import storage_reuse_cases as cases
from test_sort_gpu import MSD_FROM, MSD_HALF_UP_TO, msd_capacity


def test_the_names_are_the_issue_list_and_unique():
    assert len(set(cases.NAMES)) == len(cases.CALLS) == 21
    assert {c.sorter for c in cases.CALLS} == {"atomic", "ballot"}
    assert {c.requirement for c in cases.CALLS} == {"keys", "key-value", "keys64", "key-value64"}
    assert [c.name for c in cases.CALLS if c.failure not in (0, cases.INHERITED)] == ["segmented-invalid"]
    assert [c.name for c in cases.CALLS if c.verdict == cases.INHERITED] == ["empty"]


def test_the_constants_of_the_bounds():
    """The sizes select what the table says: the MSD plan with the half-size bucket kernel at M, at one round and at two
    rounds + 1; the hybrid plan with buckets of 4096 at H for both rankings; nothing but the four passes for the ballot
    sorter at M; one workgroup up to 16384."""
    assert cases.M % 4 == 3
    for n in (cases.M, cases.BLOCK_SUMS_N, cases.TAIL_SPLIT_N):
        assert MSD_FROM <= n <= MSD_HALF_UP_TO and model.hybrid_capacity(n) == 0 and msd_capacity(n, cases.MSD_BITS) == 18432
    assert model.hybrid_capacity(cases.H) == cases.ballot_hybrid_capacity(cases.H) == 4096
    assert cases.ballot_hybrid_capacity(cases.M) == 0
    assert cases.ballot_hybrid_capacity(4_000_000) == 16384 and cases.ballot_hybrid_capacity(4_200_000) == 0
    assert cases.BY_NAME["one-workgroup"].bound == 16384 and cases.BY_NAME["sort64-small"].bound <= 16384
    for c in cases.CALLS:
        if c.count is not None:
            assert 0 < c.count < c.bound, c.name


@pytest.mark.parametrize("name", [c.name for c in cases.CALLS if not cases.is_segmented(c) and c.name != "empty"])
def test_the_model_gives_the_verdict_of_the_table(name):
    call = cases.BY_NAME[name]
    verdict, where = cases.verdict_of(call)
    assert verdict == call.verdict, (name, verdict, where)
    keys, values, _ = cases.inputs_of(call)
    assert len(keys) == call.bound and (values is None or len(values) == call.bound)
    assert keys.dtype == (np.uint64 if cases.is_wide(call) else np.uint32)
    if values is not None:   # random words, never the index
        assert int((values == np.arange(len(values), dtype=np.uint32)).sum()) < 4


def test_the_uniform_msd_calls_scatter_by_the_top_bits():
    """uniform keys: the window lies at the top, also under the small device-side count"""
    for name in ("msd-runs-keys", "msd-runs-pairs", "msd-indirect-small"):
        assert cases.verdict_of(cases.BY_NAME[name]) == (model.VERDICT_MSD_RUNS, 32 - cases.MSD_BITS), name


def test_the_declined_calls_are_declined_for_the_reason_in_their_name():
    """decline_msd's keys: one bucket beyond the capacity (whether the sample or the spine finds it).  The keys with two
    constant bytes: the top byte varies, so the window is at the top, where 256 of its 1024 buckets hold all the keys."""
    for name in ("msd-declined-keys", "msd-indirect-declined", "tail-split", "block-sums"):
        call = cases.BY_NAME[name]
        keys = cases.inputs_of(call)[0][:cases.sorted_count(call)]
        top = np.bincount(keys >> np.uint32(32 - cases.MSD_BITS), minlength=1 << cases.MSD_BITS)
        assert int(top.max()) >= 40000 > msd_capacity(call.bound, cases.MSD_BITS), name
    skips = cases.inputs_of(cases.BY_NAME["msd-declined-pairs-skips"])[0]
    assert bool(((skips >> np.uint32(8)) & np.uint32(0xFFFF) == 0xA5C3).all())     # bytes 1 and 2 are constant ...
    assert len(np.unique(skips & np.uint32(0xFF))) == 256 and len(np.unique(skips >> np.uint32(24))) == 256   # ... 0 and 3 are not
    window = model.msd_window(skips, cases.M, cases.MSD_BITS, 18432)
    assert window["lowest"] == 22 and window["mode"] == model.MODE_PLAN   # the sample lets it through: the spine declines
    top = np.bincount(skips >> np.uint32(22), minlength=1024)
    assert int((top != 0).sum()) == 256 and int(top.max()) > 18432


def test_the_hybrid_calls_sit_at_the_capacity():
    heavy = cases.inputs_of(cases.BY_NAME["hybrid-declined"])[0]
    assert int(np.bincount(heavy >> np.uint32(24), minlength=256).max()) == 4096 + 1
    for name in ("hybrid-runs", "ballot-hybrid"):
        keys = cases.inputs_of(cases.BY_NAME[name])[0]
        assert cases.verdict_of(cases.BY_NAME[name]) == (model.VERDICT_HYBRID_RUNS, 3)
        assert int(np.bincount(keys >> np.uint32(24), minlength=256).max()) <= 4096
    # the 64-bit calls: the second inner sort scatters the high words by their top byte (63-bit keys) and by byte 1 (a
    # sixteen-bit tile id)
    assert cases.verdict_of(cases.BY_NAME["sort64-pairs"]) == (model.VERDICT_HYBRID_RUNS, 3)
    assert cases.verdict_of(cases.BY_NAME["sort64-indirect"]) == (model.VERDICT_HYBRID_RUNS, 1)


def test_the_one_workgroup_call_has_eight_bit_keys():
    keys = cases.inputs_of(cases.BY_NAME["one-workgroup"])[0]
    assert int(keys.max()) < 256 and len(np.unique(keys)) == 256


@pytest.mark.parametrize("name,mid_max", [("segmented", 16384), ("segmented64", 16384)])
def test_the_segmented_calls_hold_every_size_class(name, mid_max):
    """empty, in-LDS with 256 threads (<= 4096), in-LDS with 1024 threads, through memory -- at least one segment each, inside
    the bound, the offsets increasing"""
    call = cases.BY_NAME[name]
    _, _, offsets = cases.inputs_of(call)
    sizes = np.diff(offsets.astype(np.int64))
    assert len(sizes) == len(cases.SEGMENT_SIZES) and (sizes >= 0).all() and int(offsets[-1]) <= call.bound
    assert (sizes == 0).any() and ((sizes > 1) & (sizes <= 4096)).any()
    assert ((sizes > 4096) & (sizes <= mid_max)).any() and (sizes > mid_max).any()


def test_the_invalid_offsets_are_invalid_twice():
    call = cases.BY_NAME["segmented-invalid"]
    offsets = cases.inputs_of(call)[2].astype(np.int64)
    assert (np.diff(offsets) < 0).sum() == 1 and int(offsets[-1]) > call.bound
    assert call.failure == cases.STATUS_SEGMENTS_INVALID


def test_the_references_leave_the_tail_alone():
    """expected_of(): sorted up to the count, the input behind it (small calls only: the large ones are sorted on the GPU
    machine, once)"""
    for name in ("one-workgroup", "sort64-small", "sort64-indirect", "segmented-invalid"):
        call = cases.BY_NAME[name]
        keys, values, _ = cases.inputs_of(call)
        want_keys, want_values = cases.expected_of(call)
        n = cases.sorted_count(call)
        assert np.array_equal(want_keys[n:], keys[n:]) and np.array_equal(np.sort(want_keys), np.sort(keys))
        if not cases.is_segmented(call):
            assert bool((want_keys[1:n] >= want_keys[:n - 1]).all())
        if values is not None:
            pairs = set(zip(keys.tolist(), values.tolist()))
            assert set(zip(want_keys.tolist(), want_values.tolist())) == pairs
    assert len(cases.padded(keys)) == len(keys) + cases.GUARD_ELEMENTS
