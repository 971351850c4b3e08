"""GPU tests of the segmented sort by a bit range (vrdxHipCmdSortSegmentedBits[KeyValue],
vulkan_radix_sort_amd.sort_segments_bits): every segment must come out stably sorted by the field
f(k) = (k >> begin) & (2^(end - begin) - 1) with the keys whole and the values with their keys -- against
np.lexsort((f(keys), segment id)) over the whole call, bit for bit -- whatever size class the device put the segment in, with
both rankings, and nothing touched outside the segments.  The cases are those of tests/segmented_bits_cases.py, whose model
(checked without a GPU) shows which kernel mistakes they tell apart."""
import numpy as np
import pytest

import segmented_cases
from guarded_call import ballot_sorter, sorter, to_device, to_host, torch_mod  # noqa: F401
from segmented_bits_cases import (BUILDERS, EMPTY_RANGE, FULL_RANGE, PASS_CASES, PASS_SIZES, RANGES, case_inputs, check,  # noqa: F401
                                  expected, make_keys, mixed_offsets, payload, run_segmented_bits)
from segmented_cases import GUARD

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ranking", ["atomic", "ballot"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_every_size_class_in_one_call(torch_mod, sorter, ballot_sorter, ranking, builder):
    """Segments of 0 ... 36865 elements (both in-LDS kernels at their edges; the large kernel with one tile plus one key, two
    full tiles, three tiles with a ragged last one) shuffled into one call with untouched elements in front and behind,
    every range, keys-only and key+value, every buffer at a non-zero offset."""
    s = sorter if ranking == "atomic" else ballot_sorter
    for begin, end in RANGES:
        keys, values, offsets = case_inputs(builder, begin, end)
        want = expected(keys, values, offsets, len(keys), begin, end)
        gk, _, _ = run_segmented_bits(torch_mod, s, keys, offsets, begin, end, keys_off=12, offsets_off=8, storage_off=48)
        check(gk, None, keys, None, offsets, begin, end, want=want)
        gk, gv, _ = run_segmented_bits(torch_mod, s, keys, offsets, begin, end, values, keys_off=4, values_off=20,
                                       offsets_off=4, storage_off=16)
        check(gk, gv, keys, values, offsets, begin, end, want=want)
    assert s.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


def _scratch_stays_inside(storage, requirement, begin_index, end_index, arrays):
    """The storage was filled with 0xA5 before the call.  What changed: a few words (header, list counters, one list entry)
    and, where a pass ran, the segment's index range [begin_index, end_index) of each scratch array -- `arrays` of them, each
    starting on a 128-byte line.  A changed run longer than that range, or one that cannot lie inside it, is a write
    outside the segment's index range."""
    changed = np.flatnonzero(storage[:requirement].cpu().numpy() != 0xA5)
    if len(changed) == 0:
        return 0
    cuts = np.flatnonzero(np.diff(changed) > 64)   # (the untouched elements around the segment are 300 bytes and more)
    runs = list(zip(changed[np.concatenate([[0], cuts + 1])], changed[np.concatenate([cuts, [len(changed) - 1]])] + 1))
    small = [(a, b) for a, b in runs if b - a <= 64]   # (the header's words; a counter; a list entry)
    large = [(a, b) for a, b in runs if b - a > 64]
    assert len(small) <= 4, runs
    assert len(large) in (0, arrays), runs
    address = storage.data_ptr()
    for a, b in large:
        line = ((address + int(a) - 4 * begin_index) // 128) * 128 - address   # the scratch array's first byte, at the most
        assert int(b) <= line + 4 * end_index, (a, b, line)
    return len(large)


@pytest.mark.parametrize("size", PASS_SIZES)
@pytest.mark.parametrize("ranking", ["atomic", "ballot"])
def test_pass_logic_of_the_large_form(torch_mod, sorter, ballot_sorter, ranking, size):
    """One large segment: one, two, three and four active passes, a constant middle or lowest digit, a one-bit last digit,
    a field that is the same in every key (nothing moves: no pass runs, the scratch stays as it was), and fields that tie
    with the pads.  The result is in the caller's arrays whatever the number of passes, and the scratch arrays are
    written in the segment's index range only."""
    s = sorter if ranking == "atomic" else ballot_sorter
    for builder, (begin, end) in PASS_CASES:
        keys, values, offsets = case_inputs(builder, begin, end, sizes=[size], tag=f"pass/{size}")
        want = expected(keys, values, offsets, len(keys), begin, end)
        lo, hi = int(offsets[0]), int(offsets[1])
        for vals in (None, values):
            gk, gv, storage = run_segmented_bits(torch_mod, s, keys, offsets, begin, end, vals)
            check(gk, gv, keys, vals, offsets, begin, end, want=want)
            n = len(keys)
            requirement = (s.key_value_storage_requirements(n) if vals is not None else s.storage_requirements(n)).size
            walked = _scratch_stays_inside(storage, requirement, lo, hi, 1 if vals is None else 2)
            if builder in ("equal", "ones"):
                assert walked == 0 and np.array_equal(gk, keys), builder   # bit-identical to the input, no pass ran
            else:
                assert walked != 0, (builder, begin, end)


def _compute_units(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("size,begin,end", [(4097, 3, 12), (16385, 7, 24)])
def test_workgroups_that_take_more_than_one_listed_segment(torch_mod, sorter, size, begin, end):
    """2 x CUs + 3 segments of one listed class: the mid and the large launch have at most 2 x CUs workgroups, so some take a
    second segment of their list (the barrier between two segments, the large form's state set up again)."""
    count = 2 * _compute_units(torch_mod) + 3
    grid = min(count, 2 * _compute_units(torch_mod))
    assert count > grid
    rng = np.random.default_rng(size)
    offsets, n = mixed_offsets(rng, [size] * count)
    keys = make_keys("uniform", n, begin, end, rng)
    values = payload(n)
    want = expected(keys, values, offsets, n, begin, end)
    gk, _, _ = run_segmented_bits(torch_mod, sorter, keys, offsets, begin, end)
    check(gk, None, keys, None, offsets, begin, end, want=want)
    gk, gv, _ = run_segmented_bits(torch_mod, sorter, keys, offsets, begin, end, values)
    check(gk, gv, keys, values, offsets, begin, end, want=want)


def test_full_range_is_the_whole_key_segmented_sort(torch_mod, sorter):
    keys, values, offsets = case_inputs("uniform", *FULL_RANGE)
    for vals in (None, values):
        gk, gv, _ = run_segmented_bits(torch_mod, sorter, keys, offsets, *FULL_RANGE, vals)
        wk, wv, _ = segmented_cases.run_segmented(torch_mod, sorter, keys, offsets, vals)
        assert np.array_equal(gk, wk) and (vals is None or np.array_equal(gv, wv))
        ek, ev = segmented_cases.expected(keys, vals, offsets, len(keys))
        assert np.array_equal(gk, ek) and (vals is None or np.array_equal(gv, ev))


def _untouched_call(torch, s, keys, values, offsets, begin, end):
    """a call that must leave keys, values and every byte of the storage as they were; returns the 15 timestamps"""
    import vulkan_radix_sort_amd as vrdx
    pool = vrdx.QueryPool(15)
    gk, gv, storage = run_segmented_bits(torch, s, keys, offsets, begin, end, values, pool=pool, expect_status=None)
    assert np.array_equal(gk, keys) and (values is None or np.array_equal(gv, values))
    n = len(keys)
    requirement = (s.key_value_storage_requirements(n) if values is not None else s.storage_requirements(n)).size
    assert bool((storage[:requirement] == 0xA5).all()), "the call wrote to the storage"
    ts = pool.results_ns()   # all 15 slots readable
    pool.destroy()
    assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:])), ts
    return ts


def test_empty_range_touches_nothing(torch_mod, sorter):
    stream = torch_mod.cuda.current_stream().cuda_stream
    keys, values, offsets = case_inputs("uniform", 3, 12)
    for vals in (None, values):
        _untouched_call(torch_mod, sorter, keys, vals, offsets, *EMPTY_RANGE)
    assert sorter.read_sorter_status(stream) == 0


@pytest.mark.parametrize("begin,end", [(9, 3), (0, 33), (33, 40)])
def test_invalid_ranges_are_refused(torch_mod, sorter, begin, end):
    """keys, values and the whole storage bit-identical, VRDX_HIP_STATUS_ENQUEUE_REFUSED in the sorter's word, all 15 slots
    readable, and the next valid call works"""
    import vulkan_radix_sort_amd as vrdx
    stream = torch_mod.cuda.current_stream().cuda_stream
    keys, values, offsets = case_inputs("uniform", 3, 12)
    sorter.read_sorter_status(stream)   # (clears the word)
    for vals in (None, values):
        _untouched_call(torch_mod, sorter, keys, vals, offsets, begin, end)
        assert sorter.read_sorter_status(stream) == vrdx.STATUS_ENQUEUE_REFUSED
    gk, gv, _ = run_segmented_bits(torch_mod, sorter, keys, offsets, 3, 12, values)
    check(gk, gv, keys, values, offsets, 3, 12)
    assert sorter.read_sorter_status(stream) == 0


@pytest.mark.parametrize("key_value", [False, True])
def test_bad_offsets_leave_their_segments_alone_and_say_so(torch_mod, sorter, key_value):
    """A decreasing pair and a last offset above maxElementCount under a range: those segments are left alone, the valid ones
    sorted by the field, the failure word and the sorter's word carry STATUS_SEGMENTS_INVALID.  The buffers reach 65536
    words behind maxElementCount, so a missing bound check would change the guard band, never touch memory outside an
    allocation."""
    import vulkan_radix_sort_amd as vrdx
    stream = torch_mod.cuda.current_stream().cuda_stream
    assert sorter.read_sorter_status(stream) == 0
    n = 50000
    begin, end = 7, 24
    rng = np.random.default_rng(3)
    keys = make_keys("uniform", n, begin, end, rng)
    values = payload(n) if key_value else None
    # [100, 1100) small, [1100, 21100) large, [21100, 9000) decreasing, [9000, 9000) empty, [9000, n + 5000) beyond the bound
    offsets = np.array([100, 1100, 21100, 9000, 9000, n + 5000], np.uint32)
    gk, gv, _ = run_segmented_bits(torch_mod, sorter, keys, offsets, begin, end, values, guard=65536,
                                   expect_status=vrdx.STATUS_SEGMENTS_INVALID)
    check(gk, gv, keys, values, offsets, begin, end)
    assert np.array_equal(gk[21100:], keys[21100:]) and np.array_equal(gk[:100], keys[:100])
    assert not np.array_equal(gk[100:1100], keys[100:1100]) and not np.array_equal(gk[1100:21100], keys[1100:21100])
    assert sorter.read_sorter_status(stream) & vrdx.STATUS_SEGMENTS_INVALID
    assert sorter.read_sorter_status(stream) == 0  # (reading it cleared it)


@pytest.mark.parametrize("lead", [4, 8, 12])
def test_arrays_at_every_four_byte_alignment(torch_mod, sorter, lead):
    """keys, values and offsets `lead` bytes off a 16-byte boundary, and a 16385-element segment starting at each of the four
    phases of a 16-byte quad (plus one small and one mid segment)"""
    begin, end = 5, 21
    for phase in range(4):
        rng = np.random.default_rng(100 * lead + phase)
        sizes = [40, 16385, 300, 5000, 16385]
        offsets = (phase + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint32)
        assert int(offsets[1]) % 4 == phase and int(offsets[4]) % 4 == (phase + 1) % 4
        n = int(offsets[-1]) + 9
        keys = make_keys("uniform", n, begin, end, rng)
        values = payload(n)
        want = expected(keys, values, offsets, n, begin, end)
        gk, _, _ = run_segmented_bits(torch_mod, sorter, keys, offsets, begin, end, keys_off=lead, offsets_off=lead)
        check(gk, None, keys, None, offsets, begin, end, want=want)
        gk, gv, _ = run_segmented_bits(torch_mod, sorter, keys, offsets, begin, end, values, keys_off=lead,
                                       values_off=(lead + 4) % 16 or 4, offsets_off=lead)
        check(gk, gv, keys, values, offsets, begin, end, want=want)


def test_captured_graph_replays_on_new_keys_and_a_new_segmentation(torch_mod, sorter):
    """One call captured in torch.cuda.graph (a linear graph), segments of all three classes, range [5, 21): replayed on new
    keys, on another segmentation with the same segmentCount, and once more on the first."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    begin, end = 5, 21
    rng = np.random.default_rng(77)
    n = 250_000
    segmentations = [[300] * 30 + [5000] * 10 + [40000] * 3 + [16385] + [0] * 6,
                     [20000] * 8 + [17] * 30 + [9000] * 5 + [3] * 7]
    offsets_list = []
    for sizes in segmentations:
        sizes = list(sizes)
        rng.shuffle(sizes)
        offsets_list.append(np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32))
    assert len({len(o) for o in offsets_list}) == 1 and all(o[-1] <= n for o in offsets_list)
    dk, dv, do = to_device(torch, np.zeros(n, np.uint32)), to_device(torch, np.zeros(n, np.uint32)), to_device(torch, offsets_list[0])
    storage = torch.empty(sorter.key_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
    vrdx.sort_segments_bits(sorter, dk, do, begin, end, values=dv, storage=storage)  # one eager call first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vrdx.sort_segments_bits(sorter, dk, do, begin, end, values=dv, storage=storage)
    values = payload(n)
    for replay, offsets in enumerate([offsets_list[0], offsets_list[0], offsets_list[1], offsets_list[0]]):
        keys = make_keys("uniform" if replay % 2 == 0 else "few", n, begin, end, rng)
        dk.copy_(to_device(torch, keys))
        dv.copy_(to_device(torch, values))
        do.copy_(to_device(torch, offsets))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(to_host(dk), to_host(dv), keys, values, offsets, begin, end)
        assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0


def test_status_is_clear_and_the_plan_verdict_is_none(torch_mod, sorter):
    """a range call behind a whole-key MSD-size sort on the same storage: failure word and sorter's word 0, word 1
    VERDICT_NONE"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    assert sorter.read_sorter_status(stream) == 0
    big = 9_000_017
    assert sorter.describe_plan(big, False).name == "msd"
    rng = np.random.default_rng(9)
    storage = torch.empty(sorter.storage_requirements(big).size + 256, dtype=torch.uint8, device="cuda")
    dk = to_device(torch, rng.integers(0, 1 << 32, size=big, dtype=np.uint64).astype(np.uint32))
    sorter.cmd_sort(stream, big, dk.data_ptr(), 0, storage.data_ptr(), 0)
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_MSD_RUNS
    offsets, n = mixed_offsets(rng, [300, 5000, 20000, 0, 1])
    keys = make_keys("uniform", n, 7, 24, rng)
    gk, _, _ = run_segmented_bits(torch, sorter, keys, offsets, 7, 24, storage=storage)
    check(gk, None, keys, None, offsets, 7, 24)
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_NONE
    assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    assert sorter.read_sorter_status(stream) == 0


def test_query_pool_slots(torch_mod, sorter):
    """fill, small, mid, large; the rest coincide with the large launch's end"""
    import vulkan_radix_sort_amd as vrdx
    rng = np.random.default_rng(15)
    offsets, n = mixed_offsets(rng, [100, 6000, 40000, 2])
    keys = make_keys("uniform", n, 3, 12, rng)
    pool = vrdx.QueryPool(15)
    gk, _, _ = run_segmented_bits(torch_mod, sorter, keys, offsets, 3, 12, pool=pool)
    check(gk, None, keys, None, offsets, 3, 12)
    ts = pool.results_ns(0, 15)
    pool.destroy()
    assert len(ts) == 15 and ts[0] == 0
    assert all(b >= a for a, b in zip(ts[:4], ts[1:5])), ts
    assert all(t == ts[4] for t in ts[4:]) and ts[4] > 0, ts


def test_sort_segments_bits_python_front_end(torch_mod, sorter):
    """tensors, and contiguous views at 4 and 12 mod 16 which the front end hands on as they are"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    begin, end = 7, 24
    rng = np.random.default_rng(14)
    sizes = rng.integers(0, 3000, size=120)
    sizes[::24] = [20001, 4097, 16384, 16385, 4096]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    keys = make_keys("uniform", n, begin, end, rng)
    values = payload(n)
    want = expected(keys, values, offsets, n, begin, end)
    dk, dv, do = to_device(torch, keys), to_device(torch, values), to_device(torch, offsets)
    storage = vrdx.sort_segments_bits(sorter, dk, do, begin, end, values=dv)
    torch.cuda.synchronize()
    check(to_host(dk), to_host(dv), keys, values, offsets, begin, end, want=want)
    assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0
    big = to_device(torch, np.concatenate([np.full(1, GUARD, np.uint32), keys, np.full(64, GUARD, np.uint32)]))
    other = to_device(torch, np.concatenate([np.full(3, GUARD, np.uint32), values, np.full(64, GUARD, np.uint32)]))
    vk, vv = big[1:1 + n], other[3:3 + n]
    assert big.data_ptr() % 16 == 0 and vk.data_ptr() % 16 == 4 and vv.data_ptr() % 16 == 12
    vrdx.sort_segments_bits(sorter, vk, do, begin, end, values=vv, storage=storage)
    torch.cuda.synchronize()
    whole, whole_values = to_host(big), to_host(other)
    check(whole[1:1 + n], whole_values[3:3 + n], keys, values, offsets, begin, end, want=want)
    assert whole[0] == GUARD and bool((whole[1 + n:] == GUARD).all())
    assert bool((whole_values[:3] == GUARD).all()) and bool((whole_values[3 + n:] == GUARD).all())
    keys_only = to_device(torch, np.concatenate([np.full(1, GUARD, np.uint32), keys, np.full(64, GUARD, np.uint32)]))
    vrdx.sort_segments_bits(sorter, keys_only[1:1 + n], do, begin, end)
    torch.cuda.synchronize()
    whole = to_host(keys_only)
    check(whole[1:1 + n], None, keys, None, offsets, begin, end, want=want)
    assert whole[0] == GUARD and bool((whole[1 + n:] == GUARD).all())
