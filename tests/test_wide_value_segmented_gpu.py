"""The segmented sort of 32-bit keys with 64-bit values on the GPU (vrdxHipCmdWideValueSortSegmented, `-m gpu`): every call
between guard bytes (tests/wide_segmented_guarded_call.py), results compared bit for bit with the reference of
tests/wide_value_segmented_cases.py -- np.lexsort((keys, segment id)) -- on the cases that file's model is checked on without
a GPU; values are never the index.  Both rankings through the `sorter` / `ballot_sorter` fixtures."""
import numpy as np
import pytest

import vulkan_radix_sort_amd as vrdx
import wide_value_segmented_cases as cases
from wide_segmented_guarded_call import (ballot_sorter, poisoned_storage, sorter, to_device, to_host, torch_mod,  # noqa: F401
                                         wide_segmented_call)

pytestmark = pytest.mark.gpu

INVALID = vrdx.STATUS_SEGMENTS_INVALID


def _check(got, keys, values, offsets, what, bound=None):
    want_keys, want_values = cases.expected(keys, values, offsets, bound)
    bad = np.flatnonzero(got.keys != want_keys)
    assert bad.size == 0, f"{what}: {bad.size} keys differ, first at {bad[:8].tolist()}"
    bad = np.flatnonzero(got.values != want_values)
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:8].tolist()}"


@pytest.fixture(scope="module")
def class_cases():
    """(class, builder) -> (keys, values, offsets): built once, shared by both rankings, never changed"""
    return {(c, b): cases.class_case(c, b) for c in cases.SIZES for b in cases.BUILDERS}


@pytest.mark.parametrize("builder", cases.BUILDERS)
@pytest.mark.parametrize("size_class", tuple(cases.SIZES))
@pytest.mark.parametrize("which", ["atomic", "ballot"])
def test_every_size_of_a_class_as_neighbouring_segments(torch_mod, sorter, ballot_sorter, class_cases, which, size_class, builder):
    keys, values, offsets = class_cases[size_class, builder]
    got = wide_segmented_call(torch_mod, ballot_sorter if which == "ballot" else sorter, keys, values, offsets)
    _check(got, keys, values, offsets, f"{size_class}, {builder}, {which}")


def test_all_three_classes_in_one_call_and_untouched_elements(torch_mod, sorter):
    rng = np.random.default_rng(2)
    sizes = (9000, 1, 4097, 0, 300, 8193, 2, 8192, 4096, 1)
    offsets = cases.offsets_of(sizes, lead=11)
    n = int(offsets[-1]) + 13
    keys, values = cases.make_keys("random", n, rng), cases.make_values(n, rng)
    got = wide_segmented_call(torch_mod, sorter, keys, values, offsets)
    _check(got, keys, values, offsets, "mixed classes")
    assert np.array_equal(got.keys[:11], keys[:11]) and np.array_equal(got.values[-13:], values[-13:])


def _compute_units(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("which", ["atomic", "ballot"])
def test_more_tiny_segments_than_the_small_grid(torch_mod, sorter, ballot_sorter, which):
    """2^20 + 300 segments of 0 to 3 elements: the workgroups beyond the grid's cap take a second segment"""
    rng = np.random.default_rng(3)
    sizes = rng.integers(0, 4, size=(1 << 20) + 300)
    offsets = cases.offsets_of(sizes)
    n = int(offsets[-1])
    keys, values = cases.make_keys("two_valued", n, rng), cases.make_values(n, rng)
    got = wide_segmented_call(torch_mod, ballot_sorter if which == "ballot" else sorter, keys, values, offsets)
    _check(got, keys, values, offsets, "tiny segments")


@pytest.mark.parametrize("which", ["atomic", "ballot"])
def test_more_mid_segments_than_workgroups(torch_mod, sorter, ballot_sorter, which):
    """2 x CUs + 3 segments of 4097 ... 8192 elements: every workgroup of the mid launch sorts two or three"""
    rng = np.random.default_rng(4)
    count = 2 * _compute_units(torch_mod) + 3
    sizes = rng.integers(4097, 8193, size=count)
    sizes[:3] = (4097, 8192, 4352)
    offsets = cases.offsets_of(sizes)
    n = int(offsets[-1])
    builders = ("random", "byte1", "equal", "ones_third", "bytes02")
    keys = np.concatenate([cases.make_keys(builders[i % len(builders)], int(s), rng) for i, s in enumerate(sizes)])
    values = cases.make_values(n, rng)
    got = wide_segmented_call(torch_mod, ballot_sorter if which == "ballot" else sorter, keys, values, offsets)
    _check(got, keys, values, offsets, "mid segments")


@pytest.mark.parametrize("which", ["atomic", "ballot"])
def test_more_large_segments_than_workgroups(torch_mod, sorter, ballot_sorter, which):
    """CUs + 2 segments of more than 8192 elements with mixed pass patterns (none, even, odd, all four): two workgroups sort a
    second segment behind a copy back, behind an even pass count and behind a segment with nothing to do"""
    rng = np.random.default_rng(5)
    count = _compute_units(torch_mod) + 2
    sizes = rng.integers(8193, 8700, size=count)
    offsets = cases.offsets_of(sizes)
    n = int(offsets[-1])
    builders = ("bytes012", "equal", "bytes02", "random", "byte3", "ones_third")
    keys = np.concatenate([cases.make_keys(builders[i % len(builders)], int(s), rng) for i, s in enumerate(sizes)])
    values = cases.make_values(n, rng)
    got = wide_segmented_call(torch_mod, ballot_sorter if which == "ballot" else sorter, keys, values, offsets)
    _check(got, keys, values, offsets, "large segments")


@pytest.mark.parametrize("size,extra", [(4097, 0), (8193, 0), (8193, 4096)])
def test_a_list_filled_to_its_last_slot(torch_mod, sorter, size, extra):
    """five segments of the smallest size of a class in 5 x that size (+ extra < one more) elements: the list's cap is 5"""
    rng = np.random.default_rng(size + extra)
    offsets = cases.offsets_of([size] * 5)
    n = 5 * size + extra
    assert n // size == 5
    keys, values = cases.make_keys("random", n, rng), cases.make_values(n, rng)
    got = wide_segmented_call(torch_mod, sorter, keys, values, offsets)
    _check(got, keys, values, offsets, f"five segments of {size}")


def test_a_decreasing_pair_and_an_end_behind_the_bound(torch_mod, sorter, ballot_sorter):
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(6)
    n = 30000
    keys, values = cases.make_keys("random", n, rng), cases.make_values(n, rng)
    for s in (sorter, ballot_sorter):
        s.read_sorter_status(stream)   # (reading clears the sorter's word)
        # (9000, 19000) large and valid | (19000, 100) decreasing | (100, 5000) mid and valid | (5000, 5003) valid
        offsets = np.array([9000, 19000, 100, 5000, 5003], np.uint32)
        got = wide_segmented_call(torch, s, keys, values, offsets, expect_status=INVALID, sticky=INVALID)
        _check(got, keys, values, offsets, "a decreasing pair")
        assert not np.array_equal(got.keys[100:5000], keys[100:5000]) and np.array_equal(got.keys[19000:], keys[19000:])
        # an end behind maxElementCount: that segment is left alone, the others are sorted
        offsets = np.array([0, 4000, 13000, 29000, n + 5], np.uint32)
        got = wide_segmented_call(torch, s, keys, values, offsets, expect_status=INVALID, sticky=INVALID)
        _check(got, keys, values, offsets, "an end behind the bound")
        assert np.array_equal(got.keys[29000:], keys[29000:]) and np.array_equal(got.values[29000:], values[29000:])
        # ... and with a bound below the arrays' length: nothing from the bound on is written
        offsets = np.array([0, 4000, 13000, 20000, 25000], np.uint32)
        got = wide_segmented_call(torch, s, keys, values, offsets, count=20000, expect_status=INVALID, sticky=INVALID)
        _check(got, keys, values, offsets, "a segment behind a smaller bound", bound=20000)
        assert np.array_equal(got.keys[20000:], keys[20000:])
        # monotone offsets raise nothing
        got = wide_segmented_call(torch, s, keys, values, np.array([0, 10, 10, 9000], np.uint32), expect_status=0, sticky=0)


@pytest.mark.parametrize("size", [4097, 8193])
def test_overlapping_segments_that_would_overfill_a_list(torch_mod, sorter, size):
    """more listed segments than N / size: the slots beyond the cap are dropped, nothing is written outside the arrays or the
    storage, the bit is raised in both words, and the segment no other overlaps is sorted"""
    torch = torch_mod
    rng = np.random.default_rng(size)
    n = 2 * size + 1500
    cap = n // size
    assert cap == 2
    # one disjoint segment near the end first, then six segments of `size` elements, each starting 100 behind the one before:
    # every second pair decreases, so no pair but these seven is a segment
    offsets = [n - 900, n - 10]
    for i in range(6):
        offsets += [100 * i, 100 * i + size]
    offsets = np.array(offsets, np.uint32)
    assert [(b, e) for b, e in cases.valid_segments(offsets, n)] == [(n - 900, n - 10)] + [(100 * i, 100 * i + size) for i in range(6)]
    assert int(offsets.max()) <= n and 500 + size < n - 900
    keys, values = cases.make_keys("random", n, rng), cases.make_values(n, rng)
    sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream)
    got = wide_segmented_call(torch, sorter, keys, values, offsets, expect_status=INVALID, sticky=INVALID)
    order = np.argsort(keys[n - 900:n - 10], kind="stable")
    assert np.array_equal(got.keys[n - 900:n - 10], keys[n - 900:n - 10][order])
    assert np.array_equal(got.values[n - 900:n - 10], values[n - 900:n - 10][order])
    for lo, hi in ((500 + size, n - 900), (n - 10, n)):   # what no segment covers
        assert np.array_equal(got.keys[lo:hi], keys[lo:hi]) and np.array_equal(got.values[lo:hi], values[lo:hi])


@pytest.mark.parametrize("keys_off,storage_off", [(4, 16), (8, 48), (12, 16)])
def test_alignment(torch_mod, sorter, keys_off, storage_off):
    rng = np.random.default_rng(keys_off)
    sizes = (4097, 300, 8195, 3)
    offsets = cases.offsets_of(sizes, lead=1)
    n = int(offsets[-1]) + 2
    keys, values = cases.make_keys("random", n, rng), cases.make_values(n, rng)
    got = wide_segmented_call(torch_mod, sorter, keys, values, offsets, keys_off=keys_off, values_off=8, offsets_off=4,
                              storage_off=storage_off)
    _check(got, keys, values, offsets, f"keys at {keys_off} mod 16, values at 8, offsets at 4, storage at {storage_off}")


def test_timestamps(torch_mod, sorter):
    for n in (4096, 8192, 20000):
        rng = np.random.default_rng(n)
        keys, values = cases.make_keys("random", n, rng), cases.make_values(n, rng)
        offsets = np.array([0, n // 3, n], np.uint32)
        pool = vrdx.QueryPool(15)
        _check(wide_segmented_call(torch_mod, sorter, keys, values, offsets, pool=pool), keys, values, offsets, f"n = {n}")
        ns = pool.results_ns()
        pool.destroy()
        assert len(ns) == 15 and ns[0] == 0 and all(a <= b for a, b in zip(ns, ns[1:])), (n, ns)
        assert ns[14] > 0 and all(ns[i] == ns[4] for i in range(5, 15)), (n, ns)   # the later slots coincide with slot 4
        if n < 4097:
            assert ns[2] == ns[3] == ns[4], (n, ns)   # no mid and no large launch under this bound
        elif n < 8193:
            assert ns[3] == ns[4], (n, ns)            # no large launch


def test_empty_calls_record_only_the_timestamps(torch_mod, sorter):
    torch = torch_mod
    rng = np.random.default_rng(8)
    keys, values = cases.make_keys("random", 100, rng), cases.make_values(100, rng)
    for count, offsets in ((100, np.array([0], np.uint32)), (0, np.array([0, 50, 100], np.uint32))):
        pool = vrdx.QueryPool(15)
        got = wide_segmented_call(torch, sorter, keys, values, offsets, count=count, pool=pool, keep_before=True)
        ns = pool.results_ns()
        pool.destroy()
        assert len(ns) == 15 and all(a <= b for a, b in zip(ns, ns[1:]))
        assert np.array_equal(got.keys, keys) and np.array_equal(got.values, values)
        assert torch.equal(got.storage, got.before)


def test_a_count_beyond_the_clamp_raises_the_bit(torch_mod, sorter):
    """(with no segment nothing is recorded, so no storage of that size is needed)"""
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    sorter.read_sorter_status(stream)
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    sorter.cmd_wide_value_sort_segmented(stream, 0xFFFFFFFF, 0, small.data_ptr(), 0, small.data_ptr(), 0, small.data_ptr(), 0,
                                         small.data_ptr(), 0)
    torch.cuda.synchronize()
    assert sorter.read_sorter_status(stream) == vrdx.STATUS_COUNT_CLAMPED
    assert int(small.sum().item()) == 0


def test_graph_replay_on_another_segmentation(torch_mod, sorter):
    """one capture, the same segmentCount, segments that change class between the replays"""
    torch = torch_mod
    n = 60000
    segmentations = ((100, 5000, 9000, 20000, 3, 8192, 4096), (9000, 100, 8193, 3, 20000, 0, 5000), (3, 8192, 2, 8193, 1, 4097, 30000))
    rng = np.random.default_rng(9)
    dk = torch.zeros(n, dtype=torch.int32, device="cuda")
    dv = torch.zeros(n, dtype=torch.int64, device="cuda")
    do = torch.zeros(8, dtype=torch.int32, device="cuda")
    storage = torch.empty(sorter.wide_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        sorter.cmd_wide_value_sort_segmented(torch.cuda.current_stream().cuda_stream, n, 7, do.data_ptr(), 0, dk.data_ptr(), 0,
                                             dv.data_ptr(), 0, storage.data_ptr(), 0, None, 0)
    for sizes in segmentations:
        offsets = cases.offsets_of(sizes, lead=17)
        assert len(offsets) == 8 and int(offsets[-1]) <= n
        keys, values = cases.make_keys("random", n, rng), cases.make_values(n, rng)
        dk.copy_(torch.from_numpy(keys.view(np.int32)))
        dv.copy_(torch.from_numpy(values.view(np.int64)))
        do.copy_(torch.from_numpy(offsets.view(np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        want_keys, want_values = cases.expected(keys, values, offsets)
        assert np.array_equal(dk.cpu().numpy().view(np.uint32), want_keys), sizes
        assert np.array_equal(dv.cpu().numpy().view(np.uint64), want_values), sizes
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0


def test_storage_reuse_with_the_flat_call(torch_mod, sorter):
    """a segmented call on storage a vrdxHipCmdWideValueSort of the gather form left behind, and the reverse"""
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(10)
    n = 30000
    assert sorter.describe_wide_value_sort_plan(n).name == "gather"
    storage = poisoned_storage(torch, sorter.wide_value_storage_requirements(n).size)
    keys = cases.make_keys("random", n, rng)
    offsets = cases.offsets_of((9000, 4097, 50, 16000), lead=3)

    def flat():
        values = cases.make_values(n, rng)
        dk, dv = to_device(torch, keys), to_device(torch, values)
        sorter.cmd_wide_value_sort(stream, n, dk.data_ptr(), 0, dv.data_ptr(), 0, storage.data_ptr(), 0)
        torch.cuda.synchronize()
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(to_host(dk), keys[order]) and np.array_equal(to_host(dv), values[order])

    def segmented():
        values = cases.make_values(n, rng)
        _check(wide_segmented_call(torch, sorter, keys, values, offsets, storage=storage), keys, values, offsets, "reused storage")

    for step in (flat, segmented, flat, segmented, segmented, flat):
        step()
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0


@pytest.mark.parametrize("rows,columns", [(37, 300), (5, 4100), (3, 9000)])
@pytest.mark.parametrize("dtype", ["int64", "float64"])
def test_front_end_against_a_stable_torch_sort_per_row(torch_mod, sorter, rows, columns, dtype):
    torch = torch_mod
    gen = torch.Generator(device="cuda").manual_seed(rows)
    keys = torch.randint(-2**31, 2**31, (rows, columns), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32)
    keys[:, ::3] = -12345   # ties
    bits = torch.randint(-2**62, 2**62, (rows, columns), dtype=torch.int64, device="cuda", generator=gen)
    values = bits if dtype == "int64" else bits.to(torch.float64)
    as_unsigned = keys.to(torch.int64) & 0xFFFFFFFF
    want_keys, index = torch.sort(as_unsigned, dim=1, stable=True)
    want_values = torch.gather(values, 1, index)
    k, v = keys.clone().reshape(-1), values.clone().reshape(-1)
    offsets = torch.arange(0, rows * columns + 1, columns, dtype=torch.int32, device="cuda")
    storage = vrdx.sort_segments_key_value64(sorter, k, offsets, v)
    torch.cuda.synchronize()
    assert storage.numel() == sorter.wide_value_storage_requirements(rows * columns).size
    assert torch.equal(k.reshape(rows, columns).to(torch.int64) & 0xFFFFFFFF, want_keys)
    assert torch.equal(v.view(torch.int64).reshape(rows, columns), want_values.view(torch.int64))
    # on the caller's storage, which comes back
    k2, v2 = keys.clone().reshape(-1), values.clone().reshape(-1)
    assert vrdx.sort_segments_key_value64(sorter, k2, offsets, v2, storage=storage) is storage
    torch.cuda.synchronize()
    assert torch.equal(k2, k) and torch.equal(v2.view(torch.int64), v.view(torch.int64))
