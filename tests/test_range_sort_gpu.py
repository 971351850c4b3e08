"""GPU tests of the range sorts at every size (vrdxHipCmdRangeSort[KeyValue][Indirect]): every result bit for bit against
np.argsort(field, kind="stable") applied to keys and values (range_sort_cases.reference), on keys whose bits outside the range
are random and values that are never the index.  Every call goes through guarded_call: guard bytes around keys, values and
count word, poisoned storage with bands in front of the offset and behind the requirement, vrdxHipReadStatus 0 afterwards.  The
sizes follow the device's CU count as vrdxHipDescribeRangeSortPlan reports it: either side of one chunk of 8192 keys per CU,
the first chunks of two tiles, chunks of three.  tests/test_range_sort_cases.py runs the same cases through a numpy model
with planted faults."""
import numpy as np
import pytest

import range_sort_cases as cases
import sort_bits_cases
from guarded_call import guarded_call
from range_guarded_call import (POISON_BYTE, ballot_sorter, range_call, sorter, to_device, to_host, torch_mod)  # noqa: F401
from segmented_cases import GUARD

pytestmark = pytest.mark.gpu

MAX_ELEMENTS = 0x3FFFFFFC
LARGE = range(5)   # indices into cases.large_sizes(cus)


@pytest.fixture(scope="module")
def cus(sorter):
    """the device's CU count: the chunks of the largest sort there is"""
    info = sorter.describe_range_sort_plan(MAX_ELEMENTS, False, 0, 8)
    assert info.name == "chunked" and info.chunks >= 1
    return info.chunks


def run(torch, sorter, keys, values, begin, end, count=None, indirect=False, bound=None, lead=0, **kw):
    """One vrdxHipCmdRangeSort* call.  keys / values: the FULL host buffers, of which the first `count` (default: all) are
    sorted; indirect: the count travels in a device word and `bound` (default: the buffer's length) is maxElementCount.
    lead: the arrays start that many words past a 16-byte boundary."""
    n = len(keys) if count is None else count
    bound = (len(keys) if indirect else n) if bound is None else bound
    assert indirect or bound == n
    return range_call(torch, sorter, keys, values, begin, end, count=bound, device_count=n if indirect else None,
                      keys_off=4 * lead, values_off=4 * lead, indirect_off=4, **kw)


def check(torch, sorter, keys, values, begin, end, want=None, modes=(False, True), **kw):
    """keys-only and key+value against the reference (computed once for both)"""
    count, bound = kw.get("count"), kw.get("bound")
    n = len(keys) if count is None else count
    n = n if bound is None else min(n, bound)
    want_keys, want_values = want if want is not None else cases.reference(keys, values, begin, end, n)
    for key_value in modes:
        got = run(torch, sorter, keys, values if key_value else None, begin, end, **kw)
        assert np.array_equal(got.keys, want_keys), ("keys", key_value, len(keys), begin, end)
        assert not key_value or np.array_equal(got.values, want_values), ("values", len(keys), begin, end)


def scratch_from(chunks):
    """a byte offset behind which the storage holds nothing but the two scratch arrays: header, totals, the table of counts
    and their two pads of less than 128 bytes"""
    return 16 + 4096 + 128 + 1024 * chunks + 128


@pytest.mark.parametrize("begin,end", cases.RANGES)
def test_up_to_16384_elements_it_is_the_sort_bits_call(torch_mod, sorter, begin, end):
    """the same launch: keys, values and every byte of the storage as vrdxHipCmdSortBits* leaves them"""
    for n in (4097, 16384):
        keys, values = cases.case_inputs("uniform", n, begin, end)
        for vals in (None, values):
            theirs = guarded_call(torch_mod, sorter, keys, vals, bit_range=(begin, end))
            ours = run(torch_mod, sorter, keys, vals, begin, end)
            assert np.array_equal(ours.keys, theirs.keys) and np.array_equal(ours.keys, cases.reference(keys, None, begin, end)[0])
            assert vals is None or np.array_equal(ours.values, theirs.values)
            assert torch_mod.equal(ours.storage, theirs.storage)
        info = sorter.describe_range_sort_plan(n, False, begin, end)
        assert (info.name, info.launches, info.chunks) == ("one-workgroup", 1, 1)


@pytest.mark.parametrize("builder", cases.BUILDERS)
@pytest.mark.parametrize("n", cases.CROSS_PRODUCT_SIZES)
def test_every_builder_and_range(torch_mod, sorter, n, builder):
    torch = torch_mod
    for begin, end in cases.RANGES:
        keys, values = cases.case_inputs(builder, n, begin, end)
        if builder != "equal":
            check(torch, sorter, keys, values, begin, end)
            continue
        # an equal field: keys, values and every byte of the scratch arrays stay what they were
        info = sorter.describe_range_sort_plan(n, True, begin, end)
        for vals in (None, values):
            got = run(torch, sorter, keys, vals, begin, end)
            assert np.array_equal(got.keys, keys) and (vals is None or np.array_equal(got.values, vals))
            scratch = got.storage[scratch_from(info.chunks):got.required]
            assert scratch.numel() > 4 * n and bool((scratch == POISON_BYTE).all()), (begin, end)
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("begin,end", cases.RANGES)
def test_a_last_chunk_of_whole_tiles_and_pads(torch_mod, sorter, begin, end):
    keys, values = cases.case_inputs("uniform", 16385 + 255, begin, end)
    check(torch_mod, sorter, keys, values, begin, end)


@pytest.mark.parametrize("begin,end", cases.LARGE_RANGES)
@pytest.mark.parametrize("which", LARGE)
def test_sizes_around_the_chunk_and_tile_edges(torch_mod, sorter, cus, which, begin, end):
    """cus * 8192 -+ 1, cus * 16384 and + 1 (the first chunks of two tiles), 2 * cus * 16384 + 257 (three tiles per chunk)"""
    n = cases.large_sizes(cus)[which]
    info = sorter.describe_range_sort_plan(n, False, begin, end)
    assert info.name == "chunked" and info.chunks == min(cus, n // 8192) and info.keysPerChunk == cases.chunk_keys(n, cus)
    assert -(-info.keysPerChunk // cases.TILE) == (1, 1, 1, 2, 3)[which]
    for builder in cases.LARGE_BUILDERS:
        keys, values = cases.case_inputs(builder, n, begin, end)
        # (the largest size: one mode per builder, for the time the references take)
        modes = (False, True) if which < 4 else ((False,) if builder == "uniform" else (True,))
        check(torch_mod, sorter, keys, values, begin, end, modes=modes)
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("begin,end", [(5, 14), (1, 32)])
@pytest.mark.parametrize("large", [False, True], ids=["16385", "two-tile-chunks"])
def test_ballot_ranking(torch_mod, ballot_sorter, cus, large, begin, end):
    n = cus * 16384 + 1 if large else 16385
    for builder in ("uniform", "few"):
        keys, values = cases.case_inputs(builder, n, begin, end)
        check(torch_mod, ballot_sorter, keys, values, begin, end)


@pytest.mark.parametrize("name", cases.INDIRECT_COUNTS)
def test_indirect_counts(torch_mod, sorter, cus, name):
    """the count is read on the device and clamped to the bound; elements from it on keep their sentinel values; the count
    word is only read -- in a buffer of its own, and behind the keys in theirs"""
    bound = cases.indirect_bound(cus)
    count = cases.indirect_count(name, bound)
    n = min(count, bound)
    for (begin, end), modes, behind in (((4, 28), (True,), None), ((5, 14), (False,), 4)):
        keys, values = cases.case_inputs("uniform", bound + 8, begin, end)
        keys[n:] = np.arange(len(keys) - n, dtype=np.uint32)          # sentinels that would come first if they were sorted along
        values[n:] = np.uint32(0x70000000) + np.arange(len(values) - n, dtype=np.uint32)
        check(torch_mod, sorter, keys, values, begin, end, count=count, indirect=True, bound=bound, modes=modes,
              count_behind_keys=behind)
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("n", [16385 + 255, 65539])
@pytest.mark.parametrize("lead", [0, 1, 2, 3], ids=["0mod16", "4mod16", "8mod16", "12mod16"])
def test_arrays_at_every_four_byte_alignment(torch_mod, sorter, n, lead):
    """keys and values 0, 4, 8 and 12 bytes past a 16-byte boundary inside a larger allocation, sentinel bands on both sides"""
    for begin, end in [(5, 14), (4, 28)]:
        keys, values = cases.case_inputs("uniform", n, begin, end)
        band = np.full(64, GUARD, np.uint32)
        k, v = np.concatenate([keys, band]), np.concatenate([values, band])
        want = cases.reference(k, v, begin, end, n)
        check(torch_mod, sorter, k, v, begin, end, want=want, count=n, lead=lead)
        check(torch_mod, sorter, k, v, begin, end, want=want, count=n, lead=lead, indirect=True, bound=n)


@pytest.mark.parametrize("n", [65539, 1048583])
def test_full_range_is_the_whole_key_sort(torch_mod, sorter, n):
    """(0, 32): the result, the storage and the verdict of vrdxCmdSort[KeyValue]"""
    stream = torch_mod.cuda.current_stream().cuda_stream
    keys, values = cases.case_inputs("uniform", n, 0, 32)
    for vals in (None, values):
        whole = guarded_call(torch_mod, sorter, keys, vals)
        got = run(torch_mod, sorter, keys, vals, 0, 32)
        assert np.array_equal(got.keys, whole.keys) and np.array_equal(got.keys, np.sort(keys))
        assert vals is None or np.array_equal(got.values, whole.values)
        assert (sorter.read_plan_verdict(stream, got.storage.data_ptr(), 0) == sorter.read_plan_verdict(stream, whole.storage.data_ptr(), 0))
        info = sorter.describe_range_sort_plan(n, vals is not None, 0, 32)
        assert info.name == "whole-key" and info.launches == sorter.describe_plan(n, vals is not None).launches


@pytest.mark.parametrize("n", [4097, 65539])
@pytest.mark.parametrize("indirect", [False, True], ids=["direct", "indirect"])
def test_empty_range_touches_nothing(torch_mod, sorter, n, indirect):
    keys, values = cases.case_inputs("uniform", n, 3, 12)
    for vals in (None, values):
        got = run(torch_mod, sorter, keys, vals, *cases.EMPTY_RANGE, indirect=indirect, keep_before=True)
        assert np.array_equal(got.keys, keys) and (vals is None or np.array_equal(got.values, vals))
        assert torch_mod.equal(got.storage, got.before), "the empty range wrote to the storage"
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0
    assert sorter.describe_range_sort_plan(n, False, *cases.EMPTY_RANGE).name == "none"


@pytest.mark.parametrize("begin,end", cases.INVALID_RANGES)
@pytest.mark.parametrize("n", [4097, 65539])
def test_invalid_ranges_are_refused_with_nothing_touched(torch_mod, sorter, n, begin, end):
    import vulkan_radix_sort_amd as vrdx
    stream = torch_mod.cuda.current_stream().cuda_stream
    keys, values = cases.case_inputs("uniform", n, 3, 12)
    sorter.read_sorter_status(stream)   # (clears the word)
    for vals in (None, values):
        for indirect in (False, True):
            pool = vrdx.QueryPool(15)
            got = run(torch_mod, sorter, keys, vals, begin, end, indirect=indirect, pool=pool, expect_refused=True)
            assert np.array_equal(got.keys, keys) and (vals is None or np.array_equal(got.values, vals))
            ts = pool.results_ns()   # all 15 slots readable
            assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:]))
            pool.destroy()
    assert sorter.read_sorter_status(stream) == 0
    assert sorter.describe_range_sort_plan(n, False, begin, end).name == "none"


@pytest.mark.parametrize("n", [16385, 65539])
def test_timestamps_of_all_15_slots_are_monotone(torch_mod, sorter, n):
    import vulkan_radix_sort_amd as vrdx
    for begin, end in cases.RANGES + [cases.EMPTY_RANGE]:
        keys, values = cases.case_inputs("uniform", n, begin, end)
        for vals in (None, values):
            pool = vrdx.QueryPool(15)
            run(torch_mod, sorter, keys, vals, begin, end, pool=pool)
            ts = pool.results_ns()
            assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:])), (begin, end, ts)
            assert (ts[14] - ts[0] > 0) == (begin < end), (begin, end, ts)
            digits = cases.digits_of(begin, end)
            if begin < end:   # the slots behind the last scatter and in front of the copy back coincide
                assert len(set(ts[4 + 3 * (digits - 1):14])) == 1, (begin, end, ts)
            pool.destroy()


def test_verdict_on_storage_an_msd_sort_used(torch_mod, sorter):
    """the chunked form leaves VERDICT_NONE and status 0 where an MSD sort left its verdict; a whole-key sort behind it reports
    its own verdict again"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    n = 8_400_000
    rng = np.random.default_rng(8400)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    assert sorter.describe_plan(n, False).name == "msd"
    storage = torch.full((sorter.storage_requirements(n).size,), 0xA5, dtype=torch.uint8, device="cuda")
    dk = to_device(torch, keys)
    sorter.cmd_sort(stream, n, dk.data_ptr(), 0, storage.data_ptr(), 0)
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_MSD_RUNS
    range_keys = cases.case_inputs("uniform", 65539, 5, 14)[0]
    dr = to_device(torch, range_keys)
    sorter.cmd_range_sort(stream, len(range_keys), dr.data_ptr(), 0, 5, 14, storage.data_ptr(), 0)
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_NONE
    assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    assert np.array_equal(to_host(dr), cases.reference(range_keys, None, 5, 14)[0])
    dk.copy_(to_device(torch, keys))
    sorter.cmd_sort(stream, n, dk.data_ptr(), 0, storage.data_ptr(), 0)
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_MSD_RUNS
    assert np.array_equal(to_host(dk), np.sort(keys))


@pytest.mark.parametrize("large", [False, True], ids=["65539", "two-tile-chunks"])
def test_captured_graph_replays_on_other_data_and_counts(torch_mod, sorter, cus, large):
    """one capture of the indirect call replayed on four counts and fresh data, one capture of the direct call on other data"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    n = cus * 16384 + 1 if large else 65539
    begin, end = 4, 28
    replays = {True: (("uniform", n - 7), ("few", 1), ("const-mid", n), ("const-low", 16385)),
               False: (("const-mid", n), ("uniform", n))}
    for indirect in (True, False):
        key_value = indirect   # (the indirect call with values, the direct call keys-only)
        dk = torch.zeros(n, dtype=torch.int32, device="cuda")
        dv = torch.zeros(n, dtype=torch.int32, device="cuda") if key_value else None
        dcount = torch.full((1,), n, dtype=torch.int32, device="cuda") if indirect else None
        req = sorter.key_value_storage_requirements(n) if key_value else sorter.storage_requirements(n)
        storage = torch.empty(req.size, dtype=torch.uint8, device="cuda")
        vrdx.sort_range(sorter, dk, begin, end, values=dv, count=dcount, storage=storage)  # one eager call first
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            vrdx.sort_range(sorter, dk, begin, end, values=dv, count=dcount, storage=storage)
        for builder, count in replays[indirect]:
            keys, values = cases.case_inputs(builder, n, begin, end)
            keys = keys[::-1].copy()   # (not the arrays of the other tests)
            dk.copy_(torch.from_numpy(keys.view(np.int32)))
            if key_value:
                dv.copy_(torch.from_numpy(values.view(np.int32)))
            if indirect:
                dcount.fill_(count)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want_keys, want_values = cases.reference(keys, values, begin, end, count if indirect else n)
            assert np.array_equal(to_host(dk), want_keys), (builder, indirect)
            assert not key_value or np.array_equal(to_host(dv), want_values), (builder, indirect)
            assert not indirect or int(dcount.item()) == count
            assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
        assert sorter.read_sorter_status(stream) == 0


def test_describe_range_sort_plan(sorter, cus):
    for n in [16385, 65539] + cases.large_sizes(cus):
        for begin, end in cases.RANGES:
            for key_value in (False, True):
                info = sorter.describe_range_sort_plan(n, key_value, begin, end)
                digits = cases.digits_of(begin, end)
                assert (info.name, info.digits, info.launches) == ("chunked", digits, 3 * digits + 1), (n, begin, end)
                assert info.chunks == min(cus, n // 8192) and info.keysPerChunk == cases.chunk_keys(n, cus)
                assert (info.bytesPerElementPerPass, info.bytesPerElementCopyBack) == ((20, 16) if key_value else (12, 8))
                assert sorter.describe_sort_bits_plan(n, key_value, begin, end).plan == 0   # (that call still refuses)
    assert sorter.describe_range_sort_plan(0, False, 3, 12).name == "none"


def test_sort_range_front_end_against_torch(torch_mod, sorter):
    """vulkan_radix_sort_amd.sort_range against torch.sort(stable=True) of the field plus gathers"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    n, (begin, end) = 300_001, (5, 21)
    keys, values = cases.case_inputs("few", n, begin, end)
    dk, dv = to_device(torch, keys), to_device(torch, values)
    f = (dk.to(torch.int64) & 0xFFFFFFFF) >> begin & ((1 << (end - begin)) - 1)
    order = torch.sort(f, stable=True).indices
    want_keys, want_values = dk[order].clone(), dv[order].clone()
    storage = vrdx.sort_range(sorter, dk, begin, end, values=dv)
    assert torch.equal(dk, want_keys) and torch.equal(dv, want_values)
    assert storage.numel() == sorter.key_value_storage_requirements(n).size
    dk = to_device(torch, keys)
    count = torch.tensor([70_000], dtype=torch.int32, device="cuda")
    assert vrdx.sort_range(sorter, dk, begin, end, count=count, storage=storage) is storage
    assert np.array_equal(to_host(dk), cases.reference(keys, None, begin, end, 70_000)[0])
    assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0
    assert sort_bits_cases.REFUSED_SIZES[0] < n   # (sort_bits refuses this size)
