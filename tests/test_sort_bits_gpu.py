"""GPU tests of the bit-range sorts (vrdxHipCmdSortBits[KeyValue][Indirect]): every result bit for bit against
sort_bits_cases.reference -- np.argsort(f(keys), kind="stable") applied to keys and values -- on keys whose bits outside the
range are random, so that a whole-key sort, a sort of masked keys and an unstable sort all show.  Every call runs on poisoned
storage with a guard band behind the requirement, and vrdxHipReadStatus is 0 after it.  Range sorts run in one workgroup, up to
16384 elements; the sizes are those of sort_bits_cases.py, which tests/test_sort_bits_plan.py holds to the planner, and a
range sort of more elements must be refused and touch nothing."""
import numpy as np
import pytest

import sort_bits_cases as cases
from guarded_call import ballot_sorter, guarded_call, sorter, to_device, to_host, torch_mod  # noqa: F401
from segmented_cases import GUARD

pytestmark = pytest.mark.gpu

ALL_RANGES = cases.RANGES
FEW_RANGES = [(3, 12), (7, 24)]


def run(torch, sorter, keys, values, begin, end, count=None, indirect=False, bound=None, query_pool=None, storage_out=None,
        lead=0):
    """One vrdxHipCmdSortBits* call on torch's current stream (guarded_call).  keys / values: the FULL host buffers, of which
    the first `count` (default: all) are sorted; indirect: the count travels in a device word and `bound` (default: the
    buffer's length) is maxElementCount.  lead: the arrays start that many words past a 16-byte boundary (4-byte alignment
    cases).  storage_out: a list that receives the storage before and after the call.  Returns (keys, values) as the call left
    them."""
    n = len(keys) if count is None else count
    bound = (len(keys) if indirect else n) if bound is None else bound
    assert indirect or bound == n
    got = guarded_call(torch, sorter, keys, values, count=bound, device_count=n if indirect else None, bit_range=(begin, end),
                       keys_off=4 * lead, values_off=4 * lead, indirect_off=4, pool=query_pool, keep_before=storage_out is not None,
                       recorded=min(n, bound) > 0 and begin < end <= 32 and (bound <= 16384 or (begin, end) == cases.FULL_RANGE))
    if storage_out is not None:
        storage_out.extend([got.before, got.storage])
    return got.keys, got.values


def check(torch, sorter, keys, values, begin, end, want=None, **kw):
    """keys-only and key+value against the reference (computed once for both)"""
    count = kw.get("count")
    bound = kw.get("bound")
    n = len(keys) if count is None else count
    n = n if bound is None else min(n, bound)
    want_keys, want_values = want if want is not None else cases.reference(keys, values, begin, end, n)
    got_keys, _ = run(torch, sorter, keys, None, begin, end, **kw)
    assert np.array_equal(got_keys, want_keys), ("keys-only", len(keys), begin, end)
    got_keys, got_values = run(torch, sorter, keys, values, begin, end, **kw)
    assert np.array_equal(got_keys, want_keys), ("key+value keys", len(keys), begin, end)
    assert np.array_equal(got_values, want_values), ("key+value values", len(keys), begin, end)


@pytest.mark.parametrize("n", cases.ONE_WORKGROUP_SIZES)
def test_every_range(torch_mod, sorter, n):
    for begin, end in ALL_RANGES:
        keys, values = cases.case_inputs("uniform", n, begin, end)
        check(torch_mod, sorter, keys, values, begin, end)
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("n", cases.BUILDER_SIZES)
@pytest.mark.parametrize("builder", cases.BUILDERS)
def test_every_builder(torch_mod, sorter, builder, n):
    """many ties, a digit that is the same in every key, all fields equal, ties with the pads"""
    for begin, end in ALL_RANGES:
        keys, values = cases.case_inputs(builder, n, begin, end)
        check(torch_mod, sorter, keys, values, begin, end)


@pytest.mark.parametrize("begin,end", cases.BALLOT_RANGES)
@pytest.mark.parametrize("n", cases.BALLOT_SIZES)
def test_ballot_ranking(torch_mod, ballot_sorter, n, begin, end):
    keys, values = cases.case_inputs("uniform", n, begin, end)
    check(torch_mod, ballot_sorter, keys, values, begin, end)
    keys, values = cases.case_inputs("few", n, begin, end)
    check(torch_mod, ballot_sorter, keys, values, begin, end)


@pytest.mark.parametrize("n", [4097, 65539])   # (an empty range is no sort: legal at any size)
@pytest.mark.parametrize("indirect", [False, True], ids=["direct", "indirect"])
def test_empty_range_touches_nothing(torch_mod, sorter, n, indirect):
    begin, end = cases.EMPTY_RANGE
    keys, values = cases.case_inputs("uniform", n, 3, 12)
    for vals in (None, values):
        storages = []
        got_keys, got_values = run(torch_mod, sorter, keys, vals, begin, end, indirect=indirect, storage_out=storages)
        assert np.array_equal(got_keys, keys) and (vals is None or np.array_equal(got_values, vals))
        assert bool((storages[0] == storages[1]).all()), "the empty range wrote to the storage"
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("n", [4097, 65539, 1048583])   # (the full range is the whole-key sort: every size)
def test_full_range_is_the_whole_key_sort(torch_mod, sorter, n):
    """(0, 32): the result, the plan and the device's verdict of vrdxCmdSort[KeyValue]"""
    from test_sort_gpu import gpu_sort
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    keys, values = cases.case_inputs("uniform", n, 0, 32)
    for vals in (None, values):
        a, b = [], []
        whole_keys, whole_values = gpu_sort(torch, sorter, keys, vals, storage_out=a)
        got_keys, got_values = run(torch, sorter, keys, vals, 0, 32, storage_out=b)
        assert np.array_equal(got_keys, whole_keys) and (vals is None or np.array_equal(got_values, whole_values))
        assert np.array_equal(got_keys, np.sort(keys))
        assert (sorter.read_plan_verdict(stream, b[1].data_ptr(), 0) == sorter.read_plan_verdict(stream, a[0].data_ptr(), 0))
        want, got = sorter.describe_plan(n, vals is not None), sorter.describe_sort_bits_plan(n, vals is not None, 0, 32)
        assert bytes(want) == bytes(got)


@pytest.mark.parametrize("bound", cases.INDIRECT_BOUNDS)
def test_indirect_counts(torch_mod, sorter, bound):
    """the count is read on the device and clamped to the bound; elements from it on keep their sentinel values; the count
    word is only read"""
    for begin, end in FEW_RANGES:
        keys, values = cases.case_inputs("uniform", bound + 8, begin, end)
        for count in (0, 1, bound - 1, bound, bound + 5):
            n = min(count, bound)
            k, v = keys.copy(), values.copy()
            k[n:] = np.arange(len(k) - n, dtype=np.uint32)          # sentinels that would come first if they were sorted along
            v[n:] = np.uint32(0x70000000) + np.arange(len(v) - n, dtype=np.uint32)
            check(torch_mod, sorter, k, v, begin, end, count=count, indirect=True, bound=bound)
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("n", [4095, 4097, 16384])
@pytest.mark.parametrize("lead", [1, 2, 3], ids=["4mod16", "8mod16", "12mod16"])
def test_arrays_at_every_four_byte_alignment(torch_mod, sorter, n, lead):
    """keys and values 4, 8 and 12 bytes past a 16-byte boundary inside a larger allocation, sentinel bands on both sides"""
    for begin, end in FEW_RANGES:
        keys, values = cases.case_inputs("uniform", n, begin, end)
        band = np.full(64, GUARD, np.uint32)
        k, v = np.concatenate([keys, band]), np.concatenate([values, band])
        want = cases.reference(k, v, begin, end, n)
        check(torch_mod, sorter, k, v, begin, end, want=want, count=n, lead=lead)
        check(torch_mod, sorter, k, v, begin, end, want=want, count=n, lead=lead, indirect=True, bound=n)


@pytest.mark.parametrize("begin,end,n", [(9, 8, 4097), (0, 33, 4097), (9, 8, 65539), (0, 33, 65539)]
                         + [(begin, end, n) for n in cases.REFUSED_SIZES for begin, end in FEW_RANGES + [(0, 1), (1, 32)]])
def test_invalid_ranges_and_sizes_beyond_one_workgroup_are_refused(torch_mod, sorter, n, begin, end):
    """beginBit > endBit, endBit > 32, and a valid range over more than 16384 elements: arrays and storage untouched,
    VRDX_HIP_STATUS_ENQUEUE_REFUSED in the sorter's word, all 15 slots readable"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    keys, values = cases.case_inputs("uniform", n, 3, 12)
    sorter.read_sorter_status(stream)   # (clears the word)
    for vals in (None, values):
        for indirect in (False, True):
            pool = vrdx.QueryPool(15)
            storages = []
            got_keys, got_values = run(torch, sorter, keys, vals, begin, end, indirect=indirect, query_pool=pool, storage_out=storages)
            assert np.array_equal(got_keys, keys) and (vals is None or np.array_equal(got_values, vals))
            assert bool((storages[0] == storages[1]).all()), "a refused range wrote to the storage"
            assert sorter.read_sorter_status(stream) == vrdx.STATUS_ENQUEUE_REFUSED
            ts = pool.results_ns()   # all 15 slots readable
            assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:]))
            pool.destroy()
    assert sorter.read_sorter_status(stream) == 0
    assert sorter.describe_sort_bits_plan(n, False, begin, end).plan == 0


@pytest.mark.parametrize("n", [4096, 16384])
def test_timestamps(torch_mod, sorter, n):
    import vulkan_radix_sort_amd as vrdx
    for begin, end in ALL_RANGES + [cases.EMPTY_RANGE]:
        keys, values = cases.case_inputs("uniform", n, begin, end)
        for vals in (None, values):
            pool = vrdx.QueryPool(15)
            run(torch_mod, sorter, keys, vals, begin, end, query_pool=pool)
            ts = pool.results_ns()
            assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:])), (begin, end, ts)
            assert (ts[14] - ts[0] > 0) == (begin < end), (begin, end, ts)
            pool.destroy()


def test_verdict_on_storage_an_msd_sort_used(torch_mod, sorter):
    """a range sort leaves VERDICT_NONE where an MSD sort left its verdict (both one-workgroup kernels); a whole-key sort
    behind it reports its own verdict again"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    n = 8_400_000
    rng = np.random.default_rng(8400)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    assert sorter.describe_plan(n, False).name == "msd"
    storage = torch.full((sorter.storage_requirements(n).size,), 0xA5, dtype=torch.uint8, device="cuda")
    dk = to_device(torch, keys)
    small, mid = cases.case_inputs("uniform", 4096, 3, 12)[0], cases.case_inputs("uniform", 16384, 7, 24)[0]
    for range_keys, (begin, end) in ((small, (3, 12)), (mid, (7, 24))):
        dk.copy_(to_device(torch, keys))
        sorter.cmd_sort(stream, n, dk.data_ptr(), 0, storage.data_ptr(), 0)
        assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_MSD_RUNS
        dr = to_device(torch, range_keys)
        sorter.cmd_sort_bits(stream, len(range_keys), dr.data_ptr(), 0, begin, end, storage.data_ptr(), 0)
        assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_NONE
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
        assert np.array_equal(to_host(dr), cases.reference(range_keys, None, begin, end)[0])
    dk.copy_(to_device(torch, keys))
    sorter.cmd_sort(stream, n, dk.data_ptr(), 0, storage.data_ptr(), 0)
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_MSD_RUNS
    assert np.array_equal(to_host(dk), np.sort(keys))


@pytest.mark.parametrize("n", [4096, 16384])
@pytest.mark.parametrize("indirect", [False, True], ids=["direct", "indirect"])
def test_captured_graph_replays_on_other_data_and_counts(torch_mod, sorter, n, indirect):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    begin, end = 7, 24
    for key_value in (False, True):
        dk = torch.zeros(n, dtype=torch.int32, device="cuda")
        dv = torch.zeros(n, dtype=torch.int32, device="cuda") if key_value else None
        dcount = torch.full((1,), n, dtype=torch.int32, device="cuda") if indirect else None
        req = sorter.key_value_storage_requirements(n) if key_value else sorter.storage_requirements(n)
        storage = torch.empty(req.size, dtype=torch.uint8, device="cuda")
        vrdx.sort_bits(sorter, dk, begin, end, values=dv, count=dcount, storage=storage)  # one eager call first
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            vrdx.sort_bits(sorter, dk, begin, end, values=dv, count=dcount, storage=storage)
        for builder, count in (("uniform", n - 7), ("few", 1), ("const-byte", n)):
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
            assert np.array_equal(to_host(dk), want_keys), (builder, key_value)
            assert not key_value or np.array_equal(to_host(dv), want_values), (builder, key_value)
            assert not indirect or int(dcount.item()) == count
            assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
        assert sorter.read_sorter_status(stream) == 0


def test_describe_sort_bits_plan(sorter):
    for n in cases.ONE_WORKGROUP_SIZES + cases.REFUSED_SIZES:
        for begin, end in ALL_RANGES:
            for key_value in (False, True):
                info = sorter.describe_sort_bits_plan(n, key_value, begin, end)
                want = ("one-workgroup", 1, 16 if key_value else 8) if n <= 16384 else ("none", 0, 0)
                assert (info.name, info.launches, info.bytesPerElement) == want, (n, begin, end, key_value)
                assert info.fallbackBytesPerElement == info.bytesPerElement and info.bits == 0
    assert sorter.describe_sort_bits_plan(4097, False, *cases.EMPTY_RANGE).plan == 0
    assert sorter.describe_sort_bits_plan(0, False, 3, 12).plan == 0


def test_sort_bits_python_front_end(torch_mod, sorter):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    n = 12_345
    keys, values = cases.case_inputs("few", n, 5, 21)
    dk, dv = to_device(torch, keys), to_device(torch, values)
    storage = vrdx.sort_bits(sorter, dk, 5, 21, values=dv)
    want = cases.reference(keys, values, 5, 21)
    assert np.array_equal(to_host(dk), want[0]) and np.array_equal(to_host(dv), want[1])
    assert storage.numel() == sorter.key_value_storage_requirements(n).size
    dk = to_device(torch, keys)
    count = torch.tensor([1000], dtype=torch.int32, device="cuda")
    assert vrdx.sort_bits(sorter, dk, 5, 21, count=count, storage=storage) is storage
    assert np.array_equal(to_host(dk), cases.reference(keys, None, 5, 21, 1000)[0])
    assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0
