"""GPU tests of the sorts of 32-bit keys with 64-bit values (vrdxHipCmdWideValueSort[Indirect]): every form, bit for bit against
order = np.argsort(keys[:n], kind="stable"), keys[order] and values[order].  Values are never the index: random 64-bit words
whose halves differ, a few with a half of 0 or 0xFFFFFFFF, so that a dropped or swapped word shows."""
import numpy as np
import pytest

import vulkan_radix_sort_amd as vrdx
from wide_guarded_call import (ballot_sorter, expected, poisoned_storage, sorter, to_device, to_host, torch_mod,  # noqa: F401
                               wide_call)

pytestmark = pytest.mark.gpu


def _values(rng, n):
    v = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    v[(v >> np.uint64(32)) == (v & np.uint64(0xFFFFFFFF))] ^= np.uint64(1)   # the halves differ
    for at, word in zip(range(0, n, max(1, n // 7)), (0x00000000DEADBEEF, 0xFFFFFFFF12345678, 0x87654321FFFFFFFF, 0xCAFEF00D00000000)):
        v[at] = word
    return v


BUILDERS = {
    "uniform": lambda rng, n: rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32),
    "three": lambda rng, n: rng.choice(np.array([7, 0x80000001, 0xFFFFFFFE], np.uint32), size=n),
    "equal": lambda rng, n: np.full(n, 0x12345678, np.uint32),
    "all_ones": lambda rng, n: np.full(n, 0xFFFFFFFF, np.uint32),
    "descending": lambda rng, n: (np.uint32(0xFFFFFFF0) - np.arange(n, dtype=np.uint32) * np.uint32(3)),
    "byte2": lambda rng, n: (rng.integers(0, 256, size=n, dtype=np.uint64).astype(np.uint32) << np.uint32(16)) | np.uint32(0x5A00A55A),
}


def _check(got, keys, values, n, what):
    want_keys, want_values = expected(keys, values, n)
    assert np.array_equal(got.keys, want_keys), f"{what}: keys differ, first at {np.flatnonzero(got.keys != want_keys)[:4].tolist()}"
    assert np.array_equal(got.values, want_values), \
        f"{what}: values differ, first at {np.flatnonzero(got.values != want_values)[:4].tolist()}"


def _form(s, n):
    return s.describe_wide_value_sort_plan(n).name


@pytest.mark.parametrize("ranking", ["atomic", "ballot"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192])
def test_one_workgroup_form(torch_mod, sorter, ballot_sorter, n, ranking):
    s = sorter if ranking == "atomic" else ballot_sorter
    assert _form(s, n) == "one-workgroup"
    rng = np.random.default_rng(n)
    for name, build in BUILDERS.items():
        keys, values = build(rng, n), _values(rng, n)
        _check(wide_call(torch_mod, s, keys, values), keys, values, n, f"{name}, n = {n}")


@pytest.mark.parametrize("n", [8193, 8194, 8195, 8196, 9215, 9216, 9217, 16384, 16385, 65537])
def test_gather_form(torch_mod, sorter, n):
    assert _form(sorter, n) == "gather"
    rng = np.random.default_rng(n)
    for name, build in BUILDERS.items():
        keys, values = build(rng, n), _values(rng, n)
        _check(wide_call(torch_mod, sorter, keys, values), keys, values, n, f"{name}, n = {n}")


def test_gather_form_with_the_ballot_ranking(torch_mod, ballot_sorter):
    n = 9217
    rng = np.random.default_rng(5)
    keys, values = BUILDERS["three"](rng, n), _values(rng, n)
    _check(wide_call(torch_mod, ballot_sorter, keys, values), keys, values, n, "three")


@pytest.fixture(scope="module")
def two_sorts_from(sorter):
    info = sorter.describe_wide_value_sort_plan(1)
    assert info.oneWorkgroupMax == 8192
    return int(info.twoSortsFrom)


@pytest.mark.parametrize("delta,name", [(-1, "uniform"), (0, "three"), (0, "byte2"), (1, "uniform")])
def test_two_sorts_form_at_its_first_size(torch_mod, sorter, two_sorts_from, delta, name):
    """(one builder per case: at 2^24 elements the host's own stable argsort is what a case costs)"""
    n = two_sorts_from + delta
    assert _form(sorter, n) == ("gather" if delta < 0 else "two-sorts")
    rng = np.random.default_rng(77 + delta)
    keys, values = BUILDERS[name](rng, n), _values(rng, n)
    _check(wide_call(torch_mod, sorter, keys, values), keys, values, n, f"{name}, n = {n}")


def test_inner_msd_plan(torch_mod, sorter):
    """one direct sort at the first size at which the inner key+value sort records the MSD plan"""
    lo, hi = 1 << 20, 1 << 25
    assert sorter.describe_plan(lo, True).name != "msd" and sorter.describe_plan(hi, True).name == "msd"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if sorter.describe_plan(mid, True).name == "msd" else (mid, hi)
    n = hi
    info = sorter.describe_wide_value_sort_plan(n)
    inner = sorter.describe_plan(n, True)
    assert inner.name == "msd" and info.innerPlan == inner.plan and info.name in ("gather", "two-sorts")
    rng = np.random.default_rng(3)
    keys, values = BUILDERS["uniform"](rng, n), _values(rng, n)
    got = wide_call(torch_mod, sorter, keys, values)
    _check(got, keys, values, n, f"uniform, n = {n}")
    assert sorter.read_plan_verdict(torch_mod.cuda.current_stream().cuda_stream, got.storage.data_ptr(), 0) == vrdx.VERDICT_MSD_RUNS


def _bounds(two_sorts_from):
    return [8192, 20000, two_sorts_from]


@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("which", [0, 1, 2])
def test_indirect_bound_by_count(torch_mod, sorter, two_sorts_from, which, i):
    bound = _bounds(two_sorts_from)[which]
    assert _form(sorter, bound) == ("one-workgroup", "gather", "two-sorts")[which]
    count = (0, 1, 8193, bound - 1, bound, bound + 7)[i]
    rng = np.random.default_rng(bound + i)
    total = bound + 16
    n = min(count, bound)
    keys, values = BUILDERS["uniform" if i % 2 else "three"](rng, total), _values(rng, total)
    behind = (None, 4)[i % 2]   # the count word in a buffer of its own | behind the keys in theirs
    got = wide_call(torch_mod, sorter, keys, values, count=bound, device_count=count, count_behind_keys=behind)
    _check(got, keys, values, n, f"bound {bound}, count {count}")   # (elements from n on: as they were)


@pytest.mark.parametrize("n", [4097, 8195])
@pytest.mark.parametrize("keys_off", [4, 8, 12])
def test_alignment(torch_mod, sorter, n, keys_off):
    rng = np.random.default_rng(n + keys_off)
    keys, values = BUILDERS["uniform"](rng, n), _values(rng, n)
    got = wide_call(torch_mod, sorter, keys, values, keys_off=keys_off, values_off=8, storage_off=16 * keys_off)
    _check(got, keys, values, n, f"keys at {keys_off} mod 16, values at 8 mod 16")


def test_timestamps(torch_mod, sorter, two_sorts_from):
    for n, form in ((4096, "one-workgroup"), (20000, "gather"), (two_sorts_from, "two-sorts")):
        assert _form(sorter, n) == form
        rng = np.random.default_rng(n)
        keys, values = BUILDERS["uniform"](rng, n), _values(rng, n)
        pool = vrdx.QueryPool(15)
        _check(wide_call(torch_mod, sorter, keys, values, pool=pool), keys, values, n, form)
        ns = pool.results_ns()
        pool.destroy()
        assert len(ns) == 15 and ns[0] == 0 and all(a <= b for a, b in zip(ns, ns[1:])), (form, ns)
        assert ns[14] > 0
        if form != "one-workgroup":
            assert ns[4] == ns[14], (form, ns)   # the last step ends slot 4


def test_graph_replay(torch_mod, sorter):
    torch = torch_mod
    bound = 20000
    rng = np.random.default_rng(11)
    dk = torch.zeros(bound, dtype=torch.int32, device="cuda")
    dv = torch.zeros(bound, dtype=torch.int64, device="cuda")
    dc = torch.zeros(1, dtype=torch.int32, device="cuda")
    storage = torch.empty(sorter.wide_value_storage_requirements(bound).size, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        sorter.cmd_wide_value_sort_indirect(torch.cuda.current_stream().cuda_stream, bound, dc.data_ptr(), 0, dk.data_ptr(), 0,
                                            dv.data_ptr(), 0, storage.data_ptr(), 0, None, 0)
    for count in (0, 1, 8193, 20000):
        keys, values = BUILDERS["uniform"](rng, bound), _values(rng, bound)
        dk.copy_(torch.from_numpy(keys.view(np.int32)))
        dv.copy_(torch.from_numpy(values.view(np.int64)))
        dc.fill_(count)
        graph.replay()
        torch.cuda.synchronize()
        want_keys, want_values = expected(keys, values, count)
        assert np.array_equal(dk.cpu().numpy().view(np.uint32), want_keys), count
        assert np.array_equal(dv.cpu().numpy().view(np.uint64), want_values), count
        assert int(dc.item()) == count
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0


def test_storage_reuse(torch_mod, sorter):
    """a wide-value call on storage left by vrdxCmdSortKeyValue and by vrdxHipCmdSort64KeyValue, and the reverse"""
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(19)
    for n in (3000, 70001):
        size = max(sorter.wide_value_storage_requirements(n).size, sorter.storage_requirements64(n, True).size)
        storage = poisoned_storage(torch, size)
        keys32 = BUILDERS["uniform"](rng, n)
        values32 = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        keys64 = _values(rng, n)
        order32, order64 = np.argsort(keys32, kind="stable"), np.argsort(keys64, kind="stable")

        def sort32():
            dk, dv = to_device(torch, keys32), to_device(torch, values32)
            sorter.cmd_sort_key_value(stream, n, dk.data_ptr(), 0, dv.data_ptr(), 0, storage.data_ptr(), 0)
            torch.cuda.synchronize()
            assert np.array_equal(to_host(dk), keys32[order32]) and np.array_equal(to_host(dv), values32[order32])

        def sort64():
            dk, dv = to_device(torch, keys64), to_device(torch, values32)
            sorter.cmd_sort64_key_value(stream, n, dk.data_ptr(), 0, dv.data_ptr(), 0, storage.data_ptr(), 0)
            torch.cuda.synchronize()
            assert np.array_equal(to_host(dk), keys64[order64]) and np.array_equal(to_host(dv), values32[order64])

        def wide():
            values = _values(rng, n)
            _check(wide_call(torch, sorter, keys32, values, storage=storage), keys32, values, n, f"reused storage, n = {n}")

        for step in (sort32, wide, sort64, wide, sort32, wide, sort64):
            step()
            assert sorter.read_status(stream, storage.data_ptr(), 0) == 0


def test_front_end_against_torch(torch_mod, sorter):
    torch = torch_mod
    gen = torch.Generator(device="cuda").manual_seed(5)
    for n, dtype in ((1, torch.int64), (5000, torch.float64), (8192, torch.int64), (30001, torch.int64), (30001, torch.float64)):
        keys = torch.randint(-2**31, 2**31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32)
        keys[::3] = -12345   # ties
        bits = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device="cuda", generator=gen)
        values = bits if dtype is torch.int64 else bits.to(torch.float64)
        as_unsigned = keys.to(torch.int64) & 0xFFFFFFFF
        want_keys, index = torch.sort(as_unsigned, stable=True)
        want_values = values[index]
        k, v = keys.clone(), values.clone()
        vrdx.sort_key_value64(sorter, k, v)
        assert torch.equal(k.to(torch.int64) & 0xFFFFFFFF, want_keys) and torch.equal(v.view(torch.int64), want_values.view(torch.int64))
        # by a device-side count
        count = torch.tensor([n // 2], dtype=torch.int32, device="cuda")
        k, v = keys.clone(), values.clone()
        vrdx.sort_key_value64(sorter, k, v, count=count)
        half = n // 2
        hk, hi = torch.sort(as_unsigned[:half], stable=True)
        assert torch.equal(k[:half].to(torch.int64) & 0xFFFFFFFF, hk) and torch.equal(v[:half].view(torch.int64), values[:half][hi].view(torch.int64))
        assert torch.equal(k[half:], keys[half:]) and torch.equal(v[half:].view(torch.int64), values[half:].view(torch.int64))
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0
