"""GPU tests of the 64-bit sorts by a device-side count (vrdxHipCmdSort64[KeyValue]Indirect, vulkan_radix_sort_amd.sort64
with `count`), through the C ABI and element for element against numpy.  With n = min(count, bound) the first n elements
must be what the direct form leaves for n -- np.sort of the keys, np.argsort(kind="stable") applied to keys and values --
and every element from n on, inside the bound or behind it, bit for bit what it was.  The guard scheme is guarded_call's
(tests/guarded_call.py): guard bytes around the caller's arrays and around the storage requirement OF THE BOUND, the
status words read after every call; the count word is checked to be what it was.  Values are payload64, nowhere their own
index."""
import functools
import os
import subprocess

import numpy as np
import pytest

from guarded_call import BAND_BYTE as STORAGE_GUARD
from guarded_call import guarded_call, sorter, torch_mod  # noqa: F401
from sort64_model import case_inputs, check64, with_tail

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYBRID_BOUND = (1 << 18) + 3   # the inner sorts record the hybrid plan
MSD_BOUND = 8_200_001          # ... the MSD plan; a small count under it leaves whole workgroups of every kernel past n
BOUNDS = [1, 1027, 16384, 16385, HYBRID_BOUND]  # the one-workgroup plan, its last size, the hybrid plan from its first
COUNTS = ["0", "1", "3", "half-odd", "M-1", "M", "M+7"]
EXTRA = 5                      # elements of the arrays behind the bound


def count_of(name, bound):
    return {"0": 0, "1": 1, "3": 3, "half-odd": (bound // 2) | 1, "M-1": bound - 1, "M": bound, "M+7": bound + 7}[name]


@functools.lru_cache(maxsize=None)
def _case(pattern, bound):
    """(keys, values, order) of bound + EXTRA elements, the last EXTRA of them with_tail's (keys that would come first if they
    were sorted along); order = np.argsort(kind="stable") of the first `bound` keys.  Computed once, written by nobody."""
    keys, values = with_tail(*case_inputs(pattern, bound), extra=EXTRA)
    order = np.argsort(keys[:bound], kind="stable").astype(np.uint32)
    for a in (keys, values, order):
        a.setflags(write=False)
    return keys, values, order


def _want(pattern, bound, n, key_value):
    """the sorted first n <= bound elements.  The stable order of a prefix is the stable order of the whole with the
    indices from n on struck out, so the big bound is sorted once for all its counts."""
    keys, values, order = _case(pattern, bound)
    if n > 4096:
        order = order[order < n]
    else:
        order = np.argsort(keys[:n], kind="stable")
    return keys[order], (values[order] if key_value else None)


def run64_indirect(torch, s, keys, values, bound, count, count_in_keys=False, **where):
    """One call with the count in a device word (guarded_call: keys_off, values_off, storage_off, indirect_off, pool), the
    storage sized for `bound`; count_in_keys: the word lies in the keys' buffer, 12 bytes behind the last key, at an address
    that is 4 mod 8.  The sorter's sticky word must be 0 afterwards.  Returns the whole arrays as the device left them."""
    got = guarded_call(torch, s, keys, values, count=bound, device_count=count, sticky=0,
                       count_behind_keys=12 if count_in_keys else None, **where)
    return got.keys, got.values


def _parity(torch, s, pattern, bound, count, key_value, **where):
    keys, values, _ = _case(pattern, bound)
    values = values if key_value else None
    n = min(count, bound)
    try:
        got_keys, got_values = run64_indirect(torch, s, keys, values, bound, count, **where)
        # (check64 also asserts that elements [n, len) of keys and values are the input's, bit for bit)
        check64(got_keys, got_values, keys, values, count=n, want=_want(pattern, bound, n, key_value))
    except AssertionError as e:
        raise AssertionError(f"{pattern} bound={bound} count={count} {'pairs' if key_value else 'keys'} {where}: {e}") from e


# ---- 1. parity, bound x count ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("pattern", ["uniform", "tile-depth"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("bound", BOUNDS)
def test_indirect_matches_numpy(torch_mod, sorter, bound, count, pattern, key_value):
    _parity(torch_mod, sorter, pattern, bound, count_of(count, bound), key_value)


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("count", [0, 1000, MSD_BOUND - 1, MSD_BOUND + 7])
def test_indirect_under_an_msd_bound(torch_mod, sorter, count, key_value):
    """Both inner sorts record the MSD plan for the bound.  Counts 0 and 1000 are also the tiny count under a large bound
    for the streaming kernels: all but the first of their 8008 workgroups lie past n."""
    assert sorter.describe_plan(MSD_BOUND, True).name == "msd"
    _parity(torch_mod, sorter, "tile-depth", MSD_BOUND, count, key_value)


# ---- 2. the scalar tail in the middle of the grid ------------------------------------------------------------------------------

TAIL_BOUND = 4103
TAIL_COUNTS = list(range(1020, 1030)) + list(range(4096, 4104))


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("count", TAIL_COUNTS)
def test_the_scalar_tail_in_the_middle_of_the_grid(torch_mod, sorter, count, key_value):
    """The grid covers the bound (five workgroups of 256 x 4 elements), the thread with the last n mod 4 elements is wherever
    the count puts it: the last thread of the first workgroup, the first of the second, the last one that has work at all.
    Every alignment of the caller's arrays that the 16-byte accesses have to take."""
    for keys_off in (0, 8):
        for values_off in ((0, 4, 8, 12) if key_value else (0,)):
            _parity(torch_mod, sorter, "dup-high", TAIL_BOUND, count, key_value, keys_off=keys_off, values_off=values_off)


# ---- 3. where the count lives ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("bound,count", [(1027, 0), (1027, 513), (1027, 1027), (70_002, 35_001), (70_002, 70_002),
                                         (HYBRID_BOUND, 99_999)])
def test_the_count_in_the_keys_buffer(torch_mod, sorter, bound, count, key_value):
    """The count word shares the keys' buffer, 12 bytes behind the last key at an address that is 4 mod 8 (indirectOffset is
    that byte offset, not 0); keys 8-byte and values 4-byte aligned only; a storage offset of 16 + 128 k."""
    _parity(torch_mod, sorter, "tile-depth", bound, count, key_value, keys_off=8, values_off=4, storage_off=16 + 128 * 3,
            count_in_keys=True)


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_the_count_at_an_offset_of_its_own_buffer(torch_mod, sorter, key_value):
    _parity(torch_mod, sorter, "uniform", 16385, 8191, key_value, indirect_off=20, storage_off=16 + 128)


# ---- 4. one capture, many counts -----------------------------------------------------------------------------------------------

def _capture(torch, s, bound, key_value):
    """(graph, keys, values, count, storage): one indirect call of each form captured on a side stream after an eager one"""
    dk = torch.zeros(bound + EXTRA, dtype=torch.int64, device="cuda")
    dv = torch.zeros(bound + EXTRA, dtype=torch.int32, device="cuda") if key_value else None
    dc = torch.zeros(1, dtype=torch.int32, device="cuda")
    storage = torch.empty(s.storage_requirements64(bound, key_value).size, dtype=torch.uint8, device="cuda")

    def record():
        stream = torch.cuda.current_stream().cuda_stream
        if key_value:
            s.cmd_sort64_key_value_indirect(stream, bound, dc.data_ptr(), 0, dk.data_ptr(), 0, dv.data_ptr(), 0,
                                            storage.data_ptr(), 0)
        else:
            s.cmd_sort64_indirect(stream, bound, dc.data_ptr(), 0, dk.data_ptr(), 0, storage.data_ptr(), 0)

    record()  # one eager call first, as the other capture tests do
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        record()
    return g, dk, dv, dc, storage


def _replay(torch, s, captured, keys, values, counts, want):
    """replays the captured call once per count, each time on a fresh copy of the inputs; the count gets there by a
    device-to-device copy"""
    g, dk, dv, dc, storage = captured
    stream = torch.cuda.current_stream().cuda_stream
    bound = len(keys) - EXTRA
    device_counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
    for i, count in enumerate(counts):
        dk.copy_(torch.from_numpy(keys.view(np.int64).copy()))
        if dv is not None:
            dv.copy_(torch.from_numpy(values.view(np.int32).copy()))
        dc.copy_(device_counts[i:i + 1])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        n = min(count, bound)
        try:
            check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if dv is not None else None, keys,
                    values if dv is not None else None, count=n, want=want(n))
        except AssertionError as e:
            raise AssertionError(f"replay {i} with count {count}: {e}") from e
        assert int(dc.item()) == count
        assert s.read_status(stream, storage.data_ptr(), 0) == 0
        assert s.read_sorter_status(stream) == 0


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_one_capture_replays_on_many_counts(torch_mod, sorter, key_value):
    bound = HYBRID_BOUND
    keys, values, _ = _case("uniform", bound)
    captured = _capture(torch_mod, sorter, bound, key_value)
    _replay(torch_mod, sorter, captured, keys, values, [bound, 0, 1, 70_001, bound - 1],
            lambda n: _want("uniform", bound, n, key_value))


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_one_capture_replays_under_an_msd_bound(torch_mod, sorter, key_value):
    bound = MSD_BOUND
    keys, values, _ = _case("tile-depth", bound)
    captured = _capture(torch_mod, sorter, bound, key_value)
    _replay(torch_mod, sorter, captured, keys, values, [bound, 12_345], lambda n: _want("tile-depth", bound, n, key_value))


# ---- 5. timestamps -------------------------------------------------------------------------------------------------------------

def _slots_coincide_as_documented(ts, key_value):
    assert len(ts) == 15 and ts[0] == 0
    assert all(b >= a for a, b in zip(ts, ts[1:])), ts
    assert all(t == ts[6] for t in ts[6:]), ts
    if not key_value:
        assert ts[3] == ts[2] and ts[6] == ts[5], ts


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("count", [1027, 0])
def test_timestamp_slots(torch_mod, sorter, count, key_value):
    """All 15 slots are recorded and non-decreasing whatever the count turns out to be (the host cannot know it), and they
    coincide where the direct form's do."""
    import vulkan_radix_sort_amd as vrdx
    bound = 1027
    keys, values, _ = _case("uniform", bound)
    pool = vrdx.QueryPool(15)
    got_keys, got_values = run64_indirect(torch_mod, sorter, keys, values if key_value else None, bound, count, pool=pool)
    check64(got_keys, got_values, keys, values if key_value else None, count=count,
            want=_want("uniform", bound, count, key_value))
    ts = pool.results_ns(0, 15)
    print("sort64 indirect %s bound=%d count=%d slots (ns): %s" % ("pairs" if key_value else "keys", bound, count, ts))
    _slots_coincide_as_documented(ts, key_value)
    pool.destroy()


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_an_empty_bound_records_the_slots_and_touches_nothing(torch_mod, sorter, key_value):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    keys = np.arange(100, 0, -1, dtype=np.uint64)
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    dv = torch.arange(100, dtype=torch.int32, device="cuda")
    dc = torch.tensor([100], dtype=torch.int32, device="cuda")
    storage = torch.full((sorter.storage_requirements64(100, True).size,), STORAGE_GUARD, dtype=torch.uint8, device="cuda")
    pool = vrdx.QueryPool(15)
    if key_value:
        sorter.cmd_sort64_key_value_indirect(stream, 0, dc.data_ptr(), 0, dk.data_ptr(), 0, dv.data_ptr(), 0,
                                             storage.data_ptr(), 0, pool, 0)
    else:
        sorter.cmd_sort64_indirect(stream, 0, dc.data_ptr(), 0, dk.data_ptr(), 0, storage.data_ptr(), 0, pool, 0)
    torch.cuda.synchronize()
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), keys)
    assert np.array_equal(dv.cpu().numpy(), np.arange(100, dtype=np.int32))
    assert int(dc.item()) == 100
    assert bool((storage == STORAGE_GUARD).all())
    _slots_coincide_as_documented(pool.results_ns(0, 15), key_value)
    assert sorter.read_sorter_status(stream) == 0
    pool.destroy()


# ---- 6. the Python front end ---------------------------------------------------------------------------------------------------

def _tensors(torch, keys, values):
    return (torch.from_numpy(keys.view(np.int64).copy()).cuda(),
            torch.from_numpy(values.view(np.int32).copy()).cuda() if values is not None else None)


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_sort64_with_a_count_tensor(torch_mod, sorter, key_value):
    """sort64(..., count=t): keys.numel() is the bound and sizes the storage, only the first t elements are sorted; an int32
    count and, where torch has the dtype, a uint32 one."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    bound = 70_002
    keys, values, _ = _case("tile-depth", bound)
    keys, values = keys[:bound], (values[:bound] if key_value else None)
    dtypes = [torch.int32] + ([torch.uint32] if hasattr(torch, "uint32") else [])
    for dtype, count in zip(dtypes, (50_001, 12_345)):
        dk, dv = _tensors(torch, keys, values)
        dc = torch.tensor([count], dtype=dtype, device="cuda")
        storage = vrdx.sort64(sorter, dk, dv, count=dc)
        torch.cuda.synchronize()
        assert storage.numel() == sorter.storage_requirements64(bound, key_value=key_value).size
        check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if key_value else None, keys, values,
                count=count, want=_want("tile-depth", bound, count, key_value))
        assert int(dc.cpu().item()) == count
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    assert sorter.read_sorter_status(stream) == 0


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_sort64_with_a_count_in_a_torch_graph(torch_mod, sorter, key_value):
    """captured in torch.cuda.graph, replayed once after the count has changed"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    bound = 70_002
    keys, values, _ = _case("tile-depth", bound)
    keys, values = keys[:bound], (values[:bound] if key_value else None)
    dk, dv = _tensors(torch, keys, values)
    dc = torch.tensor([bound], dtype=torch.int32, device="cuda")
    storage = torch.empty(sorter.storage_requirements64(bound, key_value).size, dtype=torch.uint8, device="cuda")
    vrdx.sort64(sorter, dk, dv, storage=storage, count=dc)  # one eager call first, as the other capture tests do
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vrdx.sort64(sorter, dk, dv, storage=storage, count=dc)
    dk.copy_(torch.from_numpy(keys.view(np.int64).copy()))
    if key_value:
        dv.copy_(torch.from_numpy(values.view(np.int32).copy()))
    dc.fill_(33_333)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if key_value else None, keys, values,
            count=33_333, want=_want("tile-depth", bound, 33_333, key_value))
    assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    assert sorter.read_sorter_status(stream) == 0


def test_sort64_without_a_count_is_the_direct_sort(torch_mod, sorter):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    bound = 70_002
    keys, values, _ = _case("tile-depth", bound)
    keys, values = keys[:bound], values[:bound]
    dk, dv = _tensors(torch, keys, values)
    vrdx.sort64(sorter, dk, dv, count=None)
    ek, ev = _tensors(torch, keys, values)
    stream = torch.cuda.current_stream().cuda_stream
    storage = torch.empty(sorter.storage_requirements64(bound, True).size, dtype=torch.uint8, device="cuda")
    sorter.cmd_sort64_key_value(stream, bound, ek.data_ptr(), 0, ev.data_ptr(), 0, storage.data_ptr(), 0)
    torch.cuda.synchronize()
    assert torch.equal(dk, ek) and torch.equal(dv, ev)
    check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32), keys, values,
            want=_want("tile-depth", bound, bound, True))
    assert sorter.read_sorter_status(stream) == 0


def test_sort64_refuses_a_bad_count(torch_mod, sorter):
    """before anything is recorded: the keys are as they were and the sorter has nothing to report"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    keys = np.arange(64, 0, -1, dtype=np.uint64)
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    with pytest.raises(TypeError):
        vrdx.sort64(sorter, dk, count=torch.tensor([64], dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        vrdx.sort64(sorter, dk, count=64)
    with pytest.raises(ValueError):
        vrdx.sort64(sorter, dk, count=torch.tensor([64, 64], dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        vrdx.sort64(sorter, dk, count=torch.tensor([64], dtype=torch.int32))
    torch.cuda.synchronize()
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), keys)
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0


def test_sort64_refuses_a_count_on_another_device(torch_mod, sorter):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    dk = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError):
        vrdx.sort64(sorter, dk, count=torch.tensor([64], dtype=torch.int32, device="cuda:1"))


# ---- 7. the single header ------------------------------------------------------------------------------------------------------

SINGLE_HEADER_CASE = r"""
#define VRDX_IMPLEMENTATION
#include "vk_radix_sort.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>

// bound + 3 elements in the arrays, the count word behind the values in their buffer
static size_t Run(VrdxSorter sorter, uint32_t bound, uint32_t count, bool keyValue) {
  const uint32_t len = bound + 3;
  std::vector<uint64_t> keys(len);
  std::vector<uint32_t> values(len + 1);
  uint64_t x = 88172645463325252ull + bound + count;
  for (uint32_t i = 0; i < len; ++i) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    keys[i] = (i % 3 == 0) ? (x & 0xFFFF0000000000FFull) : x;  // duplicates of both words
    values[i] = i * 2654435761u ^ 0x80000000u;  // not the index
  }
  values[len] = count;
  VrdxSorterStorageRequirements req;
  if (keyValue) vrdxHipGetSorter64KeyValueStorageRequirements(sorter, bound, &req);
  else vrdxHipGetSorter64StorageRequirements(sorter, bound, &req);
  uint64_t* dk; uint32_t* dv; uint8_t* st;
  if (hipMalloc(&dk, 8ull * len) != hipSuccess || hipMalloc(&dv, 4ull * (len + 1)) != hipSuccess ||
      hipMalloc(&st, req.size) != hipSuccess)
    return ~(size_t)0;
  (void)hipMemcpy(dk, keys.data(), 8ull * len, hipMemcpyHostToDevice);
  (void)hipMemcpy(dv, values.data(), 4ull * (len + 1), hipMemcpyHostToDevice);
  if (keyValue)
    vrdxHipCmdSort64KeyValueIndirect(nullptr, sorter, bound, (VkBuffer)dv, 4ull * len, (VkBuffer)dk, 0, (VkBuffer)dv, 0,
                                     (VkBuffer)st, 0, nullptr, 0);
  else
    vrdxHipCmdSort64Indirect(nullptr, sorter, bound, (VkBuffer)dv, 4ull * len, (VkBuffer)dk, 0, (VkBuffer)st, 0, nullptr, 0);
  std::vector<uint64_t> gk(len);
  std::vector<uint32_t> gv(len + 1);
  (void)hipMemcpy(gk.data(), dk, 8ull * len, hipMemcpyDeviceToHost);
  (void)hipMemcpy(gv.data(), dv, 4ull * (len + 1), hipMemcpyDeviceToHost);
  const uint32_t n = std::min(count, bound);
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  size_t bad = 0;
  for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[idx[i]] || gv[i] != (keyValue ? values[idx[i]] : values[i]);
  for (uint32_t i = n; i < len; ++i) bad += gk[i] != keys[i] || gv[i] != values[i];  // from n on: as they were
  bad += gv[len] != count;
  (void)hipFree(dk); (void)hipFree(dv); (void)hipFree(st);
  return bad;
}

int main() {
  VrdxSorterCreateInfo info = {};
  VrdxSorter sorter = nullptr;
  if (vrdxCreateSorter(&info, &sorter) != VK_SUCCESS) { std::printf("no sorter\n"); return 2; }
  size_t bad = 0;
  for (uint32_t count : {50001u, 0u})
    for (bool keyValue : {false, true}) bad += Run(sorter, 70002u, count, keyValue);
  const uint32_t status = vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("status %u, %zu mismatches\n", status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
"""


def test_single_header_indirect_parity(tmp_path):
    """Both indirect entry points through the single header's own launcher (the kernels resolved by their mangled names,
    which carry the new parameter), compiled with plain g++: bound 70 002 with counts 50 001 and 0, against
    std::stable_sort, the elements from the count on and the count word as they were."""
    header = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
    if not os.path.exists(header):
        subprocess.run(["python3", os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", header], check=True)
    src = tmp_path / "sort64_indirect_single_header.cc"
    src.write_text(SINGLE_HEADER_CASE)
    exe = tmp_path / "sort64_indirect_single_header"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.dirname(header), str(src), "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "status 0, 0 mismatches" in r.stdout, r.stdout + r.stderr
