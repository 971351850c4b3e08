"""GPU tests of the key orders of the 64-bit sorts (vrdxHipCmdSort64Ordered[KeyValue][Indirect], vulkan_radix_sort_amd.sort64
with `order` / `descending`), through the C ABI and bit for bit against the reference of tests/key_order_cases.py:
np.argsort(T(keys), kind="stable") applied to keys and values.  Elements from the count on, guard bytes around the arrays
and around the storage requirement, and the status words are checked after every call (tests/guarded_call.py).  Sizes: the
scalar tail, the edge of a 256 x 4 workgroup, where the inner sorts leave the one-workgroup plan, and the hybrid plan --
nothing larger, because the inner sorts are the calls the unordered sorts make."""
import functools
import os
import subprocess

import numpy as np
import pytest

from guarded_call import guarded_call, sorter, torch_mod  # noqa: F401
from key_order_cases import BUILDERS, DIRECTIONS, ORDERS, assert_same, case_keys, expected, order_word
from test_sort64_gpu import run64

pytestmark = pytest.mark.gpu


def run64_ordered(torch, s, keys, values, word, *, storage_out=None, **kw):
    """One call with the order word `word` (guarded_call: count -- the elementCount, or with device_count the bound --
    keys_off, values_off, storage_off, pool, expect_refused), the count word at 4 mod 16.  Unless the call is refused the
    sorter's sticky word must be 0 afterwards.  Returns the whole arrays as the device left them."""
    got = guarded_call(torch, s, keys, values, order=word, indirect_off=4, sticky=0, **kw)
    if storage_out is not None:
        storage_out.append(got.storage)
    return got.keys, got.values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 16384, 16385, 300001]
EXTRA = 5   # elements of the arrays behind the count


@functools.lru_cache(maxsize=None)
def _case(builder, n, order, descending):
    """(keys, values) of n + EXTRA elements and the expected arrays, computed once and written by nobody"""
    keys, values = case_keys(builder, n + EXTRA, order, descending)
    want = expected(keys, values, order, descending, count=n)
    for a in (keys, values) + want:
        a.setflags(write=False)
    return keys, values, want


def _check(torch, s, builder, n, order, descending, key_value, **where):
    keys, values, want = _case(builder, n, order, descending)
    got = run64_ordered(torch, s, keys, values if key_value else None, order_word(order, descending), count=n, **where)
    assert_same(*got, want, f"{builder} n={n} {order} descending={descending} {'pairs' if key_value else 'keys'} {where}")


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", SIZES)
def test_every_order_direction_and_form(torch_mod, sorter, n, order, descending, key_value):
    builders = BUILDERS if n <= 16385 else ("float-specials", "duplicates", "mixed-int")
    for builder in builders:
        _check(torch_mod, sorter, builder, n, order, descending, key_value)


# ---- the device-side count ---------------------------------------------------------------------------------------------------

BOUND = 4103   # five workgroups of the streaming kernels


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
@pytest.mark.parametrize("order", ORDERS)
def test_the_indirect_forms(torch_mod, sorter, order, descending, key_value):
    """counts 0 and 1, counts that put the thread with the scalar tail in the middle of the grid (the last thread of the
    first workgroup, the first of the second), the bound and a count beyond it; elements from the count on lie between the
    sorted ones and the guard bytes and must stay as they were"""
    keys, values = case_keys("float-specials", BOUND + EXTRA, order, descending, tag="indirect")
    for count in (0, 1, 1022, 1027, 2049, BOUND, BOUND + 7):
        n = min(count, BOUND)
        got = run64_ordered(torch_mod, sorter, keys, values if key_value else None, order_word(order, descending), count=BOUND,
                            device_count=count)
        assert_same(*got, expected(keys, values, order, descending, count=n), f"count {count}")


# ---- alignment -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
@pytest.mark.parametrize("order", ORDERS)
def test_keys_at_8_mod_16_and_values_at_every_4_byte_alignment(torch_mod, sorter, order, descending):
    _check(torch_mod, sorter, "float-specials", 1025, order, descending, False, keys_off=8, storage_off=16 + 128)
    for values_off in (4, 8, 12):
        _check(torch_mod, sorter, "float-specials", 1025, order, descending, True, keys_off=8, values_off=values_off)
        _check(torch_mod, sorter, "duplicates", 16385, order, descending, True, keys_off=8, values_off=values_off,
               storage_off=16 + 128 * 3)


# ---- order == 0, and words that are no order -------------------------------------------------------------------------------------

@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("n", [1025, 300001])
def test_the_unsigned_order_is_the_twin(torch_mod, sorter, n, key_value):
    """VRDX_HIP_KEY_UINT64 records what vrdxHipCmdSort64[KeyValue] records: the same arrays and the same header words"""
    keys, values, _ = _case("uniform", n, "uint64", False)
    values = values if key_value else None
    twin, ordered = [], []
    want = run64(torch_mod, sorter, keys, values, count=n, storage_out=twin)
    got = run64_ordered(torch_mod, sorter, keys, values, 0, count=n, storage_out=ordered)
    assert_same(*got, want)
    assert_same(*got, expected(keys, values, "uint64", False, count=n))
    assert torch_mod.equal(twin[0][:16], ordered[0][:16]), "header words 0-3"
    stream = torch_mod.cuda.current_stream().cuda_stream
    assert (sorter.read_plan_verdict(stream, twin[0].data_ptr(), 0) == sorter.read_plan_verdict(stream, ordered[0].data_ptr(), 0))


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("word", [3, 0xFF, 0x200, 0x103, 0x10000, 0x80000001])
def test_a_word_that_is_no_order_is_refused(torch_mod, sorter, word, key_value):
    """the timestamps are recorded, neither the arrays nor the storage are touched, VRDX_HIP_STATUS_ENQUEUE_REFUSED is raised
    -- for the direct and the indirect forms"""
    import vulkan_radix_sort_amd as vrdx
    keys, values, _ = _case("float-specials", 1025, "float64", False)
    values = values if key_value else None
    for device_count in (None, 1000):
        pool = vrdx.QueryPool(15)
        got = run64_ordered(torch_mod, sorter, keys, values, word, count=1025, device_count=device_count, pool=pool,
                            expect_refused=True)
        assert_same(*got, (keys, values), "a refused call changed the arrays")
        ts = pool.results_ns(0, 15)
        assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:]))
        pool.destroy()
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0   # (read and cleared above)


# ---- timestamps ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("device_count", [None, 900], ids=["direct", "indirect"])
def test_timestamps_in_all_15_slots(torch_mod, sorter, device_count, key_value):
    import vulkan_radix_sort_amd as vrdx
    keys, values, _ = _case("float-specials", 1025, "float64", True)
    values = values if key_value else None
    pool = vrdx.QueryPool(15)
    got = run64_ordered(torch_mod, sorter, keys, values, order_word("float64", True), count=1025, device_count=device_count,
                        pool=pool)
    assert_same(*got, expected(keys, values, "float64", True, count=min(device_count or 1025, 1025)))
    ts = pool.results_ns(0, 15)
    print("sort64 ordered %s slots (ns): %s" % ("pairs" if key_value else "keys", ts))
    assert len(ts) == 15 and ts[0] == 0 and all(b >= a for a, b in zip(ts, ts[1:])), ts
    assert all(t == ts[6] for t in ts[6:]), ts
    if not key_value:
        assert ts[3] == ts[2] and ts[6] == ts[5], ts
    pool.destroy()


# ---- capture and replay ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
def test_a_captured_call_replays_on_other_data(torch_mod, sorter, descending, key_value):
    """one captured call per direction (NULL query pool), replayed on keys it has not seen"""
    torch = torch_mod
    n, order = 70_001, "float64"
    word = order_word(order, descending)
    dk = torch.zeros(n, dtype=torch.int64, device="cuda")
    dv = torch.zeros(n, dtype=torch.int32, device="cuda") if key_value else None
    storage = torch.empty(sorter.storage_requirements64(n, key_value).size, dtype=torch.uint8, device="cuda")

    def record():
        stream = torch.cuda.current_stream().cuda_stream
        if key_value:
            sorter.cmd_sort64_ordered_key_value(stream, n, dk.data_ptr(), 0, dv.data_ptr(), 0, word, storage.data_ptr(), 0)
        else:
            sorter.cmd_sort64_ordered(stream, n, dk.data_ptr(), 0, word, storage.data_ptr(), 0)

    record()  # one eager call first, as the other capture tests do
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        record()
    stream = torch.cuda.current_stream().cuda_stream
    for builder in ("float-specials", "duplicates"):
        keys, values = case_keys(builder, n, order, descending, tag="replay")
        dk.copy_(torch.from_numpy(keys.view(np.int64).copy()))
        if key_value:
            dv.copy_(torch.from_numpy(values.view(np.int32).copy()))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_same(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if key_value else None,
                    expected(keys, values, order, descending), builder)
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
        assert sorter.read_sorter_status(stream) == 0


# ---- the Python front end --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
def test_sort64_of_float64_tensors_against_torch_sort(torch_mod, sorter, descending):
    """no NaNs and no zeros of both signs: totalOrder is torch.sort's order; stable=True makes the indices comparable"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    keys, _ = case_keys("float-values", 70_001, "float64", descending, tag="torch")
    keys[1::7] = keys[0:-1:7][:len(keys[1::7])]   # equal neighbours
    t = torch.from_numpy(keys.view(np.float64).copy()).cuda()
    want, index = torch.sort(t, stable=True, descending=descending)
    dk, dv = t.clone(), torch.arange(len(keys), dtype=torch.int32, device="cuda")
    vrdx.sort64(sorter, dk, dv, order="float64", descending=descending)
    keys_only = t.clone()
    vrdx.sort64(sorter, keys_only, order="float64", descending=descending)
    torch.cuda.synchronize()
    assert torch.equal(dk.view(torch.int64), want.view(torch.int64)) and torch.equal(dv.to(torch.int64), index)
    assert torch.equal(keys_only.view(torch.int64), want.view(torch.int64))
    # 8-byte integers holding the bits are taken too
    bits = t.view(torch.int64).clone()
    vrdx.sort64(sorter, bits, order="float64", descending=descending)
    torch.cuda.synchronize()
    assert torch.equal(bits, want.view(torch.int64))
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
def test_sort64_of_negative_int64_tensors_against_torch_sort(torch_mod, sorter, descending):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    keys, _ = case_keys("mixed-int", 70_001, "int64", descending, tag="torch")
    t = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    assert bool((t < 0).any()) and bool((t > 0).any())
    want, index = torch.sort(t, stable=True, descending=descending)
    dk, dv = t.clone(), torch.arange(len(keys), dtype=torch.int32, device="cuda")
    count = torch.tensor([len(keys)], dtype=torch.int32, device="cuda")
    vrdx.sort64(sorter, dk, dv, order="int64", descending=descending)
    by_count = t.clone()
    vrdx.sort64(sorter, by_count, count=count, order="int64", descending=descending)
    torch.cuda.synchronize()
    assert torch.equal(dk, want) and torch.equal(dv.to(torch.int64), index) and torch.equal(by_count, want)
    # order=None stays the unsigned sort: the negative entries behind the others
    unsigned = t.clone()
    vrdx.sort64(sorter, unsigned)
    torch.cuda.synchronize()
    assert np.array_equal(unsigned.cpu().numpy().view(np.uint64), np.sort(keys))
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0


# ---- the single header -----------------------------------------------------------------------------------------------------------

SINGLE_HEADER_CASE = r"""
#define VRDX_IMPLEMENTATION
#include "vk_radix_sort.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>

static uint64_t T(uint64_t k, uint32_t order) {
  const uint32_t type = order & 0xFFu;
  uint64_t flip = type == VRDX_HIP_KEY_UINT64 ? 0 : 1ull << 63;
  if (order & VRDX_HIP_ORDER_DESCENDING) flip = ~flip;
  return k ^ flip ^ (type == VRDX_HIP_KEY_FLOAT64 && (k >> 63) ? 0x7FFFFFFFFFFFFFFFull : 0);
}

static size_t Run(VrdxSorter sorter, uint32_t n, uint32_t order, bool keyValue) {
  const uint32_t len = n + 3;
  std::vector<uint64_t> keys(len);
  std::vector<uint32_t> values(len);
  uint64_t x = 88172645463325252ull + n + order;
  for (uint32_t i = 0; i < len; ++i) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    keys[i] = (i % 3 == 0) ? (x & 0xFFF80000000000FFull) : x;  // duplicates of both words, both signs
    values[i] = i * 2654435761u ^ 0x80000000u;  // not the index
  }
  VrdxSorterStorageRequirements req;
  if (keyValue) vrdxHipGetSorter64KeyValueStorageRequirements(sorter, n, &req);
  else vrdxHipGetSorter64StorageRequirements(sorter, n, &req);
  uint64_t* dk; uint32_t* dv; uint8_t* st;
  if (hipMalloc(&dk, 8ull * len) != hipSuccess || hipMalloc(&dv, 4ull * len) != hipSuccess ||
      hipMalloc(&st, req.size) != hipSuccess)
    return ~(size_t)0;
  (void)hipMemcpy(dk, keys.data(), 8ull * len, hipMemcpyHostToDevice);
  (void)hipMemcpy(dv, values.data(), 4ull * len, hipMemcpyHostToDevice);
  if (keyValue)
    vrdxHipCmdSort64OrderedKeyValue(nullptr, sorter, n, (VkBuffer)dk, 0, (VkBuffer)dv, 0, order, (VkBuffer)st, 0, nullptr, 0);
  else
    vrdxHipCmdSort64Ordered(nullptr, sorter, n, (VkBuffer)dk, 0, order, (VkBuffer)st, 0, nullptr, 0);
  std::vector<uint64_t> gk(len);
  std::vector<uint32_t> gv(len);
  (void)hipMemcpy(gk.data(), dk, 8ull * len, hipMemcpyDeviceToHost);
  (void)hipMemcpy(gv.data(), dv, 4ull * len, hipMemcpyDeviceToHost);
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return T(keys[a], order) < T(keys[b], order); });
  size_t bad = 0;
  for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[idx[i]] || gv[i] != (keyValue ? values[idx[i]] : values[i]);
  for (uint32_t i = n; i < len; ++i) bad += gk[i] != keys[i] || gv[i] != values[i];  // from n on: as they were
  (void)hipFree(dk); (void)hipFree(dv); (void)hipFree(st);
  return bad;
}

int main() {
  VrdxSorterCreateInfo info = {};
  VrdxSorter sorter = nullptr;
  if (vrdxCreateSorter(&info, &sorter) != VK_SUCCESS) { std::printf("no sorter\n"); return 2; }
  size_t bad = 0;
  bad += Run(sorter, 70001u, VRDX_HIP_KEY_FLOAT64 | VRDX_HIP_ORDER_DESCENDING, true);
  bad += Run(sorter, 70001u, VRDX_HIP_KEY_INT64, false);
  const uint32_t status = vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("status %u, %zu mismatches\n", status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
"""


def test_single_header_ordered_parity(tmp_path):
    """The ordered entry points through the single header's own launcher (the kernels resolved by their mangled names from
    the one list, vrdx_launch.inc), compiled with plain g++: float64 descending key+value and int64 keys-only against
    std::stable_sort by T."""
    header = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
    if not os.path.exists(header) or "split64_ordered_kernel" not in open(header).read():
        subprocess.run(["python3", os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", header], check=True)
    text = open(header).read()
    for kernel in ("split64_ordered_kernel", "merge64_ordered_kernel", "gather_hi64_ordered_kernel", "permute64_ordered_kernel",
                   "segmented_small64_ordered_kernel", "segmented_mid64_ordered_kernel", "segmented_large64_ordered_kernel"):
        assert kernel in text, kernel
    src = tmp_path / "sort64_ordered_single_header.cc"
    src.write_text(SINGLE_HEADER_CASE)
    exe = tmp_path / "sort64_ordered_single_header"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.dirname(header), str(src), "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "status 0, 0 mismatches" in r.stdout, r.stdout + r.stderr
