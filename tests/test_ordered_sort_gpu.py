"""GPU: vrdxHipCmdOrderedSort[KeyValue][Indirect] -- int32, float32 and descending orders of the flat 32-bit sorts -- bit for
bit against the references of tests/key_order32_cases.py (np.argsort(T(keys), kind="stable")), between guard bytes
(tests/ordered_guarded_call.py): every order, direction and mode at the one-workgroup sizes, at the first streaming sizes
(every n mod 4) and at one size inside each further plan the planner reports; alignments; device-side counts; order word 0
against the twin; refused words; the ballot ranking; timestamps; capture and replay; the single header; the torch front end."""
import os
import subprocess

import numpy as np
import pytest

from key_order32_cases import DIRECTIONS, ORDERS, assert_same, case_keys, expected, order_word
from ordered_guarded_call import ballot_sorter, ordered_call, sorter, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE_WORKGROUP = (0, 1, 2, 255, 256, 257, 4096, 16383, 16384)
FIRST_STREAMING = (16385, 16386, 16387, 16388)
MODES = pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
EVERY_ORDER = pytest.mark.parametrize("order,descending", [(o, d) for o in ORDERS for d in DIRECTIONS],
                                      ids=[f"{o}-{'descending' if d else 'ascending'}" for o in ORDERS for d in DIRECTIONS])


def _builder(order):
    return {"uint32": "duplicates", "int32": "mixed-int", "float32": "float-specials"}[order]


def _check(torch, sorter, builder, n, order, descending, key_value, tag="", **kw):
    keys, values = case_keys(builder, n, order, descending, tag)
    values = values if key_value else None
    got = ordered_call(torch, sorter, keys, values, order=order_word(order, descending), **kw)
    assert_same(got.keys, got.values, expected(keys, values, order, descending), f"{builder} n={n} {order} {descending} {kw}")
    return got


def _further_plans(sorter, key_value):
    """(name, size) of one size inside each plan describe_plan reports beyond the first streaming sizes, up to the first size
    of the MSD plan (found by bisection): taken from the planner, not hand-kept"""
    seen, out, n = {sorter.describe_plan(FIRST_STREAMING[-1], key_value).name}, [], 2 * FIRST_STREAMING[0] + 3
    while n < (1 << 28):
        name = sorter.describe_plan(n, key_value).name
        if name == "msd":
            lo, hi = n // 2, n   # (lo: not msd, hi: msd)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if sorter.describe_plan(mid, key_value).name == "msd" else (mid, hi)
            out.append(("msd", hi))
            break
        if name not in seen or not out:
            out.append((name, n))
        seen.add(name)
        n = 2 * n + 1
    return out


@EVERY_ORDER
@MODES
def test_every_order_direction_and_mode(torch_mod, sorter, order, descending, key_value):
    for n in ONE_WORKGROUP + FIRST_STREAMING:
        _check(torch_mod, sorter, _builder(order), n, order, descending, key_value)
    for builder in ("ones-in-T", "all-equal", "plus-minus-x"):
        for n in (257, 5000, 16384, 16387):
            _check(torch_mod, sorter, builder, n, order, descending, key_value)
    plans = _further_plans(sorter, key_value)
    assert plans and plans[-1][0] == "msd", plans
    for name, n in plans[:-1]:
        _check(torch_mod, sorter, _builder(order), n, order, descending, key_value, tag=name)
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


@MODES
def test_the_first_size_of_the_msd_plan(torch_mod, sorter, key_value):
    name, n = _further_plans(sorter, key_value)[-1]
    assert sorter.describe_plan(n - 1, key_value).name != "msd" and sorter.describe_plan(n, key_value).name == "msd"
    info, twin = sorter.describe_ordered_sort_plan(n, key_value, order_word("float32", True)), sorter.describe_plan(n, key_value)
    assert (info.name, info.launches, info.bytesPerElement) == ("msd", twin.launches + 2, twin.bytesPerElement + 16)
    _check(torch_mod, sorter, "float-specials", n, "float32", True, key_value)


@EVERY_ORDER
def test_keys_and_values_at_every_4_byte_alignment(torch_mod, sorter, order, descending):
    for i, n in enumerate(FIRST_STREAMING):
        for keys_off in (0, 4, 8, 12):
            values_off = (keys_off + 4 * i + 4) % 16
            _check(torch_mod, sorter, _builder(order), n, order, descending, False, keys_off=keys_off)
            _check(torch_mod, sorter, _builder(order), n, order, descending, True, keys_off=keys_off, values_off=values_off,
                   storage_off=16 * (1 + i))


@EVERY_ORDER
@MODES
def test_a_device_side_count(torch_mod, sorter, order, descending, key_value):
    """elements from min(count, bound) on lie between the sorted ones and the guard bytes and must be bit-identical to the
    input (float-specials: NaN payloads among them), values included"""
    for bound, counts in ((16384, (0, 1, 5, 16383, 16384, 16391)), (40000, (0, 1, 5, 16384, 16385, 39999, 40000, 40007))):
        keys, values = case_keys("float-specials", bound, order, descending, "count")
        values = values if key_value else None
        for i, count in enumerate(counts):
            got = ordered_call(torch_mod, sorter, keys, values, order=order_word(order, descending), device_count=count,
                               indirect_off=4 * (i % 4))
            assert_same(got.keys, got.values, expected(keys, values, order, descending, count=count), f"count {count} of {bound}")


@pytest.mark.parametrize("n", [1, 4097, 16384, 16385, 40000])
@MODES
def test_order_word_0_is_the_twin(torch_mod, sorter, n, key_value):
    """VRDX_HIP_KEY32_UINT32 records what vrdxCmdSort[KeyValue][Indirect] records: the same arrays, the same header words, the
    same plan"""
    keys, values = case_keys("uniform", n, "uint32", False)
    values = values if key_value else None
    for device_count in (None, n - n // 3):
        got = ordered_call(torch_mod, sorter, keys, values, order=0, device_count=device_count)
        twin = ordered_call(torch_mod, sorter, keys, values, order=None, device_count=device_count, twin=True)
        assert_same(got.keys, got.values, (twin.keys, twin.values))
        assert_same(got.keys, got.values, expected(keys, values, "uint32", False, count=device_count))
        assert torch_mod.equal(got.storage[:16], twin.storage[:16])
    a, b = sorter.describe_ordered_sort_plan(n, key_value, 0), sorter.describe_plan(n, key_value)
    assert bytes(a) == bytes(b)


@pytest.mark.parametrize("word", [3, 0x200, 0x103, 0x10000 | 2, 0xFFFFFFFF])
@MODES
def test_a_word_that_is_no_order_is_refused(torch_mod, sorter, word, key_value):
    import vulkan_radix_sort_amd as vrdx
    assert sorter.describe_ordered_sort_plan(20000, key_value, word).name == "none"
    for n in (1000, 20000):
        keys, values = case_keys("float-specials", n, "float32", False, "refused")
        values = values if key_value else None
        for device_count in (None, 900):
            pool = vrdx.QueryPool(15)
            got = ordered_call(torch_mod, sorter, keys, values, order=word, device_count=device_count, pool=pool,
                               expect_refused=True)
            assert_same(got.keys, got.values, (keys, values))
            ts = pool.results_ns(0, 15)
            assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:]))
            pool.destroy()


@EVERY_ORDER
def test_the_ballot_ranking(torch_mod, ballot_sorter, order, descending):
    for n in (257, 5000, 16384, 16387, 40001):
        for key_value in (False, True):
            _check(torch_mod, ballot_sorter, _builder(order), n, order, descending, key_value, tag="ballot")
    assert ballot_sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize("n", [5000, 16387, 100003])
@MODES
def test_timestamps(torch_mod, sorter, n, key_value):
    import vulkan_radix_sort_amd as vrdx
    pool = vrdx.QueryPool(15)
    _check(torch_mod, sorter, "float-specials", n, "float32", True, key_value, tag="stamps", pool=pool)
    ts = pool.results_ns(0, 15)
    print("ordered sort n=%d %s slots (ns): %s" % (n, "pairs" if key_value else "keys", ts))
    assert len(ts) == 15 and ts[0] == 0 and all(b >= a for a, b in zip(ts, ts[1:])), ts
    if n > 16384:
        assert ts[1] > ts[0] and ts[14] > ts[13] and ts[13] > ts[1], ts   # the two transforms, the twin between them
    else:
        assert all(t == ts[0] for t in ts[:14]) and ts[14] > ts[13], ts      # the ONE_WORKGROUP contract
    pool.destroy()


@MODES
def test_a_captured_call_replays_on_other_data_and_another_count(torch_mod, sorter, key_value):
    torch = torch_mod
    bound, order, descending = 70_001, "float32", True
    word = order_word(order, descending)
    dk = torch.zeros(bound, dtype=torch.int32, device="cuda")
    dv = torch.zeros(bound, dtype=torch.int32, device="cuda") if key_value else None
    dc = torch.tensor([bound], dtype=torch.int32, device="cuda")
    req = sorter.key_value_storage_requirements(bound) if key_value else sorter.storage_requirements(bound)
    storage = torch.empty(req.size, dtype=torch.uint8, device="cuda")

    def record():
        stream = torch.cuda.current_stream().cuda_stream
        if key_value:
            sorter.cmd_ordered_sort_key_value_indirect(stream, bound, dc.data_ptr(), 0, dk.data_ptr(), 0, dv.data_ptr(), 0, word,
                                                       storage.data_ptr(), 0)
        else:
            sorter.cmd_ordered_sort_indirect(stream, bound, dc.data_ptr(), 0, dk.data_ptr(), 0, word, storage.data_ptr(), 0)

    record()  # one eager call first, as the other capture tests do
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        record()
    stream = torch.cuda.current_stream().cuda_stream
    for builder, count in (("float-specials", bound), ("duplicates", 33_333), ("mixed-int", 9)):
        keys, values = case_keys(builder, bound, order, descending, tag="replay")
        dk.copy_(torch.from_numpy(keys.view(np.int32).copy()))
        if key_value:
            dv.copy_(torch.from_numpy(values.view(np.int32).copy()))
        dc.fill_(count)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_same(dk.cpu().numpy().view(np.uint32), dv.cpu().numpy().view(np.uint32) if key_value else None,
                    expected(keys, values if key_value else None, order, descending, count=count), builder)
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
        assert sorter.read_sorter_status(stream) == 0


@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
def test_sort_ordered_against_torch_sort(torch_mod, sorter, descending):
    """float32 without NaNs and zeros, and int32 of both signs: where totalOrder is torch.sort's order; stable=True makes the
    indices comparable"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    for n in (5000, 70_001):
        keys, _ = case_keys("float-values", n, "float32", descending, tag="torch")
        keys[1::7] = keys[0:-1:7][:len(keys[1::7])]   # equal neighbours
        t = torch.from_numpy(keys.view(np.float32).copy()).cuda()
        want, index = torch.sort(t, stable=True, descending=descending)
        dk, dv = t.clone(), torch.arange(n, dtype=torch.int32, device="cuda")
        vrdx.sort_ordered(sorter, dk, dv, order="float32", descending=descending)
        bits = t.view(torch.int32).clone()   # 4-byte integers holding the bits are taken too
        vrdx.sort_ordered(sorter, bits, order="float32", descending=descending)
        torch.cuda.synchronize()
        assert torch.equal(dk.view(torch.int32), want.view(torch.int32)) and torch.equal(dv.to(torch.int64), index)
        assert torch.equal(bits, want.view(torch.int32))
        keys, _ = case_keys("mixed-int", n, "int32", descending, tag="torch")
        t = torch.from_numpy(keys.view(np.int32).copy()).cuda()
        assert bool((t < 0).any()) and bool((t > 0).any())
        want, index = torch.sort(t, stable=True, descending=descending)
        dk, dv = t.clone(), torch.arange(n, dtype=torch.int32, device="cuda")
        count = torch.tensor([n], dtype=torch.int32, device="cuda")
        vrdx.sort_ordered(sorter, dk, dv, count=count, order="int32", descending=descending)
        torch.cuda.synchronize()
        assert torch.equal(dk, want) and torch.equal(dv.to(torch.int64), index)
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0


SINGLE_HEADER_CASE = r"""
#define VRDX_IMPLEMENTATION
#include "vk_radix_sort.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>

static uint32_t T(uint32_t k, uint32_t order) {
  const uint32_t type = order & 0xFFu;
  uint32_t flip = type == VRDX_HIP_KEY32_UINT32 ? 0u : 1u << 31;
  if (order & VRDX_HIP_ORDER_DESCENDING) flip = ~flip;
  return k ^ flip ^ (type == VRDX_HIP_KEY32_FLOAT32 && (k >> 31) ? 0x7FFFFFFFu : 0u);
}

// segments == 0: the flat call; otherwise `segments` equal segments over [0, n)
static size_t Run(VrdxSorter sorter, uint32_t n, uint32_t order, bool keyValue, uint32_t segments) {
  const uint32_t len = n + 3;
  std::vector<uint32_t> keys(len), values(len), offsets(segments + 1);
  uint64_t x = 88172645463325252ull + n + order;
  for (uint32_t i = 0; i < len; ++i) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    keys[i] = (i % 3 == 0) ? (uint32_t)(x & 0xFFC000FFu) : (uint32_t)x;  // duplicates, both signs
    values[i] = i * 2654435761u ^ 0x80000000u;  // not the index
  }
  for (uint32_t s = 0; s <= segments; ++s) offsets[s] = (uint32_t)((uint64_t)n * s / (segments ? segments : 1));
  VrdxSorterStorageRequirements req;
  if (keyValue) vrdxGetSorterKeyValueStorageRequirements(sorter, n, &req);
  else vrdxGetSorterStorageRequirements(sorter, n, &req);
  uint32_t *dk, *dv, *dof; uint8_t* st;
  if (hipMalloc(&dk, 4ull * len) != hipSuccess || hipMalloc(&dv, 4ull * len) != hipSuccess ||
      hipMalloc(&dof, 4ull * (segments + 1)) != hipSuccess || hipMalloc(&st, req.size) != hipSuccess)
    return ~(size_t)0;
  (void)hipMemcpy(dk, keys.data(), 4ull * len, hipMemcpyHostToDevice);
  (void)hipMemcpy(dv, values.data(), 4ull * len, hipMemcpyHostToDevice);
  (void)hipMemcpy(dof, offsets.data(), 4ull * (segments + 1), hipMemcpyHostToDevice);
  if (segments == 0 && keyValue)
    vrdxHipCmdOrderedSortKeyValue(nullptr, sorter, n, (VkBuffer)dk, 0, (VkBuffer)dv, 0, order, (VkBuffer)st, 0, nullptr, 0);
  else if (segments == 0)
    vrdxHipCmdOrderedSort(nullptr, sorter, n, (VkBuffer)dk, 0, order, (VkBuffer)st, 0, nullptr, 0);
  else if (keyValue)
    vrdxHipCmdOrderedSortSegmentedKeyValue(nullptr, sorter, n, segments, (VkBuffer)dof, 0, (VkBuffer)dk, 0, (VkBuffer)dv, 0, order,
                                           (VkBuffer)st, 0, nullptr, 0);
  else
    vrdxHipCmdOrderedSortSegmented(nullptr, sorter, n, segments, (VkBuffer)dof, 0, (VkBuffer)dk, 0, order, (VkBuffer)st, 0, nullptr, 0);
  std::vector<uint32_t> gk(len), gv(len);
  (void)hipMemcpy(gk.data(), dk, 4ull * len, hipMemcpyDeviceToHost);
  (void)hipMemcpy(gv.data(), dv, 4ull * len, hipMemcpyDeviceToHost);
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  const auto less = [&](uint32_t a, uint32_t b) { return T(keys[a], order) < T(keys[b], order); };
  if (segments == 0) std::stable_sort(idx.begin(), idx.end(), less);
  for (uint32_t s = 0; s < segments; ++s) std::stable_sort(idx.begin() + offsets[s], idx.begin() + offsets[s + 1], less);
  size_t bad = 0;
  for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[idx[i]] || gv[i] != (keyValue ? values[idx[i]] : values[i]);
  for (uint32_t i = n; i < len; ++i) bad += gk[i] != keys[i] || gv[i] != values[i];  // from n on: as they were
  (void)hipFree(dk); (void)hipFree(dv); (void)hipFree(dof); (void)hipFree(st);
  return bad;
}

int main() {
  VrdxSorterCreateInfo info = {};
  VrdxSorter sorter = nullptr;
  if (vrdxCreateSorter(&info, &sorter) != VK_SUCCESS) { std::printf("no sorter\n"); return 2; }
  size_t bad = 0;
  bad += Run(sorter, 5000u, VRDX_HIP_KEY32_FLOAT32 | VRDX_HIP_ORDER_DESCENDING, true, 0);
  bad += Run(sorter, 70001u, VRDX_HIP_KEY32_FLOAT32 | VRDX_HIP_ORDER_DESCENDING, true, 0);
  bad += Run(sorter, 70001u, VRDX_HIP_KEY32_INT32, false, 0);
  bad += Run(sorter, 70001u, VRDX_HIP_KEY32_FLOAT32, true, 3);   // 23333: the large class
  bad += Run(sorter, 70001u, VRDX_HIP_KEY32_INT32 | VRDX_HIP_ORDER_DESCENDING, false, 9);   // the mid class
  const uint32_t status = vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("status %u, %zu mismatches\n", status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
"""


def test_single_header_ordered_parity(tmp_path):
    """The ordered 32-bit entry points through the single header's own launcher (the kernels resolved by their mangled names
    from the lists of vrdx_launch.inc), compiled with plain g++, against std::stable_sort by T."""
    header = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
    if not os.path.exists(header) or "order32_kernel" not in open(header).read():
        subprocess.run(["python3", os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", header], check=True)
    text = open(header).read()
    for kernel in ("small_sort_ordered_kernel", "order32_kernel", "segmented_small_ordered_kernel", "segmented_mid_ordered_kernel",
                   "segmented_large_ordered_kernel", "vrdxHipCmdOrderedSortSegmentedKeyValue"):
        assert kernel in text, kernel
    src = tmp_path / "ordered_sort_single_header.cc"
    src.write_text(SINGLE_HEADER_CASE)
    exe = tmp_path / "ordered_sort_single_header"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.dirname(header), str(src), "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "status 0, 0 mismatches" in r.stdout, r.stdout + r.stderr
