"""GPU tests of the 64-bit sorts (vrdxHipCmdSort64[KeyValue], vulkan_radix_sort_amd.sort64), through the C ABI and element
for element against numpy: keys-only against np.sort of the uint64 keys, key+value against np.argsort(kind="stable")
applied to keys and to values (distinct values over duplicate-heavy keys prove stability; where a test says payload64 they
are nowhere their own index, which a sort that hands out the index for the value needs to pass).  Every case runs with
guard words around the keys, the values and the storage requirement, and reads the status words afterwards.  The key
patterns, the values and the reference are those of tests/sort64_model.py."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from guarded_call import BAND_BYTE as STORAGE_GUARD
from guarded_call import ballot_sorter, guarded_call, sorter, torch_mod  # noqa: F401
from sort64_model import check64, expected64, make_keys64, payload64  # noqa: F401 (shared with test_sort64_edges_gpu.py)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 1000, 16384, 16385, (1 << 18) + 3, 1 << 22, 8_200_000]  # every plan of the inner sorts
PATTERNS = ["uniform", "high-constant", "low-constant", "identical", "descending", "8-distinct", "bit63-mixed", "tile-depth"]


def run64(torch, s, keys, values=None, keys_off=0, values_off=0, storage_off=0, pool=None, count=None, storage_out=None):
    """One call through the C ABI (guarded_call).  count (default: all of keys) elements are sorted; the rest of `keys` /
    `values` is followed by guard bytes.  The sorter's sticky word must be 0 afterwards.  Returns the whole arrays as the
    device left them; storage_out: a list that receives the storage tensor (its header is at storage_off)."""
    got = guarded_call(torch, s, keys, values, count=count, keys_off=keys_off, values_off=values_off, storage_off=storage_off,
                       pool=pool, sticky=0)
    if storage_out is not None:
        storage_out.append(got.storage)
    return got.keys, got.values


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_sort64_matches_numpy(torch_mod, sorter, n, pattern, key_value):
    rng = np.random.default_rng(zlib.crc32(f"{n}/{pattern}/{key_value}".encode()))
    keys = make_keys64(pattern, n + 5, rng)  # five elements behind elementCount
    values = payload64(n + 5) if key_value else None
    got_keys, got_values = run64(torch_mod, sorter, keys, values, count=n)
    check64(got_keys, got_values, keys, values, count=n)


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_sort64_of_2_pow_25_uniform_keys(torch_mod, sorter, key_value):
    n = 1 << 25
    rng = np.random.default_rng(25 + key_value)
    keys = make_keys64("uniform", n, rng)
    values = np.arange(n, dtype=np.uint32) if key_value else None
    got_keys, got_values = run64(torch_mod, sorter, keys, values)
    check64(got_keys, got_values, keys, values)


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("pattern", ["uniform", "8-distinct"])
@pytest.mark.parametrize("ranking", ["atomic", "ballot"])
def test_both_ranking_modes(torch_mod, sorter, ballot_sorter, ranking, pattern, key_value):
    s = sorter if ranking == "atomic" else ballot_sorter
    n = (1 << 18) + 3
    rng = np.random.default_rng(zlib.crc32(f"{ranking}/{pattern}/{key_value}".encode()))
    keys = make_keys64(pattern, n, rng)
    values = np.arange(n, dtype=np.uint32) if key_value else None
    got_keys, got_values = run64(torch_mod, s, keys, values)
    check64(got_keys, got_values, keys, values)


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("n", [3, 1001, 70_002, (1 << 20) + 1])
def test_unaligned_arrays_and_a_storage_offset(torch_mod, sorter, n, key_value):
    """Keys that are 8-byte but not 16-byte aligned, values that are 4-byte but not 16-byte aligned, a storage offset that is
    16-byte but not 128-byte aligned, counts that are not multiples of 4."""
    rng = np.random.default_rng(n)
    keys = make_keys64("tile-depth", n + 3, rng)
    keys[::5] = keys[1]
    values = np.arange(n + 3, dtype=np.uint32) if key_value else None
    got_keys, got_values = run64(torch_mod, sorter, keys, values, keys_off=8, values_off=4, storage_off=48, count=n)
    check64(got_keys, got_values, keys, values, count=n)


def test_an_empty_sort_touches_nothing(torch_mod, sorter):
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    keys = np.arange(100, 0, -1, dtype=np.uint64)
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    dv = torch.arange(100, dtype=torch.int32, device="cuda")
    storage = torch.full((sorter.storage_requirements64(100, True).size,), STORAGE_GUARD, dtype=torch.uint8, device="cuda")
    import vulkan_radix_sort_amd as vrdx
    pool = vrdx.QueryPool(15)
    sorter.cmd_sort64(stream, 0, dk.data_ptr(), 0, storage.data_ptr(), 0)
    sorter.cmd_sort64_key_value(stream, 0, dk.data_ptr(), 0, dv.data_ptr(), 0, storage.data_ptr(), 0, pool, 0)
    torch.cuda.synchronize()
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), keys)
    assert np.array_equal(dv.cpu().numpy(), np.arange(100, dtype=np.int32))
    assert bool((storage == STORAGE_GUARD).all())
    ts = pool.results_ns(0, 15)  # all 15 slots recorded
    assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:]))
    pool.destroy()


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_timestamp_slots(torch_mod, sorter, key_value):
    """All 15 slots, non-decreasing; the documented slot pairs are non-zero at N = 2^22, the others coincide."""
    import vulkan_radix_sort_amd as vrdx
    n = 1 << 22
    rng = np.random.default_rng(64)
    keys = make_keys64("uniform", n, rng)
    values = np.arange(n, dtype=np.uint32) if key_value else None
    pool = vrdx.QueryPool(15)
    got_keys, got_values = run64(torch_mod, sorter, keys, values, pool=pool)
    check64(got_keys, got_values, keys, values)
    ts = pool.results_ns(0, 15)
    print("sort64 %s n=%d slots (ns): %s" % ("pairs" if key_value else "keys", n, ts))
    assert len(ts) == 15 and ts[0] == 0
    assert all(b >= a for a, b in zip(ts, ts[1:])), ts
    assert ts[14] == max(ts) and ts[14] > 0
    steps = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6)] if key_value else [(0, 1), (1, 2), (3, 4), (4, 5)]
    for a, b in steps:
        assert ts[b] > ts[a], (a, b, ts)
    last = 6 if key_value else 5
    assert all(t == ts[last] for t in ts[last:]), ts
    if not key_value:
        assert ts[3] == ts[2], ts
    pool.destroy()


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_captured_graph_replays_on_new_data(torch_mod, sorter, key_value):
    """One call captured once in torch.cuda.graph (one stream, a linear graph) sorts whatever it is replayed on: three inputs
    of the same count, among them one whose words are constant (the inner sorts decide that on the device at every replay)."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    n = (1 << 20) + 2
    rng = np.random.default_rng(99)
    dk = torch.zeros(n, dtype=torch.int64, device="cuda")
    dv = torch.zeros(n, dtype=torch.int32, device="cuda") if key_value else None
    storage = torch.empty(sorter.storage_requirements64(n, key_value).size, dtype=torch.uint8, device="cuda")
    vrdx.sort64(sorter, dk, dv, storage=storage)  # one eager call first, as the other capture tests do
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vrdx.sort64(sorter, dk, dv, storage=storage)
    values = payload64(n)
    for pattern in ("uniform", "high-constant", "8-distinct"):
        keys = make_keys64(pattern, n, rng)
        dk.copy_(torch.from_numpy(keys.view(np.int64)))
        if key_value:
            dv.copy_(torch.from_numpy(values.view(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if key_value else None, keys,
                values if key_value else None)
        stream = torch.cuda.current_stream().cuda_stream
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
        assert sorter.read_sorter_status(stream) == 0


def test_sort64_python_front_end(torch_mod, sorter):
    """sort64 on int64 tensors: keys-only, with values, and with a caller's storage that is larger than needed."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    n = 123_457
    rng = np.random.default_rng(5)
    keys = make_keys64("tile-depth", n, rng)
    iota = np.arange(n, dtype=np.uint32)
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    storage = vrdx.sort64(sorter, dk)
    torch.cuda.synchronize()
    assert storage.numel() == sorter.storage_requirements64(n).size
    check64(dk.cpu().numpy().view(np.uint64), None, keys, None)
    assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    dv = torch.from_numpy(iota.view(np.int32).copy()).cuda()
    storage = vrdx.sort64(sorter, dk, dv)
    torch.cuda.synchronize()
    assert storage.numel() == sorter.storage_requirements64(n, key_value=True).size
    check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32), keys, iota)
    own = torch.empty(sorter.storage_requirements64(n, key_value=True).size + 4096, dtype=torch.uint8, device="cuda")
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    dv = torch.from_numpy(iota.view(np.int32).copy()).cuda()
    assert vrdx.sort64(sorter, dk, dv, storage=own) is own
    torch.cuda.synchronize()
    check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32), keys, iota)
    with pytest.raises(ValueError):
        vrdx.sort64(sorter, dk, dv, storage=own[:1024])
    # storage off a 16-byte boundary is refused (the front end passes storageOffset 0: the contract falls on the address),
    # at every residue, and nothing is recorded: the keys stay as they are
    assert own.data_ptr() % 16 == 0
    before = dk.clone()
    for shift in (4, 8, 12, 1):
        with pytest.raises(ValueError, match="16-byte"):
            vrdx.sort64(sorter, dk, dv, storage=own[shift:])
    assert vrdx.sort64(sorter, dk, dv, storage=own[16:]) is not None   # (a multiple of 16 is fine: 4096 spare bytes)
    torch.cuda.synchronize()
    assert bool((dk == before).all())                                     # sorted input stays as it is
    assert sorter.read_sorter_status(stream) == 0


SINGLE_HEADER_CASE = r"""
#define VRDX_IMPLEMENTATION
#include "vk_radix_sort.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>

static size_t Run(VrdxSorter sorter, uint32_t n, bool keyValue) {
  std::vector<uint64_t> keys(n);
  std::vector<uint32_t> values(n);
  uint64_t x = 88172645463325252ull + n;
  for (uint32_t i = 0; i < n; ++i) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    keys[i] = (i % 3 == 0) ? (x & 0xFFFF0000000000FFull) : x;  // duplicates of both words
    values[i] = i * 2654435761u ^ 0x80000000u;  // not the index: a sort that hands out I[j] for values[I[j]] fails
  }
  VrdxSorterStorageRequirements req;
  if (keyValue) vrdxHipGetSorter64KeyValueStorageRequirements(sorter, n, &req);
  else vrdxHipGetSorter64StorageRequirements(sorter, n, &req);
  uint64_t* dk; uint32_t* dv; uint8_t* st;
  if (hipMalloc(&dk, 8ull * n) != hipSuccess || hipMalloc(&dv, 4ull * n) != hipSuccess || hipMalloc(&st, req.size) != hipSuccess)
    return ~(size_t)0;
  (void)hipMemcpy(dk, keys.data(), 8ull * n, hipMemcpyHostToDevice);
  (void)hipMemcpy(dv, values.data(), 4ull * n, hipMemcpyHostToDevice);
  if (keyValue) vrdxHipCmdSort64KeyValue(nullptr, sorter, n, (VkBuffer)dk, 0, (VkBuffer)dv, 0, (VkBuffer)st, 0, nullptr, 0);
  else vrdxHipCmdSort64(nullptr, sorter, n, (VkBuffer)dk, 0, (VkBuffer)st, 0, nullptr, 0);
  std::vector<uint64_t> gk(n);
  std::vector<uint32_t> gv(n);
  (void)hipMemcpy(gk.data(), dk, 8ull * n, hipMemcpyDeviceToHost);
  (void)hipMemcpy(gv.data(), dv, 4ull * n, hipMemcpyDeviceToHost);
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  size_t bad = 0;
  for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[idx[i]] || (keyValue && gv[i] != values[idx[i]]);
  (void)hipFree(dk); (void)hipFree(dv); (void)hipFree(st);
  return bad;
}

int main() {
  VrdxSorterCreateInfo info = {};
  VrdxSorter sorter = nullptr;
  if (vrdxCreateSorter(&info, &sorter) != VK_SUCCESS) { std::printf("no sorter\n"); return 2; }
  size_t bad = 0;
  for (uint32_t n : {40003u, (1u << 21) + 1u})
    for (bool keyValue : {false, true}) bad += Run(sorter, n, keyValue);
  const uint32_t status = vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("status %u, %zu mismatches\n", status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
"""


def test_single_header_sort64_parity(tmp_path):
    """The 64-bit entry points through the single header's own launcher (vrdx_module_launch.inc: the kernels resolved by
    mangled name), compiled with plain g++: two sizes, keys-only and key+value, against std::stable_sort."""
    header = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
    if not os.path.exists(header):
        subprocess.run(["python3", os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", header], check=True)
    src = tmp_path / "sort64_single_header.cc"
    src.write_text(SINGLE_HEADER_CASE)
    exe = tmp_path / "sort64_single_header"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.dirname(header), str(src), "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "status 0, 0 mismatches" in r.stdout, r.stdout + r.stderr
