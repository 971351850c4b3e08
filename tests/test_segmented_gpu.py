"""GPU tests of the segmented sort (vrdxHipCmdSortSegmented[KeyValue], vulkan_radix_sort_amd.sort_segments): every segment
must come out as a stable ascending sort of itself -- checked against the oracle for segments of up to 16385 elements and
against np.lexsort((keys, segment id)) for the whole call -- with nothing touched outside the segments, whatever size class
the device put each segment in, with both ranking modes, through a captured graph replayed on another segmentation, and
through the single header's own launcher."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from guarded_call import ballot_sorter, sorter, to_device, to_host, torch_mod  # noqa: F401
from segmented_cases import GUARD, check, expected, make_keys, mixed_offsets, run_segmented

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 32768, 36865, 1 << 20]


@pytest.mark.parametrize("ranking", ["atomic", "ballot"])
@pytest.mark.parametrize("kind", ["uniform", "all-equal", "descending", "8-bit", "24-bit"])
def test_every_size_class_in_one_call(torch_mod, sorter, ballot_sorter, oracle, ranking, kind):
    """Segments of 0 ... 2^20 elements (every class boundary) shuffled into one call, o[0] > 0 and a tail behind the last
    segment, every buffer at a non-zero offset; keys-only and key+value with iota values (stability)."""
    s = sorter if ranking == "atomic" else ballot_sorter
    rng = np.random.default_rng(zlib.crc32(f"{ranking}/{kind}".encode()))
    offsets, n = mixed_offsets(rng, SIZES)
    keys = make_keys(kind, n, rng)
    iota = np.arange(n, dtype=np.uint32)
    gk, _, _ = run_segmented(torch_mod, s, keys, offsets, keys_off=12, offsets_off=8, storage_off=48)
    check(gk, None, keys, None, offsets, oracle)
    gk, gv, _ = run_segmented(torch_mod, s, keys, offsets, iota, keys_off=4, values_off=20, offsets_off=4, storage_off=16)
    check(gk, gv, keys, iota, offsets, oracle)


@pytest.mark.parametrize("key_value", [False, True])
def test_one_segment_of_four_million(torch_mod, sorter, key_value):
    n = 1 << 22
    rng = np.random.default_rng(22)
    keys = make_keys("uniform", n, rng)
    keys[::7] = keys[3]  # duplicates: stability has something to show
    iota = np.arange(n, dtype=np.uint32) if key_value else None
    offsets = np.array([0, n], np.uint32)
    gk, gv, _ = run_segmented(torch_mod, sorter, keys, offsets, iota)
    check(gk, gv, keys, iota, offsets)


@pytest.mark.parametrize("key_value", [False, True])
def test_bad_offsets_leave_their_segments_alone_and_say_so(torch_mod, sorter, key_value):
    """A decreasing pair and a last offset above maxElementCount: those segments are left alone, the valid ones sorted, the
    failure word and the sorter's word carry STATUS_SEGMENTS_INVALID.  The buffers reach 65536 words behind maxElementCount,
    so a missing bound check would change the guard band, never touch memory outside an allocation."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    assert sorter.read_sorter_status(stream) == 0
    n = 50000
    rng = np.random.default_rng(3)
    keys = make_keys("uniform", n, rng)
    iota = np.arange(n, dtype=np.uint32) if key_value else None
    # [100, 1100) small, [1100, 21100) large, [21100, 9000) decreasing, [9000, 9000) empty, [9000, n + 5000) beyond the bound
    offsets = np.array([100, 1100, 21100, 9000, 9000, n + 5000], np.uint32)
    gk, gv, _ = run_segmented(torch, sorter, keys, offsets, iota, guard=65536, expect_status=vrdx.STATUS_SEGMENTS_INVALID)
    ek, ev = expected(keys, iota, offsets, n)
    assert np.array_equal(gk, ek)
    assert np.array_equal(gk[21100:], keys[21100:]) and np.array_equal(gk[:100], keys[:100])
    if key_value:
        assert np.array_equal(gv, ev)
    assert sorter.read_sorter_status(stream) & vrdx.STATUS_SEGMENTS_INVALID
    assert sorter.read_sorter_status(stream) == 0  # (reading it cleared it)


def test_status_is_clear_and_the_plan_verdict_is_none(torch_mod, sorter):
    """Valid calls leave the failure word and the sorter's word at 0; a segmented sort behind an MSD sort on the same
    storage leaves VERDICT_NONE in word 1 (the MSD verdict does not survive into it)."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    assert sorter.read_sorter_status(stream) == 0
    big = 9_000_017
    assert sorter.describe_plan(big, False).name == "msd"
    rng = np.random.default_rng(9)
    storage = torch.empty(sorter.storage_requirements(big).size + 256, dtype=torch.uint8, device="cuda")
    dk = to_device(torch, make_keys("uniform", big, rng))
    sorter.cmd_sort(stream, big, dk.data_ptr(), 0, storage.data_ptr(), 0)
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_MSD_RUNS
    offsets, n = mixed_offsets(rng, [300, 5000, 20000, 0, 1])
    keys = make_keys("uniform", n, rng)
    gk, _, _ = run_segmented(torch, sorter, keys, offsets, storage=storage)
    check(gk, None, keys, None, offsets)
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_NONE
    assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    assert sorter.read_sorter_status(stream) == 0


def test_query_pool_slots(torch_mod, sorter):
    import vulkan_radix_sort_amd as vrdx
    rng = np.random.default_rng(15)
    offsets, n = mixed_offsets(rng, [100, 6000, 40000, 2])
    keys = make_keys("uniform", n, rng)
    pool = vrdx.QueryPool(15)
    gk, _, _ = run_segmented(torch_mod, sorter, keys, offsets, pool=pool)
    check(gk, None, keys, None, offsets)
    ts = pool.results_ns(0, 15)
    assert len(ts) == 15 and all(t >= 0 for t in ts) and ts[0] == 0
    assert ts[14] == max(ts) and ts[14] > 0
    pool.destroy()


def test_degenerate_calls_record_nothing(torch_mod, sorter):
    """segmentCount == 0 and maxElementCount == 0 touch nothing (every byte of the storage stays as it was)."""
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    keys = to_device(torch, np.arange(1000, 0, -1, dtype=np.uint32))
    offsets = to_device(torch, np.array([0, 1000], np.uint32))
    storage = torch.full((sorter.storage_requirements(1000).size,), 0xA5, dtype=torch.uint8, device="cuda")
    sorter.cmd_sort_segmented(stream, 1000, 0, offsets.data_ptr(), 0, keys.data_ptr(), 0, storage.data_ptr(), 0)
    sorter.cmd_sort_segmented(stream, 0, 1, offsets.data_ptr(), 0, keys.data_ptr(), 0, storage.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(keys), np.arange(1000, 0, -1, dtype=np.uint32))
    assert bool((storage == 0xA5).all())


def test_sort_segments_python_front_end(torch_mod, sorter):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    rng = np.random.default_rng(4)
    sizes = rng.integers(0, 3000, size=500)
    sizes[::50] = 20000
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    keys = make_keys("uniform", n, rng)
    iota = np.arange(n, dtype=np.uint32)
    dk, dv, do = to_device(torch, keys), to_device(torch, iota), to_device(torch, offsets)
    storage = vrdx.sort_segments(sorter, dk, do, values=dv)
    torch.cuda.synchronize()
    check(to_host(dk), to_host(dv), keys, iota, offsets)
    assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0


def test_sort_segments_accepts_views_off_a_sixteen_byte_boundary(torch_mod, sorter):
    """keys = big[1:1 + n] and values = other[3:3 + n]: contiguous views at 4 and 12 mod 16, which the front end hands on as
    they are.  Every size class, random values; big[0], other[:3] and the words behind both views keep their sentinel."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    rng = np.random.default_rng(14)
    sizes = rng.integers(0, 3000, size=200)
    sizes[::40] = [20001, 4097, 16384, 16385, 4096]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    keys = make_keys("uniform", n, rng)
    values = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    big = to_device(torch, np.concatenate([np.full(1, GUARD, np.uint32), keys, np.full(64, GUARD, np.uint32)]))
    other = to_device(torch, np.concatenate([np.full(3, GUARD, np.uint32), values, np.full(64, GUARD, np.uint32)]))
    dk, dv, do = big[1:1 + n], other[3:3 + n], to_device(torch, offsets)
    assert big.data_ptr() % 16 == 0 and dk.data_ptr() % 16 == 4 and dv.data_ptr() % 16 == 12
    assert dk.is_contiguous() and dv.is_contiguous()
    storage = vrdx.sort_segments(sorter, dk, do, values=dv)
    torch.cuda.synchronize()
    check(to_host(dk), to_host(dv), keys, values, offsets)
    whole, whole_values = to_host(big), to_host(other)
    assert whole[0] == GUARD and bool((whole[1 + n:] == GUARD).all())
    assert bool((whole_values[:3] == GUARD).all()) and bool((whole_values[3 + n:] == GUARD).all())
    assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0
    keys_only = to_device(torch, np.concatenate([np.full(1, GUARD, np.uint32), keys, np.full(64, GUARD, np.uint32)]))
    vrdx.sort_segments(sorter, keys_only[1:1 + n], do)
    torch.cuda.synchronize()
    whole = to_host(keys_only)
    check(whole[1:1 + n], None, keys, None, offsets)
    assert whole[0] == GUARD and bool((whole[1 + n:] == GUARD).all())


def test_captured_graph_replays_on_new_keys_and_a_new_segmentation(torch_mod, sorter):
    """One call captured in torch.cuda.graph (a linear graph) sorts whatever keys AND whatever offsets it is replayed on, as
    long as segmentCount stays: the size classes are decided on the device at every replay."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    rng = np.random.default_rng(77)
    n = 400_000
    segmentations = [[300] * 60 + [5000] * 20 + [40000] * 4 + [0] * 16,
                     [20000] * 15 + [17] * 60 + [9000] * 5 + [3] * 20]
    offsets_list = []
    for sizes in segmentations:
        sizes = list(sizes)
        rng.shuffle(sizes)
        offsets_list.append(np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32))
    assert len({len(o) for o in offsets_list}) == 1 and all(o[-1] <= n for o in offsets_list)
    dk, dv, do = to_device(torch, np.zeros(n, np.uint32)), to_device(torch, np.zeros(n, np.uint32)), to_device(torch, offsets_list[0])
    storage = torch.empty(sorter.key_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
    vrdx.sort_segments(sorter, dk, do, values=dv, storage=storage)  # one eager call first (test_sort_gpu.py explains why)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vrdx.sort_segments(sorter, dk, do, values=dv, storage=storage)
    iota = np.arange(n, dtype=np.uint32)
    for replay, offsets in enumerate(offsets_list + offsets_list[::-1]):
        keys = make_keys("uniform" if replay % 2 == 0 else "24-bit", n, rng)
        dk.copy_(to_device(torch, keys))
        dv.copy_(to_device(torch, iota))
        do.copy_(to_device(torch, offsets))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(to_host(dk), to_host(dv), keys, iota, offsets)
        assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0


SINGLE_HEADER_CASE = r"""
#define VRDX_IMPLEMENTATION
#include "vk_radix_sort.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>

int main() {
  VrdxSorterCreateInfo info = {};
  VrdxSorter sorter = nullptr;
  if (vrdxCreateSorter(&info, &sorter) != VK_SUCCESS) { std::printf("no sorter\n"); return 2; }
  const std::vector<uint32_t> sizes = {7, 40000, 0, 4096, 1, 9000, 16384, 300, 16385, 2};
  std::vector<uint32_t> offsets = {5};
  for (uint32_t s : sizes) offsets.push_back(offsets.back() + s);
  const uint32_t n = offsets.back() + 11;
  std::vector<uint32_t> keys(n), values(n);
  uint32_t x = 12345;
  for (uint32_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; keys[i] = (x >> 8) & 0xFFFFu; values[i] = i; }
  VrdxSorterStorageRequirements req;
  vrdxGetSorterKeyValueStorageRequirements(sorter, n, &req);
  uint32_t *dk, *dv, *doff; uint8_t* st;
  if (hipMalloc(&dk, 4 * n) != hipSuccess || hipMalloc(&dv, 4 * n) != hipSuccess ||
      hipMalloc(&doff, 4 * offsets.size()) != hipSuccess || hipMalloc(&st, req.size) != hipSuccess) return 3;
  (void)hipMemcpy(dk, keys.data(), 4 * n, hipMemcpyHostToDevice);
  (void)hipMemcpy(dv, values.data(), 4 * n, hipMemcpyHostToDevice);
  (void)hipMemcpy(doff, offsets.data(), 4 * offsets.size(), hipMemcpyHostToDevice);
  vrdxHipCmdSortSegmentedKeyValue(nullptr, sorter, n, (uint32_t)sizes.size(), (VkBuffer)doff, 0, (VkBuffer)dk, 0, (VkBuffer)dv, 0,
                                  (VkBuffer)st, 0, nullptr, 0);
  std::vector<uint32_t> gk(n), gv(n);
  (void)hipMemcpy(gk.data(), dk, 4 * n, hipMemcpyDeviceToHost);
  (void)hipMemcpy(gv.data(), dv, 4 * n, hipMemcpyDeviceToHost);
  const uint32_t status = vrdxHipReadSorterStatus(sorter, nullptr);
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  for (size_t s = 0; s < sizes.size(); ++s)
    std::stable_sort(idx.begin() + offsets[s], idx.begin() + offsets[s + 1], [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  size_t bad = 0;
  for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[idx[i]] || gv[i] != values[idx[i]];
  std::printf("status %u, %zu mismatches\n", status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
"""


def test_single_header_segmented_parity(tmp_path):
    """The segmented entry point through the single header's own launcher (vrdx_module_launch.inc: the kernels resolved by
    mangled name, with the LDS sizes of the launch layer it shares with the library), compiled with plain g++: every size
    class in one key+value call."""
    header = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
    if not os.path.exists(header):
        subprocess.run(["python3", os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", header], check=True)
    src = tmp_path / "segmented_single_header.cc"
    src.write_text(SINGLE_HEADER_CASE)
    exe = tmp_path / "segmented_single_header"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.dirname(header), str(src), "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "status 0, 0 mismatches" in r.stdout, r.stdout + r.stderr
