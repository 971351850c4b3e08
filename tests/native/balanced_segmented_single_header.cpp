// The balanced segmented sort through the SINGLE-HEADER distribution (tools/generate_single_header.py): this translation
// unit defines VRDX_IMPLEMENTATION, so it holds the host recorder and the embedded gfx950 code object, and the split, count,
// scan, scatter and copy-back kernels are resolved by mangled name (vrdx_module_launch.inc).  Compiled by
// tests/test_balanced_segmented_single_header_gpu.py with plain g++ against libamdhip64 only.  Sorts 300007 elements in six
// segments -- two of them spread, one large, one mid, two small -- keys-only and key+value, against a stable reference computed
// here, and reads the split words back.
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
  if (vrdxCreateSorter(&info, &sorter) != VK_SUCCESS) {
    std::printf("no sorter\n");
    return 2;
  }
  const uint32_t n = 300007u;
  const std::vector<uint32_t> offsets = {3u, 100003u, 100010u, 105010u, 135010u, 135011u, 300000u};
  const uint32_t segments = (uint32_t)offsets.size() - 1u;
  VrdxHipBalancedSegmentedPlanInfo plan = {};
  vrdxHipDescribeBalancedSegmentedPlan(sorter, n, segments, 1, &plan);
  if (plan.form != VRDX_HIP_BALANCED_BALANCED || plan.launches != 18 || plan.spreadCap == 0 || plan.pieceCap <= plan.spreadCap) {
    std::printf("plan: form %u, %u launches, caps %u %u\n", plan.form, plan.launches, plan.spreadCap, plan.pieceCap);
    return 4;
  }
  std::vector<uint32_t> keys(n), values(n);
  uint32_t x = 12345u + n;
  for (uint32_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    keys[i] = (x ^ (x >> 15)) & 0x00FFFFFFu;  // (three active bytes: a copy back)
    x = x * 1664525u + 1013904223u;
    values[i] = x;
  }
  std::vector<uint32_t> index(n);
  std::iota(index.begin(), index.end(), 0u);
  for (uint32_t s = 0; s < segments; ++s)
    std::stable_sort(index.begin() + offsets[s], index.begin() + offsets[s + 1], [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  VrdxSorterStorageRequirements req;
  vrdxGetSorterKeyValueStorageRequirements(sorter, n, &req);
  uint32_t *dk = nullptr, *dv = nullptr, *doffsets = nullptr;
  uint8_t* storage = nullptr;
  if (hipMalloc(&dk, 4 * n) != hipSuccess || hipMalloc(&dv, 4 * n) != hipSuccess ||
      hipMalloc(&doffsets, 4 * offsets.size()) != hipSuccess || hipMalloc(&storage, req.size) != hipSuccess)
    return 3;
  (void)hipMemcpy(doffsets, offsets.data(), 4 * offsets.size(), hipMemcpyHostToDevice);
  size_t bad = 0, cases = 0;
  uint32_t status = 0, spread = 0;
  for (int keyValue = 0; keyValue < 2; ++keyValue) {
    (void)hipMemcpy(dk, keys.data(), 4 * n, hipMemcpyHostToDevice);
    (void)hipMemcpy(dv, values.data(), 4 * n, hipMemcpyHostToDevice);
    if (keyValue)
      vrdxHipCmdBalancedSortSegmentedKeyValue(nullptr, sorter, n, segments, (VkBuffer)doffsets, 0, (VkBuffer)dk, 0, (VkBuffer)dv, 0,
                                              (VkBuffer)storage, 0, nullptr, 0);
    else
      vrdxHipCmdBalancedSortSegmented(nullptr, sorter, n, segments, (VkBuffer)doffsets, 0, (VkBuffer)dk, 0, (VkBuffer)storage, 0,
                                      nullptr, 0);
    std::vector<uint32_t> gk(n), gv(n);
    (void)hipMemcpy(gk.data(), dk, 4 * n, hipMemcpyDeviceToHost);
    (void)hipMemcpy(gv.data(), dv, 4 * n, hipMemcpyDeviceToHost);
    status |= vrdxHipReadStatus(nullptr, (VkBuffer)storage, 0);
    VrdxHipBalancedSplitInfo split = {};
    if (vrdxHipReadBalancedSplit(nullptr, sorter, (VkBuffer)storage, 0, n, &split) != VK_SUCCESS) ++bad;
    // listed: 100000, 30000 and 164989 elements; spread where the chip has 16 compute units and more
    bad += split.listedSegments != 3u || split.pieceKeys != 16384u || split.pieces < split.spreadSegments;
    spread += split.spreadSegments;
    for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[index[i]] || gv[i] != (keyValue ? values[index[i]] : values[i]);
    ++cases;
  }
  (void)hipFree(dk);
  (void)hipFree(dv);
  (void)hipFree(doffsets);
  (void)hipFree(storage);
  status |= vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("%zu cases, status %u, %zu mismatches, %u spread\n", cases, status, bad, spread);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
