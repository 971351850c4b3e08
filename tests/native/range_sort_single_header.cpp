// The range sorts at every size through the SINGLE-HEADER distribution (tools/generate_single_header.py): this translation
// unit defines VRDX_IMPLEMENTATION, so it holds the host recorder and the embedded gfx950 code object, and the count, scan,
// scatter and copy-back kernels are resolved by mangled name (vrdx_module_launch.inc).  Compiled by
// tests/test_range_sort_single_header_gpu.py with plain g++ against libamdhip64 only.  Sorts 65539 elements by the ranges
// [5, 14) and [4, 28), keys-only and key+value, direct and by a device-side count, against a stable reference computed here.
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
  size_t bad = 0, cases = 0;
  uint32_t status = 0;
  const uint32_t n = 65539u;
  VrdxHipRangeSortPlanInfo plan = {};
  vrdxHipDescribeRangeSortPlan(sorter, n, 1, 5, 14, &plan);
  if (plan.form != VRDX_HIP_RANGE_SORT_CHUNKED || plan.launches != 7) {
    std::printf("plan: form %u, %u launches\n", plan.form, plan.launches);
    return 4;
  }
  for (uint32_t range : {0u, 1u}) {
    const uint32_t begin = range == 0 ? 5 : 4, end = range == 0 ? 14 : 28;
    std::vector<uint32_t> keys(n), values(n);
    uint32_t x = 12345u + n + begin;
    for (uint32_t i = 0; i < n; ++i) {
      x = x * 1664525u + 1013904223u;
      keys[i] = x ^ (x >> 15);  // every bit random: the bits outside the range tell equal fields apart
      values[i] = i * 2654435761u;
    }
    const auto field = [&](uint32_t k) { return (k >> begin) & ((1u << (end - begin)) - 1u); };
    VrdxSorterStorageRequirements req;
    vrdxGetSorterKeyValueStorageRequirements(sorter, n, &req);
    uint32_t *dk = nullptr, *dv = nullptr, *dcount = nullptr;
    uint8_t* storage = nullptr;
    if (hipMalloc(&dk, 4 * n) != hipSuccess || hipMalloc(&dv, 4 * n) != hipSuccess || hipMalloc(&dcount, 4) != hipSuccess ||
        hipMalloc(&storage, req.size) != hipSuccess)
      return 3;
    for (int indirect = 0; indirect < 2; ++indirect) {
      const uint32_t count = indirect ? 40001u : n;  // (the indirect calls: part of the array, the rest left alone)
      std::vector<uint32_t> index(count);
      std::iota(index.begin(), index.end(), 0u);
      std::stable_sort(index.begin(), index.end(), [&](uint32_t a, uint32_t b) { return field(keys[a]) < field(keys[b]); });
      for (int keyValue = 0; keyValue < 2; ++keyValue) {
        (void)hipMemcpy(dk, keys.data(), 4 * n, hipMemcpyHostToDevice);
        (void)hipMemcpy(dv, values.data(), 4 * n, hipMemcpyHostToDevice);
        (void)hipMemcpy(dcount, &count, 4, hipMemcpyHostToDevice);
        if (indirect && keyValue)
          vrdxHipCmdRangeSortKeyValueIndirect(nullptr, sorter, n, (VkBuffer)dcount, 0, (VkBuffer)dk, 0, (VkBuffer)dv, 0, begin, end,
                                              (VkBuffer)storage, 0, nullptr, 0);
        else if (indirect)
          vrdxHipCmdRangeSortIndirect(nullptr, sorter, n, (VkBuffer)dcount, 0, (VkBuffer)dk, 0, begin, end, (VkBuffer)storage, 0,
                                      nullptr, 0);
        else if (keyValue)
          vrdxHipCmdRangeSortKeyValue(nullptr, sorter, n, (VkBuffer)dk, 0, (VkBuffer)dv, 0, begin, end, (VkBuffer)storage, 0, nullptr, 0);
        else
          vrdxHipCmdRangeSort(nullptr, sorter, n, (VkBuffer)dk, 0, begin, end, (VkBuffer)storage, 0, nullptr, 0);
        std::vector<uint32_t> gk(n), gv(n);
        (void)hipMemcpy(gk.data(), dk, 4 * n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(gv.data(), dv, 4 * n, hipMemcpyDeviceToHost);
        status |= vrdxHipReadStatus(nullptr, (VkBuffer)storage, 0);
        for (uint32_t i = 0; i < n; ++i) {
          const uint32_t from = i < count ? index[i] : i;
          bad += gk[i] != keys[from] || gv[i] != (keyValue ? values[from] : values[i]);
        }
        ++cases;
      }
    }
    (void)hipFree(dk);
    (void)hipFree(dv);
    (void)hipFree(dcount);
    (void)hipFree(storage);
  }
  status |= vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("%zu cases, status %u, %zu mismatches\n", cases, status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
