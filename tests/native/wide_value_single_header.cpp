// The sorts of 32-bit keys with 64-bit values through the SINGLE-HEADER distribution (tools/generate_single_header.py): this
// translation unit defines VRDX_IMPLEMENTATION, so it holds the host recorder and the embedded gfx950 code object, and the new
// kernels are resolved by mangled name (vrdx_module_launch.inc).  Compiled by tests/test_wide_value_single_header_gpu.py with
// plain g++ against libamdhip64 only.  Sorts 4095 (the 256-thread kernel), 8192 (the 1024-thread kernel), 20001 (the gather form)
// elements, directly and by a device-side count of n - 5, and twoSortsFrom + 3 elements (the two-sorts form) by a count of n - 5,
// against a stable reference computed here.
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
  VrdxHipWideValuePlanInfo plan;
  vrdxHipDescribeWideValueSortPlan(sorter, 1, &plan);
  size_t bad = 0, cases = 0;
  uint32_t status = 0, forms = 0;
  for (uint32_t n : {4095u, 8192u, 20001u, plan.twoSortsFrom + 3u}) {
    vrdxHipDescribeWideValueSortPlan(sorter, n, &plan);
    forms |= 1u << plan.form;
    std::vector<uint32_t> keys(n), index(n);
    std::vector<uint64_t> values(n);
    uint32_t x = 12345u + n;
    for (uint32_t i = 0; i < n; ++i) {
      x = x * 1664525u + 1013904223u;
      keys[i] = (x ^ (x >> 15)) & 0xFFF00FFFu;  // ties, and one byte that needs no full pass
      values[i] = ((uint64_t)(x * 2654435761u) << 32) | (uint32_t)~i;
    }
    VrdxSorterStorageRequirements req;
    vrdxHipGetSorterWideValueStorageRequirements(sorter, n, &req);
    uint32_t *dk = nullptr, *dc = nullptr;
    uint64_t* dv = nullptr;
    uint8_t* storage = nullptr;
    if (hipMalloc(&dk, 4 * (size_t)n) != hipSuccess || hipMalloc(&dv, 8 * (size_t)n) != hipSuccess || hipMalloc(&dc, 4) != hipSuccess ||
        hipMalloc(&storage, req.size) != hipSuccess)
      return 3;
    // (the two-sorts form, whose first size is large: by a device-side count only)
    for (int indirect = plan.form == VRDX_HIP_WIDE_VALUE_TWO_SORTS ? 1 : 0; indirect < 2; ++indirect) {
      const uint32_t count = indirect ? n - 5u : n;
      std::iota(index.begin(), index.end(), 0u);
      std::stable_sort(index.begin(), index.begin() + count, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
      (void)hipMemcpy(dk, keys.data(), 4 * (size_t)n, hipMemcpyHostToDevice);
      (void)hipMemcpy(dv, values.data(), 8 * (size_t)n, hipMemcpyHostToDevice);
      (void)hipMemcpy(dc, &count, 4, hipMemcpyHostToDevice);
      if (indirect)
        vrdxHipCmdWideValueSortIndirect(nullptr, sorter, n, (VkBuffer)dc, 0, (VkBuffer)dk, 0, (VkBuffer)dv, 0, (VkBuffer)storage, 0, nullptr, 0);
      else
        vrdxHipCmdWideValueSort(nullptr, sorter, n, (VkBuffer)dk, 0, (VkBuffer)dv, 0, (VkBuffer)storage, 0, nullptr, 0);
      std::vector<uint32_t> gk(n);
      std::vector<uint64_t> gv(n);
      (void)hipMemcpy(gk.data(), dk, 4 * (size_t)n, hipMemcpyDeviceToHost);
      (void)hipMemcpy(gv.data(), dv, 8 * (size_t)n, hipMemcpyDeviceToHost);
      status |= vrdxHipReadStatus(nullptr, (VkBuffer)storage, 0);
      for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[index[i]] || gv[i] != values[index[i]];
      ++cases;
    }
    (void)hipFree(dk);
    (void)hipFree(dv);
    (void)hipFree(dc);
    (void)hipFree(storage);
  }
  status |= vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("%zu cases, forms 0x%x, status %u, %zu mismatches\n", cases, forms, status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
