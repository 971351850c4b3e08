// The bit-range sorts through the SINGLE-HEADER distribution (tools/generate_single_header.py): this translation unit defines
// VRDX_IMPLEMENTATION, so it holds the host recorder and the embedded gfx950 code object, and the range kernels are resolved
// by mangled name (vrdx_module_launch.inc).  Compiled by tests/test_sort_bits_single_header_gpu.py with plain g++ against
// libamdhip64 only.  Sorts by the ranges [3, 12) and [7, 24) at 4095 (the 256-thread kernel) and 16384 (the 1024-thread kernel) elements,
// keys-only and key+value, against a stable reference computed here.
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
  for (uint32_t n : {4095u, 16384u})
    for (uint32_t range : {0u, 1u}) {
      const uint32_t begin = range == 0 ? 3 : 7, end = range == 0 ? 12 : 24;
      std::vector<uint32_t> keys(n), values(n), index(n);
      uint32_t x = 12345u + n + begin;
      for (uint32_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        keys[i] = x ^ (x >> 15);  // every bit random: the bits outside the range tell equal fields apart
        values[i] = i * 2654435761u;
      }
      const auto field = [&](uint32_t k) { return (k >> begin) & ((1u << (end - begin)) - 1u); };
      std::iota(index.begin(), index.end(), 0u);
      std::stable_sort(index.begin(), index.end(), [&](uint32_t a, uint32_t b) { return field(keys[a]) < field(keys[b]); });
      VrdxSorterStorageRequirements req;
      vrdxGetSorterKeyValueStorageRequirements(sorter, n, &req);
      uint32_t *dk = nullptr, *dv = nullptr;
      uint8_t* storage = nullptr;
      if (hipMalloc(&dk, 4 * n) != hipSuccess || hipMalloc(&dv, 4 * n) != hipSuccess || hipMalloc(&storage, req.size) != hipSuccess) return 3;
      for (int keyValue = 0; keyValue < 2; ++keyValue) {
        (void)hipMemcpy(dk, keys.data(), 4 * n, hipMemcpyHostToDevice);
        (void)hipMemcpy(dv, values.data(), 4 * n, hipMemcpyHostToDevice);
        if (keyValue)
          vrdxHipCmdSortBitsKeyValue(nullptr, sorter, n, (VkBuffer)dk, 0, (VkBuffer)dv, 0, begin, end, (VkBuffer)storage, 0, nullptr, 0);
        else
          vrdxHipCmdSortBits(nullptr, sorter, n, (VkBuffer)dk, 0, begin, end, (VkBuffer)storage, 0, nullptr, 0);
        std::vector<uint32_t> gk(n), gv(n);
        (void)hipMemcpy(gk.data(), dk, 4 * n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(gv.data(), dv, 4 * n, hipMemcpyDeviceToHost);
        status |= vrdxHipReadStatus(nullptr, (VkBuffer)storage, 0);
        for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[index[i]] || gv[i] != (keyValue ? values[index[i]] : values[i]);
        ++cases;
      }
      (void)hipFree(dk);
      (void)hipFree(dv);
      (void)hipFree(storage);
    }
  status |= vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("%zu cases, status %u, %zu mismatches\n", cases, status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
