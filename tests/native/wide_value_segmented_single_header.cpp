// The segmented sort of 32-bit keys with 64-bit values through the SINGLE-HEADER distribution
// (tools/generate_single_header.py): this translation unit defines VRDX_IMPLEMENTATION, so it holds the host recorder and the
// embedded gfx950 code object, and the new kernels are resolved by mangled name (vrdx_module_launch.inc).  Compiled by
// tests/test_wide_value_segmented_single_header_gpu.py with plain g++ against libamdhip64 only.  One call whose segments
// cover all three classes (0, 1, 2, 300, 4096, 4097, 8192, 8193 and 20001 elements, three elements in front of the first and
// five behind the last that no segment covers), and one of 3000 segments of 0 to 6 elements, against a stable reference
// computed here.
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
  for (int which = 0; which < 2; ++which) {
    std::vector<uint32_t> offsets{3u};
    if (which == 0) {
      for (uint32_t size : {0u, 1u, 2u, 300u, 4096u, 4097u, 8192u, 8193u, 20001u}) offsets.push_back(offsets.back() + size);
    } else {
      for (uint32_t i = 0; i < 3000u; ++i) offsets.push_back(offsets.back() + (i * 2654435761u >> 16) % 7u);
    }
    const uint32_t segments = (uint32_t)offsets.size() - 1u;
    const uint32_t n = offsets.back() + 5u;
    std::vector<uint32_t> keys(n), index(n);
    std::vector<uint64_t> values(n);
    uint32_t x = 12345u + n;
    for (uint32_t i = 0; i < n; ++i) {
      x = x * 1664525u + 1013904223u;
      keys[i] = (x ^ (x >> 15)) & 0xFFF00FFFu;  // ties, and one byte that needs no full pass
      values[i] = ((uint64_t)(x * 2654435761u) << 32) | (uint32_t)~i;
    }
    std::iota(index.begin(), index.end(), 0u);
    for (uint32_t s = 0; s < segments; ++s)
      std::stable_sort(index.begin() + offsets[s], index.begin() + offsets[s + 1], [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    VrdxSorterStorageRequirements req;
    vrdxHipGetSorterWideValueStorageRequirements(sorter, n, &req);
    uint32_t *dk = nullptr, *offs = nullptr;
    uint64_t* dv = nullptr;
    uint8_t* storage = nullptr;
    if (hipMalloc(&dk, 4 * (size_t)n) != hipSuccess || hipMalloc(&dv, 8 * (size_t)n) != hipSuccess ||
        hipMalloc(&offs, 4 * offsets.size()) != hipSuccess || hipMalloc(&storage, req.size) != hipSuccess)
      return 3;
    (void)hipMemcpy(dk, keys.data(), 4 * (size_t)n, hipMemcpyHostToDevice);
    (void)hipMemcpy(dv, values.data(), 8 * (size_t)n, hipMemcpyHostToDevice);
    (void)hipMemcpy(offs, offsets.data(), 4 * offsets.size(), hipMemcpyHostToDevice);
    vrdxHipCmdWideValueSortSegmented(nullptr, sorter, n, segments, (VkBuffer)offs, 0, (VkBuffer)dk, 0, (VkBuffer)dv, 0,
                                     (VkBuffer)storage, 0, nullptr, 0);
    std::vector<uint32_t> gk(n);
    std::vector<uint64_t> gv(n);
    (void)hipMemcpy(gk.data(), dk, 4 * (size_t)n, hipMemcpyDeviceToHost);
    (void)hipMemcpy(gv.data(), dv, 8 * (size_t)n, hipMemcpyDeviceToHost);
    status |= vrdxHipReadStatus(nullptr, (VkBuffer)storage, 0);
    for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[index[i]] || gv[i] != values[index[i]];
    ++cases;
    (void)hipFree(dk);
    (void)hipFree(dv);
    (void)hipFree(offs);
    (void)hipFree(storage);
  }
  status |= vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("%zu cases, status %u, %zu mismatches\n", cases, status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
