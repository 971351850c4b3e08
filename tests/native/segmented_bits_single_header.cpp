// The segmented sort by a bit range through the SINGLE-HEADER distribution (tools/generate_single_header.py): this translation
// unit defines VRDX_IMPLEMENTATION, so it holds the host recorder and the embedded gfx950 code object, and the range forms of the
// three segmented kernels are resolved by mangled name (vrdx_module_launch.inc).  Compiled by
// tests/test_segmented_bits_single_header_gpu.py with plain g++ against libamdhip64 only.  One call with segments of every size
// class sorted by the range [3, 12), keys-only and key+value, against a stable reference computed here.
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
  const uint32_t begin = 3, end = 12;
  const std::vector<uint32_t> sizes = {7, 40000, 0, 4096, 1, 9000, 16384, 300, 16385, 2};
  std::vector<uint32_t> offsets = {5};
  for (uint32_t s : sizes) offsets.push_back(offsets.back() + s);
  const uint32_t n = offsets.back() + 11;
  std::vector<uint32_t> keys(n), values(n), index(n);
  uint32_t x = 12345u;
  for (uint32_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    keys[i] = x ^ (x >> 15);  // every bit random: the bits outside the range tell equal fields apart
    values[i] = i * 2654435761u;
  }
  const auto field = [&](uint32_t k) { return (k >> begin) & ((1u << (end - begin)) - 1u); };
  std::iota(index.begin(), index.end(), 0u);
  for (size_t s = 0; s < sizes.size(); ++s)
    std::stable_sort(index.begin() + offsets[s], index.begin() + offsets[s + 1],
                     [&](uint32_t a, uint32_t b) { return field(keys[a]) < field(keys[b]); });
  VrdxSorterStorageRequirements req;
  vrdxGetSorterKeyValueStorageRequirements(sorter, n, &req);
  uint32_t *dk = nullptr, *dv = nullptr, *doff = nullptr;
  uint8_t* storage = nullptr;
  if (hipMalloc(&dk, 4 * n) != hipSuccess || hipMalloc(&dv, 4 * n) != hipSuccess ||
      hipMalloc(&doff, 4 * offsets.size()) != hipSuccess || hipMalloc(&storage, req.size) != hipSuccess)
    return 3;
  (void)hipMemcpy(doff, offsets.data(), 4 * offsets.size(), hipMemcpyHostToDevice);
  size_t bad = 0, cases = 0;
  uint32_t status = 0;
  for (int keyValue = 0; keyValue < 2; ++keyValue) {
    (void)hipMemcpy(dk, keys.data(), 4 * n, hipMemcpyHostToDevice);
    (void)hipMemcpy(dv, values.data(), 4 * n, hipMemcpyHostToDevice);
    if (keyValue)
      vrdxHipCmdSortSegmentedBitsKeyValue(nullptr, sorter, n, (uint32_t)sizes.size(), (VkBuffer)doff, 0, (VkBuffer)dk, 0,
                                          (VkBuffer)dv, 0, begin, end, (VkBuffer)storage, 0, nullptr, 0);
    else
      vrdxHipCmdSortSegmentedBits(nullptr, sorter, n, (uint32_t)sizes.size(), (VkBuffer)doff, 0, (VkBuffer)dk, 0, begin, end,
                                  (VkBuffer)storage, 0, nullptr, 0);
    std::vector<uint32_t> gk(n), gv(n);
    (void)hipMemcpy(gk.data(), dk, 4 * n, hipMemcpyDeviceToHost);
    (void)hipMemcpy(gv.data(), dv, 4 * n, hipMemcpyDeviceToHost);
    status |= vrdxHipReadStatus(nullptr, (VkBuffer)storage, 0);
    for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[index[i]] || gv[i] != (keyValue ? values[index[i]] : values[i]);
    ++cases;
  }
  status |= vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("%zu cases, status %u, %zu mismatches\n", cases, status, bad);
  (void)hipFree(dk);
  (void)hipFree(dv);
  (void)hipFree(doff);
  (void)hipFree(storage);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
