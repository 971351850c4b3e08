// CPU-only check of the plan and the layout of the segmented sort of 32-bit keys with 64-bit values (vrdx_plan.h:
// PlanWideValueSortSegmented; vrdx_layout.h: MakeSegmentedWideLayout), compiled and run by
// tests/test_wide_value_segmented_plan.py.  At 8 and 256 CUs, both rankings, for N in 1, 2, 4096, 4097, 8192, 8193, 16385,
// 100000, 2^20, 2^24 + 1, 2^30 - 4, segment counts 1, 2, CUs - 1, CUs, CUs + 1, 2 CUs + 1, 2^20, 2^20 + 1 and every storage
// address mod 128 that a caller may hand over (multiples of 16):
//   the steps    which exist (a launch whose grid would be 0 is absent), their kinds, names, slots 1 ... 4 and grids: fill 1,
//                small min(segments, 2^20), mid and large min(segments, list cap, CUs);
//   the caps     N / 4097 and N / 8193;
//   the layout   counters and lists inside the inner key+value storage, in order, not overlapping; keysScratch on a 128-byte
//                line behind the inner storage, ending before valuesScratch; valuesScratch on a 128-byte line, ending inside
//                MakeWideValueLayout(N).size, which does not depend on the address; fits;
//   nothing      segmentCount == 0 and N == 0 give no step and no refusal.
// Nothing of HIP is linked.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../vulkan_radix_sort_amd/csrc/vrdx_plan.h"

namespace {

int failures = 0;
long cases = 0;
void Check(bool ok, const char* what, uint32_t n, uint32_t segments, int cus, int atomic, uint64_t address) {
  ++cases;
  if (ok) return;
  if (failures < 20)
    std::printf("FAIL %s: n=%u segments=%u cus=%d atomic=%d address=%llu\n", what, n, segments, cus, atomic, (unsigned long long)address);
  ++failures;
}

}  // namespace

int main() {
  using vrdx::SegmentedStep;
  static_assert(vrdx::kSegWideSmallMax == 4096u && vrdx::kSegWideMidMax == 8192u && vrdx::kSegWideLargeTile == 8192u, "class bounds");
  static_assert(vrdx::SegmentWideLargeLdsWords() * 4 == 121024u, "the large kernel's LDS: 118.2 KiB");
  static_assert(vrdx::SortInWorkgroup64LdsWords(256, 16, true) * 4 == 53312u && vrdx::SortInWorkgroup64LdsWords(1024, 8, true) * 4 == 114752u,
                "the in-LDS kernels' LDS: 52 and 112 KiB");
  const uint32_t sizes[] = {1u, 2u, 4096u, 4097u, 8192u, 8193u, 16385u, 100000u, 1u << 20, (1u << 24) + 1u, VRDX_MAX_ELEMENTS};
  const char* const names[4] = {"segmented_clear_kernel", "segmented_small_wide_kernel", "segmented_mid_wide_kernel",
                                "segmented_large_wide_kernel"};
  for (int cus : {8, 256})
    for (int atomic = 0; atomic < 2; ++atomic) {
      vrdx::PlanContext c;
      c.computeUnits = cus;
      c.atomicRank = atomic != 0;
      const uint32_t align = c.minStorageBufferOffsetAlignment;
      const uint32_t u = (uint32_t)cus;
      const uint32_t counts[] = {1u, 2u, u - 1u, u, u + 1u, 2u * u + 1u, 1u << 20, (1u << 20) + 1u};
      for (uint32_t n : sizes) {
        const vrdx::WideValueLayout w = vrdx::MakeWideValueLayout(n, align);
        const uint64_t inner = vrdx::MakeLayout(n, align, 0).keyValueSize;
        for (uint32_t segments : counts)
          for (uint64_t address = 0x7000000000ull; address < 0x7000000000ull + 128; address += 16) {
            const vrdx::WideValueSegmentedPlan p = vrdx::PlanWideValueSortSegmented(c, n, segments, address);
            const auto check = [&](bool ok, const char* what) { Check(ok, what, n, segments, cus, atomic, address & 127u); };
            check(p.refusal == nullptr && p.atomicRank == (atomic != 0), "no refusal, the ranking");
            // the caps and the grids
            const vrdx::SegmentedLayout& l = p.layout;
            check(l.midCap == n / 4097u && l.largeCap == n / 8193u, "list caps");
            const uint32_t grids[4] = {1u, std::min(segments, 1u << 20), std::min(std::min(segments, n / 4097u), u),
                                       std::min(std::min(segments, n / 8193u), u)};
            uint32_t at = 0;
            bool ok = true;
            for (uint32_t i = 0; i < 4; ++i) {
              if (grids[i] == 0) continue;
              ok = ok && at < p.stepCount && p.steps[at].what == SegmentedStep(i) && p.steps[at].slot == i + 1 &&
                   p.steps[at].grid == grids[i] && std::strcmp(p.steps[at].name, names[i]) == 0;
              ++at;
            }
            check(ok && at == p.stepCount, "steps, slots and grids");
            check(p.stepCount == 2u + (n >= 4097u) + (n >= 8193u), "which steps exist");
            // the layout
            const uint64_t bytes = 4ull * n;
            check(l.fits, "fits");
            check(vrdx::MakeWideValueLayout(n, align, address).size == w.size && w.innerSize == inner, "the requirement does not depend on the address");
            check(l.midCountOffset >= 16 && l.largeCountOffset >= l.midCountOffset + 128 && l.largeCountOffset + 4 <= l.midListOffset &&
                      l.midListOffset + 4ull * l.midCap <= l.largeListOffset && l.largeListOffset + 4ull * l.largeCap <= inner,
                  "counters and lists in order inside the inner storage");
            check((address + l.midListOffset) % 4 == 0 && (address + l.midCountOffset) % 4 == 0, "word alignment");
            check(l.keysScratchOffset >= inner && (address + l.keysScratchOffset) % 128 == 0 &&
                      l.keysScratchOffset + bytes <= l.valuesScratchOffset,
                  "keysScratch behind the inner storage, ending before valuesScratch");
            check((address + l.valuesScratchOffset) % 128 == 0 && l.valuesScratchOffset + 2 * bytes <= w.size,
                  "valuesScratch on a 128-byte line, ending inside the requirement");
          }
      }
      // nothing to do
      for (uint64_t address = 0x7000000000ull; address < 0x7000000000ull + 128; address += 16) {
        const vrdx::WideValueSegmentedPlan none = vrdx::PlanWideValueSortSegmented(c, 100000u, 0u, address);
        Check(none.stepCount == 0 && none.refusal == nullptr, "no segments", 100000u, 0u, cus, atomic, address & 127u);
        const vrdx::WideValueSegmentedPlan empty = vrdx::PlanWideValueSortSegmented(c, 0u, 5u, address);
        Check(empty.stepCount == 0 && empty.refusal == nullptr, "no elements", 0u, 5u, cus, atomic, address & 127u);
      }
    }
  std::printf("wide value segmented plan: %ld cases, %d failures\n", cases, failures);
  return failures == 0 ? 0 : 1;
}
