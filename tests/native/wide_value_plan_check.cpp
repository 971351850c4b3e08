// CPU-only check of the plan and the storage of the sorts of 32-bit keys with 64-bit values (vrdx_plan.h: PlanWideValueSort;
// vrdx_layout.h: MakeWideValueLayout), compiled and run by tests/test_wide_value_plan.py.  At 8 and 256 CUs, both rankings,
// smallSort on and off, for n in 0, 1, 8191, 8192, 8193, kWideValueTwoSortsFrom - 1, kWideValueTwoSortsFrom,
// kWideValueTwoSortsFrom + 1, 2^30 - 4 (the clamp: a recorder never plans more) and what 2^30 - 3 and 2^32 - 1 are clamped
// to, and for every storage address mod 128 that
// a caller may hand over (multiples of 16):
//   the form       none | one workgroup (n <= 8192 and smallSort) | gather | two sorts (from the constant);
//   the steps      their kinds, names and slots: one step at slot 14, or four at slots 1-4;
//   the layout     A, B, C on 128-byte lines of the absolute address, in this order, not overlapping each other or the inner
//                  storage, T = B with 8 n bytes ending inside C, everything inside the requirement; the requirement is the
//                  key+value requirement + 12 n + the fixed pad, whatever the address;
//   the description form, launches and bytes per element as DescribeWideValuePlan puts them together from the inner plan.
// Nothing of HIP is linked.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../vulkan_radix_sort_amd/csrc/vrdx_plan.h"

namespace {

int failures = 0;
long cases = 0;
void Check(bool ok, const char* what, uint32_t n, int cus, int atomic, int smallSort, uint64_t address) {
  ++cases;
  if (ok) return;
  if (failures < 20) std::printf("FAIL %s: n=%u cus=%d atomic=%d smallSort=%d address=%llu\n", what, n, cus, atomic, smallSort, (unsigned long long)address);
  ++failures;
}

}  // namespace

int main() {
  using vrdx::StepWide;
  using vrdx::WideValueForm;
  const uint32_t from = vrdx::kWideValueTwoSortsFrom;
  // (2^30 - 4 is where the planners' domain ends -- PlanSort's tile arithmetic is not defined beyond it.  The recorder and the
  // describe call clamp before they plan: for counts beyond, `Clamped` below is their one line, and
  // tests/test_wide_value_abi.py holds the describe call itself to it on a GPU)
  const auto Clamped = [](uint32_t n) { return n > VRDX_MAX_ELEMENTS ? (uint32_t)VRDX_MAX_ELEMENTS : n; };
  const uint32_t sizes[] = {0u, 1u, 8191u, 8192u, 8193u, from - 1u, from, from + 1u, VRDX_MAX_ELEMENTS,
                            Clamped(VRDX_MAX_ELEMENTS + 1u), Clamped(0xFFFFFFFFu)};
  static_assert(vrdx::kWideSmallMaxElements == 8192u, "the one-workgroup form's last size");
  static_assert(vrdx::kWideValueTwoSortsFrom > vrdx::kWideSmallMaxElements + 1u, "the gather form has sizes of its own");
  for (int cus : {8, 256})
    for (int atomic = 0; atomic < 2; ++atomic)
      for (int smallSort = 0; smallSort < 2; ++smallSort) {
        vrdx::PlanContext c;
        c.computeUnits = cus;
        c.atomicRank = atomic != 0;
        c.smallSort = smallSort != 0;
        const uint32_t align = c.minStorageBufferOffsetAlignment;
        for (uint32_t n : sizes) {
          const uint64_t inner = vrdx::MakeLayout(n, align, 0).keyValueSize;
          const uint64_t required = vrdx::MakeWideValueLayout(n, align).size;
          Check(required == inner + 12ull * n + vrdx::WideValuePadBytes(align), "requirement", n, cus, atomic, smallSort, 0);
          Check(vrdx::WideValuePadBytes(16) == 112 + 248, "fixed pad", n, cus, atomic, smallSort, 0);
          const WideValueForm want = n == 0                                              ? WideValueForm::kNone
                                     : (n <= vrdx::kWideSmallMaxElements && smallSort) ? WideValueForm::kOneWorkgroup
                                     : n < from                                         ? WideValueForm::kGather
                                                                                        : WideValueForm::kTwoSorts;
          for (uint64_t address = 0x7000000000ull; address < 0x7000000000ull + 128; address += 16) {
            const vrdx::WideValuePlan p = vrdx::PlanWideValueSort(c, n, address);
            const auto check = [&](bool ok, const char* what) { Check(ok, what, n, cus, atomic, smallSort, address & 127u); };
            check(p.form == want && p.elementCount == n && p.atomicRank == (atomic != 0), "form");
            // the steps
            if (want == WideValueForm::kNone) {
              check(p.stepCount == 0, "steps of the empty sort");
              continue;
            }
            if (want == WideValueForm::kOneWorkgroup) {
              check(p.stepCount == 1 && p.steps[0].what == StepWide::kSmallSort && p.steps[0].slot == 14 &&
                        std::strcmp(p.steps[0].name, "small_sort_wide_kernel") == 0,
                    "steps of one workgroup");
            } else {
              const bool gather = want == WideValueForm::kGather;
              const StepWide kinds[2][4] = {{StepWide::kSplit, StepWide::kSortAB, StepWide::kSortKeysC, StepWide::kMerge},
                                            {StepWide::kIota, StepWide::kSortKeysA, StepWide::kGather, StepWide::kCopyBack}};
              const char* const kernels[2][2] = {{"split_wide_kernel", "merge_wide_kernel"}, {"iota_wide_kernel", "copy_back_wide_kernel"}};
              bool ok = p.stepCount == 4;
              for (uint32_t i = 0; ok && i < 4; ++i) ok = p.steps[i].what == kinds[gather][i] && p.steps[i].slot == i + 1 && p.steps[i].name != nullptr;
              ok = ok && std::strcmp(p.steps[0].name, kernels[gather][0]) == 0 && std::strcmp(p.steps[3].name, kernels[gather][1]) == 0;
              ok = ok && (!gather || std::strcmp(p.steps[2].name, "gather_wide_kernel") == 0);
              check(ok, "steps and slots");
            }
            // the layout
            const vrdx::WideValueLayout& l = p.layout;
            const uint64_t bytes = 4ull * n;
            check(l.innerSize == inner && l.size == required, "sizes do not depend on the address");
            check((address + l.aOffset) % 128 == 0 && (address + l.bOffset) % 128 == 0 && (address + l.cOffset) % 128 == 0, "128-byte lines");
            check(l.aOffset >= l.innerSize && l.aOffset + bytes <= l.bOffset && l.bOffset + bytes <= l.cOffset &&
                      l.cOffset + bytes <= l.size,
                  "A, B, C in order, apart, behind the inner storage, inside the requirement");
            check(l.tOffset == l.bOffset && (address + l.tOffset) % 8 == 0 && l.tOffset + 2 * bytes <= l.cOffset + bytes &&
                      l.tOffset + 2 * bytes <= l.size && l.aOffset + bytes <= l.tOffset,
                  "T over B and C");
            // the description
            VrdxHipWideValuePlanInfo info;
            std::memset(&info, 0, sizeof(info));
            vrdx::DescribeWideValuePlan(c, p, &info);
            VrdxHipPlanInfo innerInfo;
            std::memset(&innerInfo, 0, sizeof(innerInfo));
            vrdx::DescribePlan(vrdx::PlanSort(c, true, n, 0), &innerInfo);
            bool ok = info.form == (uint32_t)want && info.twoSortsFrom == from && info.oneWorkgroupMax == (smallSort ? 8192u : 0u);
            if (want == WideValueForm::kOneWorkgroup)
              ok = ok && info.launches == 1 && info.bytesPerElement == 24 && info.innerPlan == 0;
            else if (want == WideValueForm::kGather)
              ok = ok && info.launches == 3 + innerInfo.launches && info.bytesPerElement == 40 + innerInfo.bytesPerElement &&
                   info.innerPlan == innerInfo.plan;
            else
              ok = ok && info.launches == 2 + 2 * innerInfo.launches && info.bytesPerElement == 40 + 2 * innerInfo.bytesPerElement &&
                   info.innerPlan == innerInfo.plan;
            check(ok, "description");
          }
        }
      }
  std::printf("two sorts from %u, one workgroup up to %u\n", from, vrdx::kWideSmallMaxElements);
  std::printf("wide value plan: %ld cases, %d failures\n", cases, failures);
  return failures == 0 ? 0 : 1;
}
