// CPU-only check of the plan of the bit-range sorts (vrdx_plan.h, PlanSortBits), compiled and run by
// tests/test_sort_bits_plan.py (also under ASan + UBSan).  For 256 CUs, both rankings, keys-only and key+value, every range
// (b, e) with 0 <= b <= e <= 33 at the sizes given on the command line (default: those of tests/sort_bits_cases.py):
//   up to 16384 elements one step, small_sort_bits_kernel at slot 14, one launch, 8 / 16 bytes per element, a layout that fits;
//   beyond: no step and fits == false (range sorts beyond one workgroup are refused);
//   no hybrid or MSD step anywhere; (0, 32) equals PlanSort; empty and invalid ranges have no step.
// All of it under every planning knob that sends PlanSort down the general path at small sizes -- smallSort on and off times
// forcedConfig -1, 0 ... 3: a range over part of the key is planned by size alone, the plan being PlanSort's under the default
// knobs field by field (a range sort has no general-path form for a knob to select), and (0, 32) follows the knobs as PlanSort
// does.
// Prints one line per size, ranking and value mode: `plan <n> <atomic: 0 | 1> <key+value: 0 | 1> <one-workgroup | refused>`.
// Nothing of HIP is linked (vrdx_kernels.h needs one of its headers).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vulkan_radix_sort_amd/csrc/vrdx_plan.h"

namespace {

int failures = 0;
void Fail(const char* what, uint32_t n, int atomic, int keyValue, uint32_t b, uint32_t e) {
  if (failures < 20) std::printf("FAIL %s: n=%u atomic=%d key+value=%d range=[%u,%u)\n", what, n, atomic, keyValue, b, e);
  ++failures;
}

bool SamePlan(const vrdx::SortPlan& x, const vrdx::SortPlan& y) {
  bool same = x.keyValue == y.keyValue && x.elementCount == y.elementCount && x.oneWorkgroup == y.oneWorkgroup &&
              x.hybridCap == y.hybridCap && x.msdBits == y.msdBits && x.msdCap == y.msdCap && x.configIndex == y.configIndex &&
              x.blockSums == y.blockSums && x.fits == y.fits && x.stepCount == y.stepCount && x.launches == y.launches &&
              x.rangeWidth == y.rangeWidth && x.tilePlan.tiles == y.tilePlan.tiles && x.tilePlan.slots == y.tilePlan.slots &&
              x.tilePlan.fullTiles == y.tilePlan.fullTiles && x.tilePlan.tailSlots == y.tilePlan.tailSlots &&
              std::memcmp(&x.layout, &y.layout, sizeof(x.layout)) == 0;
  for (uint32_t i = 0; same && i < x.stepCount; ++i)
    same = x.steps[i].what == y.steps[i].what && x.steps[i].pass == y.steps[i].pass && x.steps[i].slot == y.steps[i].slot;
  return same;
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<uint32_t> sizes;
  for (int i = 1; i < argc; ++i) sizes.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
  if (sizes.empty()) sizes = {1, 2, 257, 4096, 4097, 16383, 16384, 16385, 65539, 8400000};
  uint64_t cases = 0;
  for (uint32_t n : sizes)
    for (int atomic = 1; atomic >= 0; --atomic)
      for (int keyValue = 0; keyValue < 2; ++keyValue) {
        const bool kv = keyValue != 0;
        char geometry[64] = "";
        for (int smallSort = 1; smallSort >= 0; --smallSort)
          for (int forced = -1; forced < vrdx::kNumTileConfigs; ++forced) {
            vrdx::PlanContext c, defaults;
            c.computeUnits = defaults.computeUnits = 256;
            c.atomicRank = defaults.atomicRank = atomic != 0;
            c.smallSort = smallSort != 0;
            c.forcedConfig = forced;
            for (uint32_t b = 0; b <= 32; ++b)
              for (uint32_t e = b; e <= 33; ++e) {
                const vrdx::SortPlan p = vrdx::PlanSortBits(c, kv, n, b, e, 0);
                ++cases;
                if (e == b || e > 32) {  // the empty range records nothing and is fine; the invalid one is refused
                  if (p.stepCount != 0 || p.launches != 0 || p.fits != (e <= 32)) Fail("empty or invalid range", n, atomic, keyValue, b, e);
                  continue;
                }
                if (b == 0 && e == 32) {  // the whole key: PlanSort under the same knobs
                  const vrdx::SortPlan sort = vrdx::PlanSort(c, kv, n, 0);
                  if (!SamePlan(p, sort) || p.rangeWidth != 0) Fail("(0, 32) is not PlanSort", n, atomic, keyValue, b, e);
                  if (n != 0 && n <= vrdx::kSmallSortMaxElements && sort.oneWorkgroup != (smallSort != 0 && forced < 0))
                    Fail("(0, 32) does not follow the knobs", n, atomic, keyValue, b, e);
                  VrdxHipPlanInfo whole = {}, ranged = {};
                  vrdx::DescribePlan(sort, &whole);
                  vrdx::DescribePlan(p, &ranged);
                  if (std::memcmp(&whole, &ranged, sizeof(whole)) != 0) Fail("(0, 32) described", n, atomic, keyValue, b, e);
                  continue;
                }
                const uint32_t width = e - b;
                bool ok = p.hybridCap == 0 && p.msdBits == 0 && p.atomicRank == c.atomicRank && p.keyValue == kv && p.elementCount == n;
                VrdxHipPlanInfo info = {};
                char now[64];
                if (n <= vrdx::kSmallSortMaxElements) {
                  vrdx::DescribePlan(p, &info);
                  ok = ok && p.fits && p.rangeBegin == b && p.rangeWidth == width && p.oneWorkgroup && p.stepCount == 1 && p.launches == 1 &&
                       p.steps[0].what == vrdx::Step::kSmallSortBits && p.steps[0].slot == 14 && p.steps[0].name != nullptr &&
                       info.plan == VRDX_HIP_PLAN_ONE_WORKGROUP && info.bits == 0 && info.launches == 1 &&
                       info.bytesPerElement == (kv ? 16u : 8u) && info.fallbackBytesPerElement == info.bytesPerElement &&
                       vrdx::LayoutFits(p.layout, n);
                  // the knobs play no part: but for the range and its one step, PlanSort's plan under the default knobs
                  vrdx::SortPlan whole = vrdx::PlanSort(defaults, kv, n, 0), same = p;
                  same.rangeBegin = same.rangeWidth = 0;
                  ok = ok && whole.oneWorkgroup && whole.stepCount == 1 && whole.steps[0].what == vrdx::Step::kSmallSort;
                  same.steps[0].what = vrdx::Step::kSmallSort;
                  ok = ok && SamePlan(same, whole);
                  std::snprintf(now, sizeof(now), "one-workgroup");
                } else {
                  ok = ok && !p.fits && p.refusal != nullptr && p.stepCount == 0 && p.launches == 0 && !p.oneWorkgroup;
                  std::snprintf(now, sizeof(now), "refused");
                }
                if (!ok) Fail("range plan", n, atomic, keyValue, b, e);
                // one answer per (n, ranking, value mode), whatever the range and whatever the knobs
                if (geometry[0] == 0) std::snprintf(geometry, sizeof(geometry), "%s", now);
                if (std::strcmp(geometry, now) != 0) Fail("the plan depends on the range or on a knob", n, atomic, keyValue, b, e);
              }
          }
        std::printf("plan %u %d %d %s\n", n, atomic, keyValue, geometry);
      }
  std::printf("sort bits plan: %llu cases, %d failures\n", (unsigned long long)cases, failures);
  return failures != 0;
}
