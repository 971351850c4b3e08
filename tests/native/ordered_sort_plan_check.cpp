// CPU-only check of the plans of the ordered 32-bit sorts (vrdx_plan.h: PlanOrderedSort, and PlanSegmentedSort with an order
// word for 4-byte keys), compiled and run by tests/test_ordered_sort_plan.py.  At 8 and 256 CUs, both rankings, keys-only and
// key+value, for counts either side of 16384 and of every size at which PlanSort changes plan (found here by bisection on
// PlanSort itself), and every order word of {0, 1, 2, 0x100, 0x101, 0x102, 3, 0x200, 0x10002}:
//   order 0            PlanOrderedSort is PlanSort field for field, and describes itself the same;
//   a valid order      the twin's plan and steps, with small_sort_ordered_kernel in place of small_sort_kernel, or with the two
//                      transform steps first (slot 1, in front of the fill, which ends slot 1 too) and last (slot 14, behind
//                      pass 3 at slot 13): two launches more, nothing else moved;
//   an invalid word    no step, fits == false and the key-order refusal;
//   the segmented plan order 0 identical to the plan without one, valid orders the ordered kernel names on the same grids and
//                      slots, invalid orders and an order with a partial bit range refused.
// Prints one line per CU count, ranking and value mode with the sizes at which the plan changes.  Nothing of HIP is linked.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../vulkan_radix_sort_amd/csrc/vrdx_plan.h"

namespace {

int failures = 0;
void Fail(const char* what, uint32_t n, int cus, int atomic, int keyValue, uint32_t order) {
  if (failures < 20) std::printf("FAIL %s: n=%u cus=%d atomic=%d key+value=%d order=0x%x\n", what, n, cus, atomic, keyValue, order);
  ++failures;
}

bool SameStep(const vrdx::SortStep& x, const vrdx::SortStep& y) {
  return x.what == y.what && x.pass == y.pass && x.slot == y.slot && std::strcmp(x.name, y.name) == 0;
}

// every field but the steps, their count and the order word
bool SameDecisions(const vrdx::SortPlan& x, const vrdx::SortPlan& y) {
  return x.keyValue == y.keyValue && x.elementCount == y.elementCount && x.atomicRank == y.atomicRank &&
         x.oneWorkgroup == y.oneWorkgroup && x.hybridCap == y.hybridCap && x.msdBits == y.msdBits && x.msdCap == y.msdCap &&
         x.msdTileKeys == y.msdTileKeys && x.msdTiles == y.msdTiles && x.configIndex == y.configIndex &&
         std::memcmp(&x.tilePlan, &y.tilePlan, sizeof(x.tilePlan)) == 0 && x.blockSums == y.blockSums && x.fits == y.fits &&
         x.refusal == y.refusal && std::memcmp(&x.layout, &y.layout, sizeof(x.layout)) == 0 && x.rangeBegin == y.rangeBegin &&
         x.rangeWidth == y.rangeWidth;
}

bool SamePlan(const vrdx::SortPlan& x, const vrdx::SortPlan& y) {
  bool same = SameDecisions(x, y) && x.stepCount == y.stepCount && x.launches == y.launches && x.order == y.order;
  for (uint32_t i = 0; same && i < x.stepCount; ++i) same = SameStep(x.steps[i], y.steps[i]);
  return same;
}

// what tells two plans apart when looking for the sizes at which PlanSort changes plan
std::string Kind(const vrdx::SortPlan& p) {
  char text[64];
  std::snprintf(text, sizeof(text), "%d/%u/%u/%u", p.oneWorkgroup ? 1 : 0, p.hybridCap, p.msdBits, p.msdCap);
  return text;
}

}  // namespace

int main() {
  const uint32_t orders[] = {0u, 1u, 2u, 0x100u, 0x101u, 0x102u, 3u, 0x200u, 0x10002u};
  uint64_t cases = 0;
  for (int cus : {8, 256})
    for (int atomic = 1; atomic >= 0; --atomic)
      for (int keyValue = 0; keyValue < 2; ++keyValue) {
        vrdx::PlanContext c;
        c.computeUnits = cus;
        c.atomicRank = atomic != 0;
        const bool kv = keyValue != 0;
        // the sizes at which the plan changes: a coarse walk, then bisection between two sizes of different kinds
        std::set<uint32_t> sizes = {0u, 1u, 2u, 16383u, 16384u, 16385u, 16386u, VRDX_MAX_ELEMENTS};
        std::string edges;
        uint32_t before = 1;
        for (uint64_t n = 2; n <= VRDX_MAX_ELEMENTS; n += 1 + n / 64) {
          if (Kind(vrdx::PlanSort(c, kv, (uint32_t)n, 0)) != Kind(vrdx::PlanSort(c, kv, before, 0))) {
            uint32_t lo = before, hi = (uint32_t)n;  // (lo: the old kind; a second change inside the step is not looked for)
            while (hi - lo > 1) {
              const uint32_t mid = lo + (hi - lo) / 2;
              (Kind(vrdx::PlanSort(c, kv, mid, 0)) == Kind(vrdx::PlanSort(c, kv, lo, 0)) ? lo : hi) = mid;
            }
            sizes.insert(lo);
            sizes.insert(hi);
            edges += " " + std::to_string(lo);
          }
          before = (uint32_t)n;
        }
        for (uint32_t n : sizes) {
          const vrdx::SortPlan twin = vrdx::PlanSort(c, kv, n, 0);
          VrdxHipPlanInfo twinInfo = {};
          vrdx::DescribePlan(twin, &twinInfo);
          for (uint32_t order : orders) {
            const vrdx::SortPlan p = vrdx::PlanOrderedSort(c, kv, n, order, 0);
            ++cases;
            if (order == 0) {
              VrdxHipPlanInfo info = {};
              vrdx::DescribePlan(p, &info);
              if (!SamePlan(p, twin) || std::memcmp(&info, &twinInfo, sizeof(info)) != 0) Fail("order 0 is not PlanSort", n, cus, atomic, keyValue, order);
              continue;
            }
            if (!vrdx::KeyOrderValid(order)) {
              if (p.stepCount != 0 || p.launches != 0 || p.fits || p.refusal != vrdx::kKeyOrderRefused) Fail("an invalid word", n, cus, atomic, keyValue, order);
              continue;
            }
            bool ok = SameDecisions(p, twin) && p.stepCount <= vrdx::kMaxSortSteps;
            if (twin.stepCount == 0) {  // the empty sort (and one PlanSort refuses): no step, no transform
              ok = ok && p.stepCount == 0 && p.launches == 0;
            } else if (twin.oneWorkgroup) {
              ok = ok && p.order == order && p.stepCount == 1 && p.launches == 1 && p.steps[0].what == vrdx::Step::kSmallSortOrdered &&
                   p.steps[0].slot == 14 && std::strcmp(p.steps[0].name, "small_sort_ordered_kernel") == 0 && n <= 16384;
            } else {
              ok = ok && p.order == order && n > 16384 && p.stepCount == twin.stepCount + 2 && p.launches == twin.launches + 2;
              const vrdx::SortStep &first = p.steps[0], &last = p.steps[p.stepCount - 1];
              ok = ok && first.what == vrdx::Step::kOrderForward && first.slot == 1 && std::strcmp(first.name, "order32_kernel") == 0;
              ok = ok && last.what == vrdx::Step::kOrderInverse && last.slot == 14 && std::strcmp(last.name, "order32_kernel") == 0;
              for (uint32_t i = 0; ok && i < twin.stepCount; ++i) ok = SameStep(p.steps[1 + i], twin.steps[i]);
              // the fill ends slot 1 right behind the forward transform; no step of the twin ends slot 14
              ok = ok && p.steps[1].what == vrdx::Step::kFill && p.steps[1].slot == 1 && p.steps[p.stepCount - 2].slot == 13;
            }
            if (!ok) Fail("an ordered plan", n, cus, atomic, keyValue, order);
          }
          // the segmented plan of 4-byte keys
          for (uint32_t segments : {0u, 1u, 2u * (uint32_t)cus + 1u}) {
            const vrdx::SegmentedPlan plain = vrdx::PlanSegmentedSort(c, 4, kv, n, segments, vrdx::SegmentedKey{}, 0);
            for (uint32_t order : orders) {
              const vrdx::SegmentedPlan p = vrdx::PlanSegmentedSort(c, 4, kv, n, segments, vrdx::SegmentedKey{0, 32, order}, 0);
              ++cases;
              bool ok = true;
              if (!vrdx::KeyOrderValid(order)) {
                ok = p.stepCount == 0 && p.refusal == vrdx::kKeyOrderRefused;
              } else {
                ok = p.refusal == nullptr && p.stepCount == plain.stepCount && p.order == order && p.rangeWidth == 0 &&
                     p.keyValue == plain.keyValue && p.atomicRank == plain.atomicRank &&
                     std::memcmp(&p.layout, &plain.layout, sizeof(p.layout)) == 0;
                static const char* const kOrdered[4] = {"segmented_clear_kernel", "segmented_small_ordered_kernel",
                                                        "segmented_mid_ordered_kernel", "segmented_large_ordered_kernel"};
                for (uint32_t i = 0; ok && i < p.stepCount; ++i) {
                  const vrdx::SegmentedSortStep &x = p.steps[i], &y = plain.steps[i];
                  ok = x.what == y.what && x.slot == y.slot && x.grid == y.grid &&
                       std::strcmp(x.name, order == 0 ? y.name : kOrdered[(int)x.what]) == 0;
                }
              }
              if (!ok) Fail("a segmented plan", n, cus, atomic, keyValue, order);
              // an order with a partial range is not built; with an empty or invalid range the range's own rule comes first
              if (order != 0 && vrdx::KeyOrderValid(order)) {
                const vrdx::SegmentedPlan ranged = vrdx::PlanSegmentedSort(c, 4, kv, n, segments, vrdx::SegmentedKey{3, 20, order}, 0);
                const vrdx::SegmentedPlan invalid = vrdx::PlanSegmentedSort(c, 4, kv, n, segments, vrdx::SegmentedKey{9, 4, order}, 0);
                if (ranged.refusal == nullptr || ranged.stepCount != 0 || invalid.refusal != vrdx::kBitRangeRefused)
                  Fail("an order with a bit range", n, cus, atomic, keyValue, order);
              }
            }
          }
        }
        std::printf("cus %d atomic %d key+value %d: the plan changes behind%s (%zu sizes)\n", cus, atomic, keyValue, edges.c_str(),
                    sizes.size());
      }
  std::printf("ordered sort plan: %llu cases, %d failures\n", (unsigned long long)cases, failures);
  return failures != 0;
}
