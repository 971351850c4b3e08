// Shared by the CPU checks of the host planner (layout_check.cpp, plan_check.cpp, sanitized_host_check.cpp): the element
// counts they sweep, the sizes at which the plan changes on an MI355X, and what must hold of every plan PlanSort makes.
#ifndef VRDX_TESTS_PLAN_INVARIANTS_H
#define VRDX_TESTS_PLAN_INVARIANTS_H

#include <cstdint>
#include <initializer_list>

#include "../../vulkan_radix_sort_amd/csrc/vrdx_plan.h"

namespace plan_test {

constexpr uint32_t kCuCounts[] = {256, 304, 64, 8};

// The last size of every plan, by the rules of vrdx_plan.h (HybridCapacity, MsdBits) -- behaviour: plan_check derives the
// same list from the functions themselves.  With the ballot ranking there is no MSD plan and no bucket of 32768.
constexpr uint32_t kAtomicEdges[] = {16384, 524288, 1048576, 2097152, 8144384, 18149376, 36649984, 67108864};
constexpr uint32_t kBallotEdges[] = {16384, 524288, 1048576, 4072192};

// check(n, dense): every element count the layout and plan checks sweep; dense marks the counts worth every alignment.
template <typename Check>
void ForEachSweptCount(Check&& check) {
  for (uint32_t n = 0; n <= 70000; ++n) check(n, n % 97 == 0);
  for (uint64_t n = 70001; n <= VRDX_MAX_ELEMENTS; n += 1 + n / 977) check((uint32_t)n, false);
  for (uint32_t lg = 10; lg < 30; ++lg)
    for (int d = -2; d <= 2; ++d) check((1u << lg) + d, true);
  // the edges of the rounds: multiples of one round of every geometry and CU count, +- a few keys and +- one granule
  for (uint32_t cus : kCuCounts)
    for (uint32_t capacity : {32768u, 65536u})
      for (uint32_t rounds = 1; rounds <= 6; ++rounds)
        for (int d : {-4097, -4096, -1, 0, 1, 2, 4095, 4096, 4097, 8192, 8193})
          check((uint32_t)((int64_t)rounds * cus * capacity + d), true);
  check(VRDX_MAX_ELEMENTS, true);
  // the MSD plan's range: its first size, where its buckets go from half to full size, where it goes from ten to eleven
  // bits, its last size, tile edges
  for (uint32_t n : {8144385u, 8388608u, 16252929u, 16252930u, 18149376u, 35790291u, 35790292u, 36649984u, 36651000u, 67108863u,
                     67108864u, 67108865u})
    for (int d : {-32769, -32768, -1, 0, 1, 32767, 32768})
      check((uint32_t)((int64_t)n + d), true);
}

// What holds of the plan PlanSort makes of ANY context, element count and storage address (vrdx_plan.h).
inline bool PlanInvariantsHold(const vrdx::PlanContext& c, bool keyValue, uint32_t n, uint64_t storageAddress) {
  using vrdx::Step;
  const vrdx::SortPlan p = vrdx::PlanSort(c, keyValue, n, storageAddress);
  bool ok = p.stepCount <= vrdx::kMaxSortSteps && p.keyValue == keyValue && p.elementCount == n && p.atomicRank == c.atomicRank;
  uint32_t launches = 0, count[10] = {};
  int bucketSortAt = -1, firstPassAt = -1;
  uint32_t passes[4], passCount = 0;
  for (uint32_t i = 0; i < p.stepCount && ok; ++i) {
    const vrdx::SortStep& s = p.steps[i];
    ok = ok && s.slot <= 14 && (i == 0 || s.slot > p.steps[i - 1].slot) && s.name != nullptr && (uint32_t)s.what < 10;
    if (!ok) break;
    if (s.what != Step::kFill) ++launches;
    ++count[(uint32_t)s.what];
    if (s.what == Step::kBucketSort) bucketSortAt = (int)i;
    if (s.what == Step::kPass) {
      if (firstPassAt < 0) firstPassAt = (int)i;
      ok = ok && passCount < 4 && s.slot == 4 + 3 * s.pass;
      if (ok) passes[passCount++] = s.pass;
    }
  }
  const auto has = [&count](Step what) { return count[(uint32_t)what] == 1; };
  const auto none = [&count](Step what) { return count[(uint32_t)what] == 0; };
  ok = ok && p.launches == launches;
  // the refused sort and the empty one record nothing
  if (!p.fits || n == 0) return ok && p.stepCount == 0 && p.launches == 0 && (p.fits || n != 0);
  // one step, at slot 14, if and only if the sort takes one workgroup
  const bool oneStep = p.stepCount == 1 && p.steps[0].slot == 14;
  ok = ok && oneStep == p.oneWorkgroup && has(Step::kSmallSort) == p.oneWorkgroup;
  ok = ok && (!p.oneWorkgroup || (n <= vrdx::kSmallSortMaxElements && p.hybridCap == 0 && p.msdBits == 0));
  if (p.oneWorkgroup) return ok;
  ok = ok && has(Step::kFill) && p.steps[0].what == Step::kFill && p.steps[0].slot == 1 && none(Step::kSmallSort);
  // the MSD plan's steps if and only if the plan is recorded; then passes 1-3 follow half-size buckets, passes 2-3 full-size ones
  const bool msd = p.msdBits != 0, half = msd && p.msdCap == vrdx::kMsdHalfCap;
  ok = ok && has(Step::kHistogramMsd) == msd && has(Step::kSpineMsd) == msd && has(Step::kMsdScatterOrPass0) == msd;
  ok = ok && has(Step::kHistogram) == !msd && has(Step::kBucketSortHalf) == half && has(Step::kMsdBucketsOrPass1) == (msd && !half);
  ok = ok && (has(Step::kBucketSortHalf) || none(Step::kBucketSortHalf)) && (has(Step::kMsdBucketsOrPass1) || none(Step::kMsdBucketsOrPass1));
  const uint32_t firstPass = !msd ? 0u : half ? 1u : 2u;
  ok = ok && passCount == 4 - firstPass;
  for (uint32_t i = 0; i < passCount; ++i) ok = ok && passes[i] == firstPass + i;
  if (msd) {
    ok = ok && (p.msdBits == 10 || p.msdBits == 11) && (p.msdCap == vrdx::kMsdHalfCap || p.msdCap == (keyValue ? vrdx::kMsdCapKeyValue : vrdx::kMsdCapKeys));
    ok = ok && p.hybridCap == 0 && c.atomicRank && p.configIndex == (keyValue ? vrdx::kCfg1024x32 : vrdx::kCfg1024x32x2);
    ok = ok && firstPassAt >= 5 && p.steps[firstPassAt - 1].slot == 5 && p.steps[firstPassAt - 2].what == Step::kMsdScatterOrPass0;
  }
  // the eight-bit plan: its bucket sort right in front of pass 1, never with block sums
  ok = ok && (bucketSortAt >= 0) == (p.hybridCap != 0);
  if (p.hybridCap != 0)
    ok = ok && !p.blockSums && !msd && bucketSortAt >= 1 && (uint32_t)bucketSortAt + 1 < p.stepCount &&
         p.steps[bucketSortAt - 1].what == Step::kPass && p.steps[bucketSortAt - 1].pass == 0 &&
         p.steps[bucketSortAt + 1].what == Step::kPass && p.steps[bucketSortAt + 1].pass == 1;
  ok = ok && p.configIndex >= 0 && p.configIndex < vrdx::kNumTileConfigs && p.tilePlan.tiles >= 1;
  const uint32_t grid = vrdx::HistogramGrid(c, p);
  ok = ok && grid >= 1 && grid <= (uint32_t)c.computeUnits;
  // a forced tile geometry: the general path with that geometry at every size and no plan in front (the two-sub-tile kernel is
  // keys-only and needs the one-atomic ranking: 1024x32 otherwise)
  if (c.forcedConfig >= 0) {
    const bool noPair = c.forcedConfig == vrdx::kCfg1024x32x2 && (keyValue || !c.atomicRank);
    ok = ok && p.hybridCap == 0 && !msd && p.configIndex == (noPair ? vrdx::kCfg1024x32 : c.forcedConfig);
  }
  return ok;
}

}  // namespace plan_test

#endif  // VRDX_TESTS_PLAN_INVARIANTS_H
