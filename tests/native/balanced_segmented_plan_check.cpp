// CPU-only check of the plan and the layout of the balanced segmented sort (vrdx_plan.h, PlanBalancedSegmentedSort;
// vrdx_layout.h, MakeBalancedSegmentedLayout and the caps), compiled and run by tests/test_balanced_segmented_plan.py (also
// under ASan + UBSan).
// usage: balanced_segmented_plan_check <compute units> <maxElementCount> ...
// For both rankings, keys-only and key+value, segment counts 1, 3 and 100000 and every storage address modulo 128, at every
// bound given:
//   up to 65536 elements the plan is PlanSegmentedSort's, step for step, and has no step of its own;
//   beyond, the balanced form: 18 launches -- fill, small, mid in slots 1-3 with the twin's grids, the split and the large
//   kernel on the rest in slot 4, count and scan in slot 5 + 2 p and the scatter in slot 6 + 2 p for p = 0 ... 3, the copy
//   back in slot 13 -- the caps equal to their derivation, the twin's counters and lists where the twin keeps them, and the
//   rest list, the split words, both tables, the rows (on a 128-byte line) and both scratch arrays (on 128-byte lines) behind
//   one another inside the storage requirement;
//   PlanSegmentedSort itself answers as before: its names, slots and grids are re-derived here.
// Prints one line per bound: `plan <cus> <n> <form> <spreadCap> <pieceCap> <split> <keysScratch> <valuesScratch>` (the three
// offsets at address 127; 0 where the form is not the balanced one), then the number of cases and failures.
// Nothing of HIP is linked (vrdx_kernels.h needs one of its headers).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vulkan_radix_sort_amd/csrc/vrdx_plan.h"

namespace {

int failures = 0;
void Fail(const char* what, uint32_t n, uint32_t segments, int atomic, int keyValue, uint32_t address) {
  if (failures < 20)
    std::printf("FAIL %s: n=%u segments=%u atomic=%d key+value=%d address=%u\n", what, n, segments, atomic, keyValue, address);
  ++failures;
}

bool SameSegmentedPlan(const vrdx::SegmentedPlan& x, const vrdx::SegmentedPlan& y) {
  bool same = x.keyValue == y.keyValue && x.atomicRank == y.atomicRank && x.refusal == y.refusal && x.rangeBegin == y.rangeBegin &&
              x.rangeWidth == y.rangeWidth && x.order == y.order && x.stepCount == y.stepCount;
  if (same && x.stepCount != 0)
    same = x.layout.midCountOffset == y.layout.midCountOffset && x.layout.largeCountOffset == y.layout.largeCountOffset &&
           x.layout.midListOffset == y.layout.midListOffset && x.layout.largeListOffset == y.layout.largeListOffset &&
           x.layout.midCap == y.layout.midCap && x.layout.largeCap == y.layout.largeCap &&
           x.layout.keysScratchOffset == y.layout.keysScratchOffset &&
           x.layout.valuesScratchOffset == y.layout.valuesScratchOffset && x.layout.fits == y.layout.fits;
  for (uint32_t i = 0; same && i < x.stepCount; ++i)
    same = x.steps[i].what == y.steps[i].what && x.steps[i].slot == y.steps[i].slot && x.steps[i].name == y.steps[i].name &&
           x.steps[i].grid == y.steps[i].grid;
  return same;
}

// the twin as it has always answered, derived again: a fill and three launches in slots 1-4, a launch of grid 0 absent
bool TwinAsBefore(const vrdx::SegmentedPlan& p, uint32_t n, uint32_t segments, uint32_t cus) {
  if (n == 0 || segments == 0) return p.stepCount == 0 && p.refusal == nullptr;
  static const char* const names[4] = {"segmented_clear_kernel", "segmented_small_kernel", "segmented_mid_kernel",
                                       "segmented_large_kernel"};
  const uint32_t grids[4] = {1u, std::min<uint32_t>(segments, 1u << 20), std::min<uint32_t>(std::min(segments, n / 4097u), 2u * cus),
                             std::min<uint32_t>(std::min(segments, n / 16385u), 2u * cus)};
  uint32_t at = 0;
  for (uint32_t i = 0; i < 4; ++i) {
    if (grids[i] == 0) continue;
    if (at >= p.stepCount || (uint32_t)p.steps[at].what != i || p.steps[at].slot != i + 1 || p.steps[at].grid != grids[i] ||
        std::strcmp(p.steps[at].name, names[i]) != 0)
      return false;
    ++at;
  }
  return at == p.stepCount && p.layout.midCap == n / 4097u && p.layout.largeCap == n / 16385u && p.layout.fits;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint32_t cus = (uint32_t)std::atoi(argv[1]);
  std::vector<uint32_t> sizes;
  for (int i = 2; i < argc; ++i) sizes.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
  unsigned long long cases = 0;
  for (const uint32_t n : sizes) {
    uint32_t formSeen = 0, spreadSeen = 0, pieceSeen = 0;
    unsigned long long scratchSeen = 0, valuesSeen = 0, splitSeen = 0;  // (of the last case: key+value, address 127)
    for (int atomic = 0; atomic < 2; ++atomic)
      for (int keyValue = 0; keyValue < 2; ++keyValue)
        for (const uint32_t segments : {1u, 3u, 100000u})
          for (uint32_t address = 0; address < 128; ++address) {
            ++cases;
            vrdx::PlanContext c;
            c.computeUnits = (int)cus;
            c.atomicRank = atomic != 0;
            const auto fail = [&](const char* what) { Fail(what, n, segments, atomic, keyValue, address); };
            const vrdx::SegmentedPlan twin = vrdx::PlanSegmentedSort(c, 4, keyValue != 0, n, segments, vrdx::SegmentedKey{}, address);
            if (!TwinAsBefore(twin, n, segments, cus)) fail("PlanSegmentedSort changed");
            const vrdx::BalancedSegmentedPlan p = vrdx::PlanBalancedSegmentedSort(c, keyValue != 0, n, segments, address);
            VrdxHipBalancedSegmentedPlanInfo info{};
            vrdx::DescribeBalancedSegmentedPlan(p, &info);
            formSeen = info.form, spreadSeen = info.spreadCap, pieceSeen = info.pieceCap;
            if (info.spreadFrom != 65536u || info.spreadShares != 3u || info.minPieceKeys != 16384u || info.launches != p.launches)
              fail("describe");
            // the caps against their derivation
            const uint32_t spreadCap = std::min<uint32_t>(n / 65537u, std::min<uint32_t>((cus - 1u) / 3u, 256u));
            const uint32_t pieceCap = spreadCap != 0 ? std::min<uint32_t>(cus, n / 16384u) + spreadCap : 0u;
            if (vrdx::SegSpreadCap(n, cus) != spreadCap || vrdx::SegPieceCap(n, cus) != pieceCap) fail("caps");
            if (n <= 65536u || spreadCap == 0) {
              if (p.form == vrdx::BalancedForm::kBalanced || p.stepCount != 0 || !SameSegmentedPlan(p.twin, twin) ||
                  p.launches != twin.stepCount || info.spreadCap != 0 || info.pieceCap != 0 ||
                  (p.form == vrdx::BalancedForm::kTwin) != (twin.stepCount != 0))
                fail("the twin's plan up to 65536 elements");
              continue;
            }
            if (p.form != vrdx::BalancedForm::kBalanced || p.refusal != nullptr || p.launches != 18 || p.stepCount != 18 ||
                info.spreadCap != spreadCap || info.pieceCap != pieceCap) {
              fail("the balanced form");
              continue;
            }
            // the steps: kinds, slots, grids
            using S = vrdx::StepBalanced;
            const S kinds[18] = {S::kClear, S::kSmall, S::kMid, S::kSplit, S::kLargeRest, S::kCount, S::kScan, S::kScatter,
                                 S::kCount, S::kScan, S::kScatter, S::kCount, S::kScan, S::kScatter, S::kCount, S::kScan,
                                 S::kScatter, S::kCopyBack};
            bool steps = true;
            for (uint32_t i = 0; i < 18; ++i) {
              const vrdx::BalancedSegmentedStep& s = p.steps[i];
              const uint32_t pass = i >= 5 && i < 17 ? (i - 5) / 3 : 0;
              uint32_t slot = 0, grid = 0;
              switch (kinds[i]) {
                case S::kClear: slot = 1, grid = 1; break;
                case S::kSmall: slot = 2, grid = twin.steps[1].grid; break;
                case S::kMid: slot = 3, grid = twin.steps[2].grid; break;
                case S::kSplit: slot = 4, grid = 1; break;
                case S::kLargeRest: slot = 4, grid = twin.steps[3].grid; break;
                case S::kCount: slot = 5 + 2 * pass, grid = pieceCap; break;
                case S::kScan: slot = 5 + 2 * pass, grid = spreadCap; break;
                case S::kScatter: slot = 6 + 2 * pass, grid = pieceCap; break;
                case S::kCopyBack: slot = 13, grid = pieceCap; break;
              }
              steps = steps && s.what == kinds[i] && s.slot == slot && s.grid == grid && s.grid != 0 && s.pass == pass && s.name != nullptr;
            }
            if (!steps || twin.stepCount != 4) fail("steps, slots and grids");
            // the layout: the twin's counters and lists, then everything behind one another inside the requirement
            const vrdx::BalancedSegmentedLayout& l = p.layout;
            const vrdx::StorageLayout whole = vrdx::MakeLayout(n, c.minStorageBufferOffsetAlignment, 0, address);
            const uint64_t size = keyValue ? whole.keyValueSize : whole.keysOnlySize;
            const uint64_t bytes = 4ull * n;
            const bool lists = l.lists.midCountOffset == twin.layout.midCountOffset && l.lists.largeCountOffset == twin.layout.largeCountOffset &&
                               l.lists.midListOffset == twin.layout.midListOffset && l.lists.largeListOffset == twin.layout.largeListOffset &&
                               l.lists.midCap == twin.layout.midCap && l.lists.largeCap == twin.layout.largeCap;
            const bool order = l.lists.largeListOffset + 4ull * l.lists.largeCap <= l.restListOffset &&
                               l.restListOffset + 4ull * l.lists.largeCap <= l.splitOffset &&
                               l.splitOffset + 4ull * vrdx::kSegSplitWords <= l.spreadTableOffset &&
                               l.spreadTableOffset + 4ull * vrdx::kSegSpreadEntryWords * spreadCap <= l.pieceTableOffset &&
                               l.pieceTableOffset + 4ull * vrdx::kSegPieceEntryWords * pieceCap <= l.rowsOffset &&
                               l.rowsOffset + 1024ull * pieceCap <= l.lists.keysScratchOffset &&
                               l.lists.keysScratchOffset + bytes <= (keyValue ? l.lists.valuesScratchOffset : size) &&
                               (!keyValue || l.lists.valuesScratchOffset + bytes <= size);
            const bool aligned = (address + l.rowsOffset) % 128 == 0 && (address + l.lists.keysScratchOffset) % 128 == 0 &&
                                 (address + l.lists.valuesScratchOffset) % 128 == 0 && (address + l.splitOffset) % 4 == 0;
            // the rows take at most N / 16384 + N / 65537 KiB of the ceil(N / 4096) KiB of the reference's partition histograms
            const bool rows = 1024ull * pieceCap <= 1024ull * (n / 16384u + n / 65537u) && l.rowsOffset + 1024ull * pieceCap <= whole.keysOnlySize - bytes;
            if (!l.lists.fits || !lists || !order || !aligned || !rows) fail("layout");
            scratchSeen = l.lists.keysScratchOffset, valuesSeen = l.lists.valuesScratchOffset, splitSeen = l.splitOffset;
          }
    std::printf("plan %u %u %u %u %u %llu %llu %llu\n", cus, n, formSeen, spreadSeen, pieceSeen, splitSeen, scratchSeen, valuesSeen);
  }
  std::printf("balanced segmented plan: %llu cases, %d failures\n", cases, failures);
  return failures == 0 ? 0 : 1;
}
