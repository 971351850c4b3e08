// CPU-only check of the plan and the layout of the range sorts at every size (vrdx_plan.h, PlanRangeSort; vrdx_layout.h,
// MakeRangeSortLayout, RangeChunkKeys), compiled and run by tests/test_range_sort_plan.py (also under ASan + UBSan).
// usage: range_sort_plan_check <compute units> <n> ...
// For both rankings, keys-only and key+value, every range width 1 ... 31 (at bit 0 and at the top of the key) and every
// storage address modulo 128, at every size given:
//   up to 16384 elements, and for the full, the empty and invalid ranges at every size, the plan is PlanSortBits' plan field
//   for field and has no step of its own;
//   beyond, the chunked form: chunks of a multiple of 256 keys and at least 8192 that cover [0, n) exactly once, at most one
//   per CU and per 8192 keys; 3 P + 1 launches in the slots 2 + 3 p, 3 + 3 p, 4 + 3 p and 14 behind the fill in slot 1; the
//   table of counts and both scratch arrays inside the storage requirement, on 128-byte lines, behind one another;
//   the same formula under counts below the bound (what the kernels evaluate for an indirect call): the chunks cover [0, count)
//   exactly once with at most `grid` of them.
// Prints one line per size: `plan <cus> <n> <grid> <chunkKeys>` (0 0: not chunked), then the number of cases and failures.
// Nothing of HIP is linked (vrdx_kernels.h needs one of its headers).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vulkan_radix_sort_amd/csrc/vrdx_plan.h"

namespace {

int failures = 0;
void Fail(const char* what, uint32_t n, int atomic, int keyValue, uint32_t b, uint32_t e, uint32_t address) {
  if (failures < 20)
    std::printf("FAIL %s: n=%u atomic=%d key+value=%d range=[%u,%u) address=%u\n", what, n, atomic, keyValue, b, e, address);
  ++failures;
}

bool SamePlan(const vrdx::SortPlan& x, const vrdx::SortPlan& y) {
  bool same = x.keyValue == y.keyValue && x.elementCount == y.elementCount && x.atomicRank == y.atomicRank &&
              x.oneWorkgroup == y.oneWorkgroup && x.hybridCap == y.hybridCap && x.msdBits == y.msdBits && x.msdCap == y.msdCap &&
              x.msdTileKeys == y.msdTileKeys && x.msdTiles == y.msdTiles && x.configIndex == y.configIndex &&
              x.blockSums == y.blockSums && x.fits == y.fits && x.refusal == y.refusal && x.stepCount == y.stepCount &&
              x.launches == y.launches && x.rangeBegin == y.rangeBegin && x.rangeWidth == y.rangeWidth && x.order == y.order &&
              x.tilePlan.tiles == y.tilePlan.tiles && x.tilePlan.slots == y.tilePlan.slots &&
              x.tilePlan.fullTiles == y.tilePlan.fullTiles && x.tilePlan.tailSlots == y.tilePlan.tailSlots &&
              x.tilePlan.blockSums == y.tilePlan.blockSums;
  // (the layout of a plan without steps is never filled in)
  if (same && x.stepCount != 0) same = std::memcmp(&x.layout, &y.layout, sizeof(x.layout)) == 0;
  for (uint32_t i = 0; same && i < x.stepCount; ++i)
    same = x.steps[i].what == y.steps[i].what && x.steps[i].pass == y.steps[i].pass && x.steps[i].slot == y.steps[i].slot &&
           x.steps[i].name == y.steps[i].name;
  return same;
}

// chunks of `keys` keys, `used` of them, cover [0, n) exactly once
bool Covers(uint32_t n, uint32_t keys, uint32_t used) {
  if (n == 0) return used == 0;
  return keys != 0 && keys % 256u == 0 && used >= 1 && (uint64_t)(used - 1) * keys < n && (uint64_t)used * keys >= n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int cus = std::atoi(argv[1]);
  std::vector<uint32_t> sizes;
  for (int i = 2; i < argc; ++i) sizes.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
  uint64_t cases = 0;
  for (uint32_t n : sizes) {
    uint32_t printedGrid = 0, printedKeys = 0;
    for (int atomic = 1; atomic >= 0; --atomic)
      for (int keyValue = 0; keyValue < 2; ++keyValue) {
        const bool kv = keyValue != 0;
        vrdx::PlanContext c;
        c.computeUnits = cus;
        c.atomicRank = atomic != 0;
        const vrdx::StorageLayout requirement = vrdx::MakeLayout(n, c.minStorageBufferOffsetAlignment, 0);
        for (uint32_t address = 0; address < 128; ++address) {
          // the full, the empty and two invalid ranges: PlanSortBits' plan, no step of its own
          const uint32_t others[4][2] = {{0, 32}, {7, 7}, {9, 8}, {0, 33}};
          for (const auto& r : others) {
            const vrdx::RangeSortPlan p = vrdx::PlanRangeSort(c, kv, n, r[0], r[1], address);
            const vrdx::SortPlan bits = vrdx::PlanSortBits(c, kv, n, r[0], r[1], address);
            ++cases;
            const vrdx::RangeSortForm form = bits.stepCount == 0 ? vrdx::RangeSortForm::kNone : vrdx::RangeSortForm::kWholeKey;
            if (!SamePlan(p.inner, bits) || p.stepCount != 0 || p.form != form || p.launches != bits.launches || p.refusal != nullptr)
              Fail("full, empty or invalid range", n, atomic, keyValue, r[0], r[1], address);
          }
          for (uint32_t width = 1; width <= 31; ++width)
            for (int top = 0; top < 2; ++top) {
              const uint32_t b = top ? 32 - width : 0, e = b + width;
              const vrdx::RangeSortPlan p = vrdx::PlanRangeSort(c, kv, n, b, e, address);
              ++cases;
              bool ok = p.keyValue == kv && p.elementCount == n && p.atomicRank == c.atomicRank && p.refusal == nullptr;
              VrdxHipRangeSortPlanInfo info = {};
              vrdx::DescribeRangeSortPlan(p, &info);
              if (n <= vrdx::kSmallSortMaxElements) {
                const vrdx::SortPlan bits = vrdx::PlanSortBits(c, kv, n, b, e, address);
                ok = ok && SamePlan(p.inner, bits) && p.stepCount == 0 && p.launches == bits.launches &&
                     p.form == (n == 0 ? vrdx::RangeSortForm::kNone : vrdx::RangeSortForm::kOneWorkgroup) &&
                     info.form == (uint32_t)p.form && info.launches == (n == 0 ? 0u : 1u) &&
                     info.digits == (n == 0 ? 0u : (width + 7) / 8) && info.bytesPerElementPerPass == (n == 0 ? 0u : kv ? 16u : 8u) &&
                     info.bytesPerElementCopyBack == 0;
                if (!ok) Fail("one-workgroup range plan", n, atomic, keyValue, b, e, address);
                continue;
              }
              const uint32_t P = (width + 7) / 8;
              ok = ok && p.form == vrdx::RangeSortForm::kChunked && p.inner.stepCount == 0 && p.rangeBegin == b &&
                   p.rangeWidth == width && p.digits == P;
              // chunks
              const uint32_t used = p.chunkKeys != 0 ? vrdx::RoundUp(n, p.chunkKeys) : 0;
              ok = ok && p.grid >= 1 && p.grid <= (uint32_t)cus && p.grid <= n / 8192u && p.chunkKeys >= 8192u &&
                   Covers(n, p.chunkKeys, used) && used <= p.grid && p.chunkKeys == vrdx::RangeChunkKeys(n, p.grid) &&
                   used == vrdx::RangeChunks(n, p.grid);
              // the same formula under a count below the bound, as the kernels evaluate it
              const uint32_t counts[] = {0, 1, 5, 255, 256, 257, 8191, 8192, 8193, 16384, 16385, n / 2, n - 1, n};
              for (uint32_t m : counts)
                ok = ok && Covers(m, vrdx::RangeChunkKeys(m, p.grid), vrdx::RangeChunks(m, p.grid)) &&
                     vrdx::RangeChunks(m, p.grid) <= p.grid;
              // steps
              ok = ok && p.launches == 3 * P + 1 && p.stepCount == 3 * P + 2 && p.steps[0].what == vrdx::StepRange::kFill &&
                   p.steps[0].slot == 1 && p.steps[p.stepCount - 1].what == vrdx::StepRange::kCopyBack &&
                   p.steps[p.stepCount - 1].slot == 14;
              for (uint32_t pass = 0; ok && pass < P; ++pass) {
                const vrdx::RangeSortStep* s = &p.steps[1 + 3 * pass];
                ok = s[0].what == vrdx::StepRange::kCount && s[0].slot == 2 + 3 * pass && s[0].pass == pass &&
                     s[1].what == vrdx::StepRange::kScan && s[1].slot == 3 + 3 * pass && s[1].pass == pass &&
                     s[2].what == vrdx::StepRange::kScatter && s[2].slot == 4 + 3 * pass && s[2].pass == pass &&
                     s[0].name != nullptr && s[1].name != nullptr && s[2].name != nullptr;
              }
              // layout: header and totals | counts | keys scratch | values scratch, inside the requirement
              const vrdx::RangeSortLayout& l = p.layout;
              const uint64_t bytes = 4ull * n;
              ok = ok && l.fits && l.totalsOffset == 16 && l.clearBytes == 16 + 4096 && l.countsOffset >= l.clearBytes &&
                   l.countsOffset < l.clearBytes + 128 && (address + l.countsOffset) % 128 == 0 &&
                   l.countsBytes == 1024ull * p.grid && l.keysScratchOffset >= l.countsOffset + l.countsBytes &&
                   l.keysScratchOffset < l.countsOffset + l.countsBytes + 128 && (address + l.keysScratchOffset) % 128 == 0 &&
                   l.keysScratchOffset + bytes <= requirement.keysOnlySize;
              if (kv)
                ok = ok && l.valuesScratchOffset >= l.keysScratchOffset + bytes && (address + l.valuesScratchOffset) % 128 == 0 &&
                     l.valuesScratchOffset + bytes <= requirement.keyValueSize;
              // the table takes at most half of the reference's partition-histogram area
              ok = ok && 2 * l.countsBytes <= 1024ull * vrdx::RoundUp(n, VRDX_REF_PARTITION_SIZE);
              ok = ok && info.form == VRDX_HIP_RANGE_SORT_CHUNKED && info.chunks == p.grid && info.keysPerChunk == p.chunkKeys &&
                   info.digits == P && info.launches == 3 * P + 1 && info.bytesPerElementPerPass == (kv ? 20u : 12u) &&
                   info.bytesPerElementCopyBack == (kv ? 16u : 8u);
              if (!ok) Fail("chunked range plan", n, atomic, keyValue, b, e, address);
              printedGrid = p.grid;
              printedKeys = p.chunkKeys;
            }
        }
      }
    std::printf("plan %d %u %u %u\n", cus, n, printedGrid, printedKeys);
  }
  std::printf("range sort plan: %llu cases, %d failures\n", (unsigned long long)cases, failures);
  return failures != 0;
}
