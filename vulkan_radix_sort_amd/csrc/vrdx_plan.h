// Everything the HOST decides about a sort, as plain functions of the element count, key+value or not, and a PlanContext
// (CU count, ranking mode, storage alignment, the planning knobs): the plan (one workgroup, eight-bit hybrid, MSD by 10 or
// 11 bits, four passes), the bucket capacity, the tile geometry and tile plan, block sums, the storage layout, the step
// list with its timestamp slots, the histogram grid and the fallback taken when a layout does not fit.  No HIP call, no
// environment, no static state: the recorder (vrdx_api.cpp) builds one PlanContext per recorded sort and calls PlanSort[Bits],
// PlanSegmentedSort or PlanSort64; tests/native/plan_check.cpp and layout_check.cpp call the same functions on a CPU.
#ifndef VRDX_PLAN_H
#define VRDX_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/vk_radix_sort.h"
#include "../../include/vk_radix_sort_balanced.h"
#include "vrdx_kernels.h"
#include "vrdx_layout.h"

namespace vrdx {

// What planning depends on besides the sort itself.  The knobs are those of the environment (vrdx_api.cpp, EnvKnobs;
// INTEGRATION.md) at their defaults.
struct PlanContext {
  int computeUnits = 0;
  bool atomicRank = false;  // the one-atomic ranking (LDS returning atomics proven lane-ordered), else the ballot ranking
  uint32_t minStorageBufferOffsetAlignment = VRDX_STORAGE_ALIGN;
  int forcedConfig = -1;    // VRDX_TILE_CONFIG: one geometry for everything, and the general path at every size
  bool hybrid = true;       // VRDX_HYBRID=0: always the four-pass plan
  bool msd = true;          // VRDX_MSD=0 (or VRDX_HYBRID=0): no MSD plan
  bool smallSort = true;    // VRDX_SMALL_SORT=0: always the general path
  bool blockSums = true;    // VRDX_BLOCK_SUMS=0: sorts of one round keep the classic look-back (measurements)
};

// "1024x32", or "1024x32x2" for the two-sub-tile kernel
static inline void ConfigName(const TileConfig& c, char* out, size_t size) {
  if (c.subTiles == 1)
    snprintf(out, size, "%dx%d", c.threads, c.keysPerThread);
  else
    snprintf(out, size, "%dx%dx%d", c.threads, c.keysPerThread, c.subTiles);
}

// Tile geometry by problem size, measured on MI355X (tools: `vrdx_selftest sweep`, tables in
// profiles/r01_sweep_*.txt).  Three regimes:
//  * small sorts want many small tiles (parallelism across the CUs; six launches cost ~45 us);
//  * beyond that throughput grows with the tile (fewer look-backs per key, longer digit runs) up to
//    the 32768 keys whose staging buffer fits the CU's LDS ONCE -- so these tiles run one workgroup
//    per CU in lock-step ROUNDS of computeUnits tiles, and a sort whose tile count is just above a
//    multiple of the CU count pays for a whole extra round.  f below is the size in such rounds.
//    (16384-key tiles, two workgroups per CU, degrade gracefully in a partial round and used to win
//    just past the round boundaries; on the final kernels they no longer do);
//  * the two-sub-tile kernel (65536 keys, keys-only) halves the rounds again: best when f is in
//    (1, 2], just below 4 or 6.
enum : int { kCfg1024x8 = 0, kCfg1024x16 = 1, kCfg1024x32 = 2, kCfg1024x32x2 = 3 };  // indices of kTileConfigs

// msd: the MSD plan is recorded in front of the passes, which are then only the fallback for skewed keys; its per-tile counts
// take a quarter to a half of the reference's partition-histogram area, so the passes must not take tiles of 16384.
constexpr int ConfigIndex(const PlanContext& c, bool keyValue, uint32_t elementCount, bool msd = false) {
  const int forced = c.forcedConfig;
  // (the two-sub-tile kernel is keys-only: a key+value sort under a forced 1024x32x2 takes 1024x32)
  if (forced >= 0) return forced == kCfg1024x32x2 && (keyValue || !c.atomicRank) ? kCfg1024x32 : forced;
  const double f = (double)elementCount / ((double)c.computeUnits * 32768.0);
  // Behind the MSD plan the passes are the fallback only, and the plan's own launches double as its first two (one kernel, two
  // roles): those kernels exist for 1024x32 key+value and the two-sub-tile geometry keys-only (the plan is recorded with the
  // one-atomic ranking only), which are then taken at every size -- keys-only at one round of tiles and below as even-split
  // tiles of two half-size sub-tiles.
  if (msd) return keyValue ? kCfg1024x32 : kCfg1024x32x2;
  if (keyValue) {
    if (f <= 0.26) return kCfg1024x8;
    if (f <= 0.53) return kCfg1024x16;
    // just past one round of 32768-element tiles, two workgroups of 16384 per CU fill the second round's gap
    // (1.2-2.6 % at 1.07 <= f <= 1.32, profiles/r03_sweep_by_geometry.txt; still so with the tail split of round 4,
    // profiles/r04_tail_split_kv.txt)
    if (f > 1.0 && f <= 1.35) return kCfg1024x16;
    return kCfg1024x32;
  }
  if (f <= 0.125) return kCfg1024x8;
  if (f <= 0.5) return kCfg1024x16;   // beyond: even-split 1024x32 tiles (PlanTiles), 7 % faster at f = 0.536
  if (f <= 1.0) return kCfg1024x32;
  // Beyond one round the two-sub-tile kernel (65536 keys per workgroup: half the look-backs per key), whose last,
  // partial round is cut into small equal tiles (tail split, PlanTiles): with that it is the fastest geometry at every
  // size from one round up (profiles/r04_tail_split_keys.txt; without it, it lost a whole 65536-key round to the
  // 1024x32 tiles whenever the tile count passed a multiple of the CU count -- f in (2, 3.3] and beyond 4 in round 3).
  // It holds two sub-tiles' keys in registers: only with the one-atomic ranking.
  return c.atomicRank ? kCfg1024x32x2 : kCfg1024x32;
}

// Mid-size sorts record the hybrid plan (vrdx_kernels.hip, PassPlan) next to the four passes: launch 0 scatters by the
// keys' highest byte that varies and bucket_sort_kernel finishes every bucket inside one workgroup -- if the DEVICE finds that no bucket
// exceeds the capacity returned here; otherwise the four passes run as usual and the bucket launch is empty.  The
// capacity is the smallest of 4096 / 8192 / 16384 / 32768 (the last one with the one-atomic ranking only) that leaves a
// bucket twice the room of its mean N / 256; the largest one is recorded as long as it leaves 3 % (a bucket sort
// costs what the bucket's elements cost, whatever the capacity; uniform keys spread by half a percent at these sizes --
// mean 31800, sigma 178 at 8.1 M: the capacity is 5 sigma away -- and a plan that does not apply costs one empty
// launch, 3 us, where one that does saves 17-25 %): N <= 8.1 M elements (4.0 M with the ballot ranking).
// 0 = the plan is not recorded (larger N, a forced tile geometry, VRDX_HYBRID=0).
constexpr uint32_t HybridCapacity(const PlanContext& c, uint32_t elementCount) {
  if (!c.hybrid || elementCount <= kSmallSortMaxElements) return 0;
  // a bucket may hold twice the mean bucket; the LARGEST capacity is tried with less room than the others (3 %): failing
  // costs one empty launch, the plan is worth a fifth to a third of the sort (profiles/r03_hybrid_headroom.txt)
  const uint64_t mean = (elementCount + VRDX_RADIX - 1) / VRDX_RADIX;
  const uint32_t need = (uint32_t)(mean * 200u / 100u);
  const uint32_t needLast = (uint32_t)(mean * 103u / 100u);
  // 32768-element buckets: the one-atomic ranking only (the ballot forms of that kernel would spill); key+value stages
  // keys and values through one buffer there (SharedStage in vrdx_kernels.hip)
  const uint32_t largest = c.atomicRank ? 32768u : 16384u;
  if (need <= 4096u) return 4096u;
  if (need <= 8192u) return 8192u;
  if (need <= 16384u) return 16384u;
  if (need <= largest) return largest;
  return needLast <= largest ? largest : 0u;
}

// The MSD plan (vrdx_kernels.hip, "MSD plan"): one stable scatter by the keys' top 10 or 11 bits, then every bucket by its
// remaining bits in two passes inside one workgroup -- three ranking steps and two trips through memory instead of four
// and four.  Recorded, in front of the four passes (which return on its verdict), for sorts beyond the eight-bit
// plan's reach whose mean bucket leaves 3 % of room in the bucket kernel's capacity (uniform keys spread by half a percent
// at these sizes): ten bits up to 36.6 M keys / 32.5 M pairs, eleven bits up to twice that.  Returns the bits or 0.
// One-atomic ranking only.  VRDX_MSD=0 switches it off (VRDX_HYBRID=0 and a forced tile geometry as well).
constexpr uint32_t MsdBits(const PlanContext& c, bool keyValue, uint32_t elementCount, uint32_t hybridCap, uint32_t* capacity) {
  if (!c.msd || !c.atomicRank) return 0;
  // From where the EIGHT-bit plan ends (8.1 M: hybridCap == 0), keys-only and key+value.  Up to 18.1 M elements the buckets
  // hold at most 18432 and the half-size bucket kernel sorts them, two workgroups to a CU: with it the plan is 8-15 % faster
  // than round 4's nine-bit hybrid plan and the four passes at one round of tiles, which key+value sorts of these sizes
  // took before (profiles/r05_msd_half_buckets.txt); that plan's kernels are gone since.
  if (hybridCap != 0 || elementCount <= kSmallSortMaxElements || RoundUp(elementCount, kMsdTileKeys) > kMsdMaxTiles) return 0;
  const uint32_t cap = keyValue ? kMsdCapKeyValue : kMsdCapKeys;
  *capacity = cap;
  for (uint32_t bits = 10; bits <= 11; ++bits) {
    const uint64_t mean = ((uint64_t)elementCount + (1u << bits) - 1u) >> bits;
    if (mean * 103u / 100u <= cap) {
      // buckets of half the size: the bucket kernel of 512 threads, two workgroups per CU (bucket_sort2_half_kernel)
      // (4 % of headroom here: 5.3 sigma of a uniform bucket of 17700; the 3 % of the full size would be 4 sigma at this
      // capacity, and with 1024 buckets one sort in thirty at the top of the range would be turned down)
      if (bits == 10 && mean * 104u / 100u <= kMsdHalfCap)
        *capacity = kMsdHalfCap;
      return bits;
    }
  }
  return 0;
}

// kMsdStreamedOutputUpTo (vrdx_kernels.h) quotes the rule above: the ten-bit plan's last size, keys-only and key+value.
constexpr uint32_t AdaptiveMsdBits(bool keyValue, uint32_t elementCount) {
  const PlanContext mi355x{256, true};
  uint32_t capacity = 0;
  return MsdBits(mi355x, keyValue, elementCount, HybridCapacity(mi355x, elementCount), &capacity);
}
static_assert(AdaptiveMsdBits(false, kMsdStreamedOutputUpTo) == 10 && AdaptiveMsdBits(false, kMsdStreamedOutputUpTo + 1) == 11 &&
                  AdaptiveMsdBits(true, kMsdStreamedOutputUpTo) == 10 && AdaptiveMsdBits(true, kMsdStreamedOutputUpTo + 1) == 11,
              "kMsdStreamedOutputUpTo is not the ten-bit MSD plan's last size");

// The tile plan of a sort (vrdx_layout.h, PlanTiles): even-split tiles for sorts of one round, tail-split tiles behind
// the whole rounds of a longer one -- where the kernels' forms with run-time slot counts exist and where they were
// measured to pay (profiles/r04_tail_split_keys.txt, r04_tail_split_kv.txt; f = size in rounds of CUs x 32768):
//   keys-only 1024x32x2   even split (-9.5 % at f = 1.07) and tail split at every size (f = 2.06: 0.191 instead of
//                         0.230 ms; 3.06: 0.261 / 0.272; 4.06: 0.340 / 0.388)
//   keys-only 1024x32     even split (-3.5 % at f = 0.5); NO tail split (+0 ... +4 %: these tiles are short enough that
//                         a few of them in a last round cost what 256 small ones cost)
//   key+value 1024x32     NO even split (its split form fetches the values late, vrdx_kernels.hip: +2 ... +7 % at
//                         0.55 < f < 1); tail split while the rest is at most half a round (f = 1.06: 0.184 / 0.193 ms,
//                         2.06: 0.294 / 0.303, 3.06: 0.399 / 0.408, 4.06: 0.524 / 0.532; beyond half a round -1 ... +4 %)
static inline TilePlan PlanTiles(const PlanContext& c, int configIndex, bool keyValue, uint32_t elementCount) {
  const TileConfig& t = kTileConfigs[configIndex];
  const bool pair = configIndex == kCfg1024x32x2;
  const bool splitForms = pair ? (!keyValue && c.atomicRank) : configIndex == kCfg1024x32;
  const bool evenSplit = !keyValue;
  const uint32_t tailPercent = pair ? 100u : (keyValue ? 50u : 0u);
  return PlanTiles(elementCount, (uint32_t)c.computeUnits, (uint32_t)t.threads, (uint32_t)t.keysPerThread, (uint32_t)t.subTiles,
                   splitForms, evenSplit, tailPercent);
}

// The steps of a sort in the order they are enqueued, each with the timestamp slot it ends.  The slots carry the
// reference's names (include/vk_radix_sort.h): 0 start, 1 "transfer", 2 + 3 p "upsweep" / 3 + 3 p "spine" / 4 + 3 p
// "downsweep" of pass p, 14 end; a slot no step ends coincides with the one before it (StampCursor in vrdx_api.cpp).
enum class Step : uint8_t {
  kFill,               // slot 1: state fill, and the copy of an indirect count (not counted as a launch)
  kHistogram,          // slot 2, pass 0's "upsweep": the fused histogram of all four passes
  kHistogramMsd,       // slot 2: the MSD plan's form of it
  kSpineMsd,           // slot 3: a real "spine"
  kMsdScatterOrPass0,  // slot 4, pass 0's "downsweep": the MSD plan's scatter, whose second role is pass 0
  kMsdBucketsOrPass1,  // slot 5, pass 1's "upsweep": the MSD plan's full-size buckets, whose second role is pass 1
  kBucketSortHalf,     // slot 5: its half-size buckets
  kBucketSort,         // slot 5: the eight-bit plan's buckets
  kPass,               // slot 4 + 3 p, "downsweep": pass p, look-back fused into it ("spine" = "upsweep" = the slot before)
  kSmallSort,          // slot 14: the one-workgroup sort
  kSmallSortBits,      // slot 14: the one-workgroup sort by the digits of a bit range (PlanSortBits)
  // a key order of the 32-bit sorts (PlanOrderedSort)
  kSmallSortOrdered,   // slot 14: the one-workgroup sort by T(key)
  kOrderForward,       // slot 1, in front of the fill (which ends the same slot): keys -> T(key), in place
  kOrderInverse,       // slot 14, behind pass 3 (slot 13): T(key) -> keys, in place
};
struct SortStep { Step what; uint8_t pass, slot; const char* name; };  // (pass: kPass only; name: what EnqueueCheck reports)
constexpr uint32_t kMaxSortSteps = 10;  // fill, histogram, spine, scatter, half-size buckets, passes 1-3; the two transforms

// Everything the host decides about a sort, in ONE place: RecordSort records it and vrdxHipDescribePlan reports it.
// storageAddress: the absolute address the storage is handed over at -- only its low seven bits matter (the pads in front
// of the 128-byte aligned regions); 0 is the worst case for what fits, which is what vrdxHipDescribePlan assumes.
struct SortPlan {
  bool keyValue = false;
  uint32_t elementCount = 0;
  bool atomicRank = false;
  bool oneWorkgroup = false;    // small_sort_kernel: one launch, no storage layout
  uint32_t hybridCap = 0;       // the eight-bit hybrid plan is recorded with this bucket capacity
  uint32_t msdBits = 0;         // the MSD plan is recorded in front of the passes (10 | 11)
  uint32_t msdCap = 0;          // kMsdHalfCap: bucket_sort2_half_kernel, and pass 1 a launch of its own
  uint32_t msdTileKeys = 0;
  uint32_t msdTiles = 0;
  int configIndex = 0;
  TilePlan tilePlan{};
  bool blockSums = false;
  bool fits = true;             // false: not even tiles of full capacity fit the caller's storage (refused)
  const char* refusal = nullptr;  // fits == false: why, as EnqueueCheck reports it
  StorageLayout layout{};
  SortStep steps[kMaxSortSteps];  // none: the empty sort and the refused one
  uint32_t stepCount = 0;
  uint32_t launches = 0;        // kernels among the steps
  // a bit-range sort (PlanSortBits): by the rangeWidth bits (1 ... 31) of the key from bit rangeBegin; 0: the whole key
  uint32_t rangeBegin = 0, rangeWidth = 0;
  // an ordered sort (PlanOrderedSort): the order word (vrdx_kernels.h); kKeyOrderUint32: the whole key as it stands
  uint32_t order = kKeyOrderUint32;
};

// The MSD plan's scatter launch is ALSO pass 0 of the fallback and its bucket launch pass 1 (one branch on the verdict, on
// the device; vrdx_kernels.hip, msd_scatter_or_pass0_kernel): only passes 2 and 3 remain as launches that return when the
// plan runs.  With buckets of the half-size kernel (512 threads; the passes' bodies need 1024) only the scatter launch has
// a second role.  The eight-bit plan's bucket sort sits between launch 0 and launch 1 (which is empty when the plan applies).
static inline void ListSteps(SortPlan& p) {
  const auto add = [&p](Step what, const char* name, uint32_t slot, uint32_t pass = 0) {
    p.steps[p.stepCount++] = SortStep{what, (uint8_t)pass, (uint8_t)slot, name};
    if (what != Step::kFill) ++p.launches;
  };
  const bool msd = p.msdBits != 0, halfBuckets = msd && p.msdCap == kMsdHalfCap;
  const bool ordered = p.order != kKeyOrderUint32;
  if (p.oneWorkgroup && p.rangeWidth != 0) return add(Step::kSmallSortBits, "small_sort_bits_kernel", 14);
  if (p.oneWorkgroup && ordered) return add(Step::kSmallSortOrdered, "small_sort_ordered_kernel", 14);
  if (p.oneWorkgroup) return add(Step::kSmallSort, "small_sort_kernel", 14);
  // an ordered sort beyond one workgroup: the plan below, unchanged, on T(key) -- one streaming launch in front of it and
  // one behind it, both in place on the caller's keys
  if (ordered) add(Step::kOrderForward, "order32_kernel", 1);
  add(Step::kFill, "hipMemcpyAsync(count)", 1);
  if (msd)
    add(Step::kHistogramMsd, "histogram_msd_kernel", 2);
  else
    add(Step::kHistogram, "histogram_kernel", 2);
  if (msd) {
    add(Step::kSpineMsd, "spine_msd_kernel", 3);
    add(Step::kMsdScatterOrPass0, "msd_scatter_or_pass0_kernel", 4);
    if (halfBuckets)
      add(Step::kBucketSortHalf, "bucket_sort2_half_kernel", 5);
    else
      add(Step::kMsdBucketsOrPass1, "msd_buckets_or_pass1_kernel", 5);
  }
  for (uint32_t pass = !msd ? 0u : halfBuckets ? 1u : 2u; pass < VRDX_PASSES; ++pass) {
    if (pass == 1 && p.hybridCap != 0) add(Step::kBucketSort, "bucket_sort_kernel", 5);
    add(Step::kPass, "onesweep_kernel", 4 + 3 * pass, pass);
  }
  if (ordered) add(Step::kOrderInverse, "order32_kernel", 14);
}

static inline SortPlan PlanSort(const PlanContext& c, bool keyValue, uint32_t elementCount, uint64_t storageAddress) {
  SortPlan p;
  p.keyValue = keyValue;
  p.elementCount = elementCount;
  p.atomicRank = c.atomicRank;  // one answer for the whole sort
  const bool adaptive = c.forcedConfig < 0;
  if (elementCount == 0) return p;
  // Small sorts: one workgroup, one launch, nothing but the caller's keys / values and words 1-3 of the storage header
  // touched -- the kernel zeroes the plan's verdict, the MSD plan's word and the failure word, so that the verdict an
  // earlier sort left on this storage is not read as this one's (the general path costs six launches = 30-45 us however
  // small N is).  Forcing a tile geometry (VRDX_TILE_CONFIG) also forces the general path, which is how the tests reach
  // it at small sizes.
  if (elementCount <= kSmallSortMaxElements && adaptive && c.smallSort) {
    p.oneWorkgroup = true;
    p.layout = MakeLayout(elementCount, c.minStorageBufferOffsetAlignment, 0, storageAddress);  // (the failure word)
    ListSteps(p);
    return p;
  }
  p.hybridCap = adaptive ? HybridCapacity(c, elementCount) : 0u;
  p.msdBits = adaptive ? MsdBits(c, keyValue, elementCount, p.hybridCap, &p.msdCap) : 0u;
  p.configIndex = ConfigIndex(c, keyValue, elementCount, p.msdBits != 0);
  p.tilePlan = PlanTiles(c, p.configIndex, keyValue, elementCount);
  // Block sums instead of the look-back chain: sorts of one round (PlanTiles) on the four-pass plan -- with a hybrid
  // plan recorded, launch 0 may rank by another byte than its pass index, which the block-sum form does not look up.
  p.blockSums = p.tilePlan.blockSums && p.hybridCap == 0 && c.blockSums;
  // keys per tile of the MSD plan's histogram and scatter: equal tiles that fill whole rounds of one workgroup per CU
  // (vrdx_layout.h); keys-only sorts by ten bits take two consecutive tiles per scatter workgroup (vrdx_kernels.hip)
  p.msdTileKeys = MsdTileKeysFor(elementCount, (uint32_t)c.computeUnits, kMsdMaxTiles, !keyValue && p.msdBits == 10);
  p.msdTiles = RoundUp(elementCount, p.msdTileKeys);
  const uint32_t align = c.minStorageBufferOffsetAlignment;
  p.layout = MakeLayout(elementCount, align, p.tilePlan.tiles, storageAddress, p.blockSums, p.msdBits, p.msdTiles);
  if (p.msdBits != 0 && !LayoutFits(p.layout, elementCount)) {
    // (never taken for the sizes MsdBits admits -- tests/native/layout_check.cpp asserts it on this very function, at every
    // size it sweeps -- but the storage is the caller's: without the plan's rows in front of the status regions the layout
    // fits for every N)
    p.msdBits = 0;
    p.layout = MakeLayout(elementCount, align, p.tilePlan.tiles, storageAddress, p.blockSums);
  }
  if (!LayoutFits(p.layout, elementCount)) {
    // EVERY sort of the general path is checked, not only those with a plan in front: the layout depends on the tile plan,
    // and a forced tile geometry (VRDX_TILE_CONFIG) can select plans the sweep of tests/native/layout_check.cpp (adaptive
    // plans only) never saw.  Tiles of the kernel's full capacity without block rows fit for every N (2 (tiles - 1) KiB <=
    // (P - 1) KiB from 8192 keys per tile up); smaller tiles cannot be helped: the scratch arrays must not leave the caller's
    // allocation, so that sort is refused and says so (VRDX_HIP_STATUS_ENQUEUE_REFUSED).
    const TileConfig& t = kTileConfigs[p.configIndex];
    p.tilePlan = PlanTiles(elementCount, (uint32_t)c.computeUnits, (uint32_t)t.threads, (uint32_t)t.keysPerThread,
                           (uint32_t)t.subTiles, false, false, 0);
    p.blockSums = false;
    p.msdBits = 0;
    p.layout = MakeLayout(elementCount, align, p.tilePlan.tiles, storageAddress, false, 0);
    p.fits = LayoutFits(p.layout, elementCount);
    if (!p.fits) p.refusal = "storage layout (status rows do not fit the reference's partition-histogram area)";
  }
  if (p.fits) ListSteps(p);
  return p;
}

// The plan of a bit-range sort (vrdxHipCmdSortBits; include/vk_radix_sort.h) by the bits [beginBit, endBit) of the key: one
// workgroup ranking ceil((endBit - beginBit) / 8) digits in one launch -- up to kSmallSortMaxElements elements, whatever
// PlanContext::smallSort and forcedConfig say.  Larger range sorts are NOT built: the plan then has
// no step and fits == false, and the recorder refuses the call like a layout that does not fit.
// The range of all 32 bits is PlanSort itself, knobs and all; an empty range has no step, like an empty sort; an invalid one (beginBit >
// endBit, endBit > 32) has none either and is refused.
constexpr const char* kBitRangeRefused = "bit range (0 <= beginBit <= endBit <= 32)";
static inline SortPlan PlanSortBits(const PlanContext& c, bool keyValue, uint32_t elementCount, uint32_t beginBit, uint32_t endBit,
                                    uint64_t storageAddress) {
  if (beginBit == 0 && endBit == 32) return PlanSort(c, keyValue, elementCount, storageAddress);
  SortPlan p;
  p.keyValue = keyValue;
  p.elementCount = elementCount;
  p.atomicRank = c.atomicRank;
  p.fits = beginBit <= endBit && endBit <= 32;
  if (!p.fits) p.refusal = kBitRangeRefused;
  if (!p.fits || beginBit == endBit || elementCount == 0) return p;
  if (elementCount > kSmallSortMaxElements) {
    p.fits = false;  // beyond one workgroup: not built
    p.refusal = "bit range over more than 16384 elements (not built)";
    return p;
  }
  // By size alone: a range sort has no general-path form that VRDX_SMALL_SORT=0 or VRDX_TILE_CONFIG could select, so the plan
  // is the one-workgroup plan PlanSort records with those two knobs at their defaults.
  PlanContext sizeOnly = c;
  sizeOnly.smallSort = true;
  sizeOnly.forcedConfig = -1;
  p = PlanSort(sizeOnly, keyValue, elementCount, storageAddress);
  p.rangeBegin = beginBit;
  p.rangeWidth = endBit - beginBit;  // 1 ... 31: the kernel extracts with v_bfe_u32, which takes a width modulo 32
  p.stepCount = p.launches = 0;
  ListSteps(p);
  return p;
}

// The plan of a range sort at every size (vrdxHipCmdRangeSort[KeyValue][Indirect]; include/vk_radix_sort.h).  Up to
// kSmallSortMaxElements elements, and for the full, the empty and an invalid range, it IS PlanSortBits' plan (`inner`, which the
// recorder hands to the recorder of vrdxHipCmdSortBits*: the same launches, the same slots).  Beyond that, where PlanSortBits
// refuses, the chunked form (vrdx_kernels.hip, "range sort") with a step list of its own -- SortPlan
// and kMaxSortSteps stay what they are:
//   fill (header and totals; an indirect count is copied)                        slot 1
//   digit p = 0 ... P - 1, P = ceil(width / 8):  range_count_kernel              slot 2 + 3 p
//                                                 range_scan_kernel               slot 3 + 3 p
//                                                 range_scatter_kernel            slot 4 + 3 p
//   range_copy_back_kernel                                                        slot 14
// 3 P + 1 launches, known from the range alone; which passes are active and whether the copy back copies is decided on the
// device.  `grid` workgroups take the chunks of RangeChunkKeys (vrdx_layout.h), sized from elementCount -- the bound of an
// indirect call.  Like PlanSortBits the chunked form is chosen by size alone: no planning knob selects anything in it.
enum class RangeSortForm : uint8_t { kNone, kOneWorkgroup, kWholeKey, kChunked };  // VRDX_HIP_RANGE_SORT_*
enum class StepRange : uint8_t { kFill, kCount, kScan, kScatter, kCopyBack };
struct RangeSortStep { StepRange what; uint8_t pass, slot; const char* name; };
constexpr uint32_t kMaxRangeSortSteps = 2 + 3 * VRDX_PASSES;
struct RangeSortPlan {
  RangeSortForm form = RangeSortForm::kNone;
  SortPlan inner{};               // every form but kChunked: PlanSortBits' plan, refusal included
  bool keyValue = false;
  uint32_t elementCount = 0;
  bool atomicRank = false;
  uint32_t rangeBegin = 0, rangeWidth = 0;
  // kChunked only
  uint32_t digits = 0;            // P
  uint32_t grid = 0;              // chunks = workgroups of the count and scatter launches
  uint32_t chunkKeys = 0;         // keys per chunk for elementCount itself (an indirect count: RangeChunkKeys on the device)
  RangeSortLayout layout{};
  const char* refusal = nullptr;  // the layout does not fit (cannot happen: see MakeRangeSortLayout)
  RangeSortStep steps[kMaxRangeSortSteps];
  uint32_t stepCount = 0;
  uint32_t launches = 0;          // kernels among the steps
};

static inline RangeSortPlan PlanRangeSort(const PlanContext& c, bool keyValue, uint32_t elementCount, uint32_t beginBit,
                                          uint32_t endBit, uint64_t storageAddress) {
  RangeSortPlan p;
  p.keyValue = keyValue;
  p.elementCount = elementCount;
  p.atomicRank = c.atomicRank;
  const bool valid = beginBit <= endBit && endBit <= 32;
  const bool partial = valid && beginBit != endBit && endBit - beginBit != 32;
  if (!partial || elementCount <= kSmallSortMaxElements) {
    p.inner = PlanSortBits(c, keyValue, elementCount, beginBit, endBit, storageAddress);
    p.rangeBegin = p.inner.rangeBegin;
    p.rangeWidth = p.inner.rangeWidth;
    p.launches = p.inner.launches;
    p.form = p.inner.stepCount == 0 ? RangeSortForm::kNone
             : partial              ? RangeSortForm::kOneWorkgroup
                                    : RangeSortForm::kWholeKey;
    return p;
  }
  p.form = RangeSortForm::kChunked;
  p.rangeBegin = beginBit;
  p.rangeWidth = endBit - beginBit;  // 1 ... 31
  p.digits = (p.rangeWidth + 7u) / 8u;
  p.grid = RangeSortGrid(elementCount, (uint32_t)c.computeUnits);
  p.chunkKeys = RangeChunkKeys(elementCount, p.grid);
  p.layout = MakeRangeSortLayout(elementCount, c.minStorageBufferOffsetAlignment, p.grid, keyValue, storageAddress);
  if (!p.layout.fits) {
    p.form = RangeSortForm::kNone;
    p.refusal = "range sort storage layout";
    return p;
  }
  const auto add = [&p](StepRange what, const char* name, uint32_t slot, uint32_t pass = 0) {
    p.steps[p.stepCount++] = RangeSortStep{what, (uint8_t)pass, (uint8_t)slot, name};
    if (what != StepRange::kFill) ++p.launches;
  };
  add(StepRange::kFill, "hipMemcpyAsync(count)", 1);
  for (uint32_t pass = 0; pass < p.digits; ++pass) {
    add(StepRange::kCount, "range_count_kernel", 2 + 3 * pass, pass);
    add(StepRange::kScan, "range_scan_kernel", 3 + 3 * pass, pass);
    add(StepRange::kScatter, "range_scatter_kernel", 4 + 3 * pass, pass);
  }
  add(StepRange::kCopyBack, "range_copy_back_kernel", 14);
  return p;
}

// The plan of an ordered 32-bit sort (vrdxHipCmdOrderedSort[KeyValue][Indirect]; include/vk_radix_sort.h) in the order of the
// word `order` (vrdx_kernels.h, kKeyOrder*): kKeyOrderUint32 is PlanSort itself; an invalid word has no step and is refused.
// Otherwise the plan is PlanSort's with its steps listed again: one workgroup runs small_sort_ordered_kernel, and beyond that
// the same steps -- MSD, hybrid or four passes, verdict and fallback on the device as ever -- sort T(key) between the two
// transform steps.  An empty sort and one PlanSort refuses stay what they are: no step, no transform.
constexpr const char* kKeyOrderRefused = "key order (a key type 0 ... 2, VRDX_HIP_ORDER_DESCENDING or not)";
static inline SortPlan PlanOrderedSort(const PlanContext& c, bool keyValue, uint32_t elementCount, uint32_t order,
                                       uint64_t storageAddress) {
  if (order == kKeyOrderUint32) return PlanSort(c, keyValue, elementCount, storageAddress);
  if (!KeyOrderValid(order)) {
    SortPlan p;
    p.keyValue = keyValue;
    p.elementCount = elementCount;
    p.atomicRank = c.atomicRank;
    p.fits = false;
    p.refusal = kKeyOrderRefused;
    return p;
  }
  SortPlan p = PlanSort(c, keyValue, elementCount, storageAddress);
  if (p.stepCount == 0) return p;
  p.order = order;
  p.stepCount = p.launches = 0;
  ListSteps(p);
  return p;
}

// ---- the segmented sorts (vrdxHipCmdSortSegmented*; include/vk_radix_sort.h) ----
// How a segmented sort orders its keys.  4-byte keys: by the bits [beginBit, endBit) -- the full range is the whole key, an
// empty one orders by nothing (no step), an invalid one is refused; with the full range also by an order word
// (vrdxHipCmdOrderedSortSegmented*: kKeyOrderUint32 is the whole key as it stands, an invalid word is refused, and a word
// combined with a partial range is not built and refused).  8-byte keys: by the order word (vrdx_kernels.h,
// kKeyOrder*; kKeyOrderUint64 is the whole key as it stands, an invalid word is refused); the range is not looked at.
struct SegmentedKey {
  uint32_t beginBit = 0, endBit = 32;
  uint32_t order = kKeyOrderUint64;
};

// The steps of a segmented sort: a fill of the header and the two list counters (a one-wave kernel, not a memset), then three
// launches whose work is decided on the device from the offsets -- the 256-thread in-LDS form over every segment (it also
// lists the bigger ones), the 1024-thread in-LDS form over the mid list, one workgroup per large segment.  A launch whose
// grid would be 0 is absent (no segment can be that large under this bound); its slot coincides with the one before.
enum class SegmentedStep : uint8_t { kClear, kSmall, kMid, kLarge };  // slots 1 ... 4; kSmall + c = SegmentClass c
struct SegmentedSortStep { SegmentedStep what; uint8_t slot; const char* name; uint32_t grid; };

// Everything the host decides about a segmented sort.  Grids depend on segmentCount, maxElementCount and the CU count only,
// so a captured call can be replayed on any segmentation with the same segmentCount.
struct SegmentedPlan {
  bool keyValue = false;
  bool atomicRank = false;
  const char* refusal = nullptr;           // non-null: refused (no step), and why
  uint32_t rangeBegin = 0, rangeWidth = 0;  // 4-byte keys by a bit range: width 1 ... 31; 0: the whole key
  uint32_t order = kKeyOrderUint64;        // 8-byte keys, and 4-byte keys by the whole key
  SegmentedLayout layout{};
  SegmentedSortStep steps[4];              // none: refused, or empty (no elements, no segments, an empty range)
  uint32_t stepCount = 0;
};

static inline SegmentedPlan PlanSegmentedSort(const PlanContext& c, uint32_t keyBytes, bool keyValue, uint32_t maxElementCount,
                                              uint32_t segmentCount, const SegmentedKey& key, uint64_t storageAddress) {
  static constexpr const char* kNames[5][4] = {
      {"segmented_clear_kernel", "segmented_small_kernel", "segmented_mid_kernel", "segmented_large_kernel"},
      {"segmented_clear_kernel", "segmented_small_bits_kernel", "segmented_mid_bits_kernel", "segmented_large_bits_kernel"},
      {"segmented_clear_kernel", "segmented_small64_kernel", "segmented_mid64_kernel", "segmented_large64_kernel"},
      {"segmented_clear_kernel", "segmented_small64_ordered_kernel", "segmented_mid64_ordered_kernel", "segmented_large64_ordered_kernel"},
      {"segmented_clear_kernel", "segmented_small_ordered_kernel", "segmented_mid_ordered_kernel", "segmented_large_ordered_kernel"}};
  const bool wide = keyBytes == 8;
  SegmentedPlan p;
  p.keyValue = keyValue;
  p.atomicRank = c.atomicRank;  // one answer for the whole sort
  if (wide ? !KeyOrderValid(key.order) : key.beginBit > key.endBit || key.endBit > 32) {
    p.refusal = wide ? kKeyOrderRefused : kBitRangeRefused;
    return p;
  }
  if (!wide && key.order != kKeyOrderUint32) {
    if (!KeyOrderValid(key.order)) p.refusal = kKeyOrderRefused;
    else if (key.endBit - key.beginBit != 32) p.refusal = "key order combined with a bit range (not built)";
    if (p.refusal != nullptr) return p;
  }
  if (!wide && key.beginBit == key.endBit) return p;  // nothing to order by
  p.order = key.order;
  if (!wide && key.endBit - key.beginBit < 32) p.rangeBegin = key.beginBit, p.rangeWidth = key.endBit - key.beginBit;
  const uint32_t align = c.minStorageBufferOffsetAlignment;
  p.layout = wide ? MakeSegmented64Layout(maxElementCount, align, keyValue, storageAddress)
                  : MakeSegmentedLayout(maxElementCount, align, keyValue, storageAddress);
  if (segmentCount == 0 || maxElementCount == 0) return p;
  if (!p.layout.fits) {  // (cannot happen for N >= 1: both layouts fit every count)
    p.refusal = wide ? "segmented 64-bit storage layout" : "segmented storage layout";
    return p;
  }
  // one workgroup per segment up to 2^20 of them (a grid-stride loop beyond); the other two launches take their lists by grid
  // stride with at most as many workgroups as can be resident: two per CU of the 4-byte forms, one of the 8-byte forms (their
  // 1024-thread kernels take 66 to 89 registers and 90 to 144 KiB of LDS)
  const uint32_t resident = (wide ? 1u : 2u) * (uint32_t)c.computeUnits;
  const uint32_t grids[4] = {1u, std::min<uint32_t>(segmentCount, 1u << 20),
                             std::min<uint32_t>(std::min<uint32_t>(segmentCount, p.layout.midCap), resident),
                             std::min<uint32_t>(std::min<uint32_t>(segmentCount, p.layout.largeCap), resident)};
  const char* const* names = kNames[wide ? (p.order != kKeyOrderUint64 ? 3 : 2) : p.order != kKeyOrderUint32 ? 4 : (p.rangeWidth != 0 ? 1 : 0)];
  for (uint32_t i = 0; i < 4; ++i)
    if (grids[i] != 0) p.steps[p.stepCount++] = SegmentedSortStep{SegmentedStep(i), (uint8_t)(i + 1), names[i], grids[i]};
  return p;
}

// ---- the balanced segmented sort (vrdxHipCmdBalancedSortSegmented[KeyValue]; include/vk_radix_sort.h) ----
// Up to kSegSpreadFrom elements -- and where the CU count admits no spread segment -- no segment can be spread and the plan IS
// PlanSegmentedSort's (`twin`, which the recorder hands to the recorder of vrdxHipCmdSortSegmented*: the same launches, the same
// slots).  Beyond that a step list of its own on the storage of MakeBalancedSegmentedLayout (vrdx_kernels.hip, "balanced
// segmented sort") -- SegmentedPlan stays what it is:
//   segmented_clear_kernel                                              slot 1
//   segmented_small_kernel                                              slot 2
//   segmented_mid_kernel                                                slot 3
//   segmented_split_kernel, segmented_large_kernel on the rest list     slot 4
//   byte p = 0 ... 3:  segmented_piece_count_kernel, _scan_kernel       slot 5 + 2 p
//                      segmented_piece_scatter_kernel                   slot 6 + 2 p
//   segmented_piece_copy_back_kernel                                    slot 13 (slot 14 coincides)
// 18 launches, known from the bound alone; which segments are spread, which passes are active and whether the copy back copies
// is decided on the device.  Grids depend on segmentCount, maxElementCount and the CU count only, so a captured call replays
// on any segmentation with the same segmentCount.  Chosen by size alone: no planning knob selects anything in it.
enum class BalancedForm : uint8_t { kNone, kTwin, kBalanced };  // VRDX_HIP_BALANCED_*
enum class StepBalanced : uint8_t { kClear, kSmall, kMid, kSplit, kLargeRest, kCount, kScan, kScatter, kCopyBack };
struct BalancedSegmentedStep { StepBalanced what; uint8_t pass, slot; const char* name; uint32_t grid; };
constexpr uint32_t kMaxBalancedSteps = 6 + 3 * VRDX_PASSES;
struct BalancedSegmentedPlan {
  BalancedForm form = BalancedForm::kNone;
  SegmentedPlan twin{};             // every form but kBalanced: PlanSegmentedSort's plan
  bool keyValue = false;
  bool atomicRank = false;
  uint32_t computeUnits = 0;
  const char* refusal = nullptr;    // the layout does not fit (cannot happen: see MakeBalancedSegmentedLayout)
  BalancedSegmentedLayout layout{};  // kBalanced only
  BalancedSegmentedStep steps[kMaxBalancedSteps];
  uint32_t stepCount = 0;
  uint32_t launches = 0;            // kernels among the steps (the fill is one)
};

static inline BalancedSegmentedPlan PlanBalancedSegmentedSort(const PlanContext& c, bool keyValue, uint32_t maxElementCount,
                                                              uint32_t segmentCount, uint64_t storageAddress) {
  BalancedSegmentedPlan p;
  p.keyValue = keyValue;
  p.atomicRank = c.atomicRank;
  p.computeUnits = (uint32_t)c.computeUnits;
  if (maxElementCount <= kSegSpreadFrom || segmentCount == 0 || SegSpreadCap(maxElementCount, p.computeUnits) == 0) {
    p.twin = PlanSegmentedSort(c, 4, keyValue, maxElementCount, segmentCount, SegmentedKey{}, storageAddress);
    p.refusal = p.twin.refusal;
    p.launches = p.twin.stepCount;
    p.form = p.twin.stepCount != 0 ? BalancedForm::kTwin : BalancedForm::kNone;
    return p;
  }
  p.layout = MakeBalancedSegmentedLayout(maxElementCount, c.minStorageBufferOffsetAlignment, p.computeUnits, keyValue, storageAddress);
  if (!p.layout.lists.fits) {
    p.refusal = "balanced segmented storage layout";
    return p;
  }
  p.form = BalancedForm::kBalanced;
  const auto add = [&p](StepBalanced what, const char* name, uint32_t slot, uint32_t grid, uint32_t pass = 0) {
    p.steps[p.stepCount++] = BalancedSegmentedStep{what, (uint8_t)pass, (uint8_t)slot, name, grid};
    ++p.launches;
  };
  // the twin's grids (PlanSegmentedSort): beyond kSegSpreadFrom elements both lists hold a segment at least, so none is 0
  const uint32_t resident = 2u * p.computeUnits;
  const SegmentedLayout& s = p.layout.lists;
  add(StepBalanced::kClear, "segmented_clear_kernel", 1, 1u);
  add(StepBalanced::kSmall, "segmented_small_kernel", 2, std::min<uint32_t>(segmentCount, 1u << 20));
  add(StepBalanced::kMid, "segmented_mid_kernel", 3, std::min<uint32_t>(std::min<uint32_t>(segmentCount, s.midCap), resident));
  add(StepBalanced::kSplit, "segmented_split_kernel", 4, 1u);
  add(StepBalanced::kLargeRest, "segmented_large_kernel", 4, std::min<uint32_t>(std::min<uint32_t>(segmentCount, s.largeCap), resident));
  for (uint32_t pass = 0; pass < VRDX_PASSES; ++pass) {
    add(StepBalanced::kCount, "segmented_piece_count_kernel", 5 + 2 * pass, p.layout.pieceCap, pass);
    add(StepBalanced::kScan, "segmented_piece_scan_kernel", 5 + 2 * pass, p.layout.spreadCap, pass);
    add(StepBalanced::kScatter, "segmented_piece_scatter_kernel", 6 + 2 * pass, p.layout.pieceCap, pass);
  }
  add(StepBalanced::kCopyBack, "segmented_piece_copy_back_kernel", 13, p.layout.pieceCap);
  return p;
}

// ---- the 64-bit sorts (vrdxHipCmdSort64[Ordered][KeyValue][Indirect]) ----
// Two stable 32-bit key+value sorts, low words first and high words second, on word arrays inside the storage (vrdx_layout.h,
// MakeSort64Layout), with the streaming kernels of vrdx_kernels.hip ("64-bit keys") around them:
//   keys-only   split (A = lo, B = hi) | sort (A, B) | sort (B, A) | merge (keys = B << 32 | A)
//   key+value   split (A = lo, I = iota) | sort (A, I) | gather (A = hi of keys[I]) | sort (A, I) |
//               permute (T = A << 32 | lo of keys[I], A = values[I]) | copy back (keys = T, values = A)
// Each step ends one slot; keys-only, slot 3 coincides with slot 2 (no step between the sorts).  With an order word other than
// kKeyOrderUint64 the split, the gather, the permutation and the merge are their ordered forms -- A, B hold the words of T(key)
// (vrdx_kernels.h), so the inner sorts and the copy back are the same.  Nothing is decided from the data, and an indirect
// call is planned from its bound alone.
enum class Step64 : uint8_t { kSplit, kSortLoOther, kSortOtherLo, kGatherHi, kPermute, kCopyBack, kMerge };
struct Sort64Step { Step64 what; uint8_t slot; const char* name; };  // (name: what EnqueueCheck reports; an inner sort reports its own)
struct Sort64Plan {
  bool keyValue = false;
  uint32_t elementCount = 0;
  uint32_t order = kKeyOrderUint64;
  const char* refusal = nullptr;  // non-null: refused (an invalid order word), no step
  Sort64Layout layout{};
  Sort64Step steps[6];            // none: refused, or the empty sort
  uint32_t stepCount = 0;
};

static inline Sort64Plan PlanSort64(const PlanContext& c, bool keyValue, uint32_t elementCount, uint32_t order, uint64_t storageAddress) {
  Sort64Plan p;
  p.keyValue = keyValue;
  p.elementCount = elementCount;
  if (!KeyOrderValid(order)) {
    p.refusal = kKeyOrderRefused;
    return p;
  }
  p.order = order;
  if (elementCount == 0) return p;
  p.layout = MakeSort64Layout(elementCount, c.minStorageBufferOffsetAlignment, storageAddress);
  const bool ordered = order != kKeyOrderUint64;
  const auto add = [&p](Step64 what, uint32_t slot, const char* name) { p.steps[p.stepCount++] = Sort64Step{what, (uint8_t)slot, name}; };
  add(Step64::kSplit, 1, ordered ? "split64_ordered_kernel" : "split64_kernel");
  add(Step64::kSortLoOther, 2, "sort of the low words");
  if (keyValue) {
    add(Step64::kGatherHi, 3, ordered ? "gather_hi64_ordered_kernel" : "gather_hi64_kernel");
    add(Step64::kSortLoOther, 4, "sort of the high words");
    add(Step64::kPermute, 5, ordered ? "permute64_ordered_kernel" : "permute64_kernel");
    add(Step64::kCopyBack, 6, "copy_back64_kernel");
  } else {
    add(Step64::kSortOtherLo, 4, "sort of the high words");
    add(Step64::kMerge, 5, ordered ? "merge64_ordered_kernel" : "merge64_kernel");
  }
  return p;
}

// ---- 32-bit keys with 64-bit values (vrdxHipCmdWideValueSort[Indirect]) ----
// One of three step lists, on the storage of MakeWideValueLayout (vrdx_layout.h); nothing is decided from the data, and an
// indirect call is planned from its bound alone:
//   one workgroup  n <= kWideSmallMaxElements (and PlanContext::smallSort): small_sort_wide_kernel, slot 14
//   gather         iota (A[i] = i) | sort (keys, A) on the caller's keys in place | gather (T[j] = values[A[j]]) |
//                  copy back (values[j] = T[j]); slots 1-4
//   two sorts      from kWideValueTwoSortsFrom elements: split (A = keys, B = value low, C = value high) | sort (A, B) |
//                  sort (keys, C) | merge (values[i] = C[i] << 32 | B[i]); slots 1-4.  Both inner sorts are stable sorts of
//                  the same key sequence, so they apply the same permutation whatever plan or verdict each takes.
// A native two-payload form of the MSD, hybrid and pass kernels would become a fourth list here.
// kWideValueTwoSortsFrom: where the gathered array has left the caches and one more streaming sort costs less than the random
// reads -- the smallest measured size from which the two-sorts form wins by more than the box's 3 %: equal at 2^22 (0.171
// against 0.167 ms), 13 % faster at 2^24, 10 % at 2^26.  tools/build_variants.sh with
// name:-DVRDX_WIDE_VALUE_TWO_SORTS_FROM=... builds the always-gather (0xFFFFFFFF) and always-two-sorts (0) libraries of that
// measurement.
#ifndef VRDX_WIDE_VALUE_TWO_SORTS_FROM
#define VRDX_WIDE_VALUE_TWO_SORTS_FROM (1u << 24)
#endif
constexpr uint32_t kWideValueTwoSortsFrom = VRDX_WIDE_VALUE_TWO_SORTS_FROM;
enum class WideValueForm : uint8_t { kNone, kOneWorkgroup, kGather, kTwoSorts };  // VRDX_HIP_WIDE_VALUE_*
enum class StepWide : uint8_t { kSmallSort, kIota, kSortKeysA, kGather, kCopyBack, kSplit, kSortAB, kSortKeysC, kMerge };
struct WideValueStep { StepWide what; uint8_t slot; const char* name; };  // (name: what EnqueueCheck reports; an inner sort reports its own)
struct WideValuePlan {
  uint32_t elementCount = 0;
  bool atomicRank = false;
  WideValueForm form = WideValueForm::kNone;
  WideValueLayout layout{};
  WideValueStep steps[4];  // none: the empty sort
  uint32_t stepCount = 0;
};

static inline WideValuePlan PlanWideValueSort(const PlanContext& c, uint32_t elementCount, uint64_t storageAddress) {
  WideValuePlan p;
  p.elementCount = elementCount;
  p.atomicRank = c.atomicRank;
  if (elementCount == 0) return p;
  p.layout = MakeWideValueLayout(elementCount, c.minStorageBufferOffsetAlignment, storageAddress);
  const auto add = [&p](StepWide what, uint32_t slot, const char* name) { p.steps[p.stepCount++] = WideValueStep{what, (uint8_t)slot, name}; };
  if (elementCount <= kWideSmallMaxElements && c.smallSort) {
    p.form = WideValueForm::kOneWorkgroup;
    add(StepWide::kSmallSort, 14, "small_sort_wide_kernel");
  } else if (elementCount < kWideValueTwoSortsFrom) {
    p.form = WideValueForm::kGather;
    add(StepWide::kIota, 1, "iota_wide_kernel");
    add(StepWide::kSortKeysA, 2, "sort of the keys with the index");
    add(StepWide::kGather, 3, "gather_wide_kernel");
    add(StepWide::kCopyBack, 4, "copy_back_wide_kernel");
  } else {
    p.form = WideValueForm::kTwoSorts;
    add(StepWide::kSplit, 1, "split_wide_kernel");
    add(StepWide::kSortAB, 2, "sort of the key copy with the low words");
    add(StepWide::kSortKeysC, 3, "sort of the keys with the high words");
    add(StepWide::kMerge, 4, "merge_wide_kernel");
  }
  return p;
}

// ---- segmented sort of 32-bit keys with 64-bit values (vrdxHipCmdWideValueSortSegmented) ----
// Its own plan function, in the shape of PlanSegmentedSort (whose steps it lists: a fill, then segmented_small_wide /
// mid_wide / large_wide_kernel, slots 1 ... 4) on the wide-value storage carved by MakeSegmentedWideLayout.  Nothing is
// decided from the data: grids depend on segmentCount, maxElementCount and the CU count only, so a captured call replays on
// any segmentation with the same segmentCount.  A launch whose grid would be 0 is absent; its slot coincides with the one
// before.  No order word, no bit range: the keys are uint32, whole.
struct WideValueSegmentedPlan {
  bool atomicRank = false;
  const char* refusal = nullptr;  // non-null: refused (no step), and why
  SegmentedLayout layout{};
  SegmentedSortStep steps[4];     // none: refused, or empty (no elements, no segments)
  uint32_t stepCount = 0;
};

static inline WideValueSegmentedPlan PlanWideValueSortSegmented(const PlanContext& c, uint32_t maxElementCount,
                                                                uint32_t segmentCount, uint64_t storageAddress) {
  static constexpr const char* kNames[4] = {"segmented_clear_kernel", "segmented_small_wide_kernel",
                                            "segmented_mid_wide_kernel", "segmented_large_wide_kernel"};
  WideValueSegmentedPlan p;
  p.atomicRank = c.atomicRank;  // one answer for the whole sort
  p.layout = MakeSegmentedWideLayout(maxElementCount, c.minStorageBufferOffsetAlignment, storageAddress);
  if (segmentCount == 0 || maxElementCount == 0) return p;
  if (!p.layout.fits) {  // (cannot happen for N >= 1: the layout fits every count)
    p.refusal = "segmented wide-value storage layout";
    return p;
  }
  // one workgroup per segment up to 2^20 of them (a grid-stride loop beyond); the other two launches take their lists by grid
  // stride with at most as many workgroups as can be resident: one per CU (112 and 118 KiB of LDS)
  const uint32_t resident = (uint32_t)c.computeUnits;
  const uint32_t grids[4] = {1u, std::min<uint32_t>(segmentCount, 1u << 20),
                             std::min<uint32_t>(std::min<uint32_t>(segmentCount, p.layout.midCap), resident),
                             std::min<uint32_t>(std::min<uint32_t>(segmentCount, p.layout.largeCap), resident)};
  for (uint32_t i = 0; i < 4; ++i)
    if (grids[i] != 0) p.steps[p.stepCount++] = SegmentedSortStep{SegmentedStep(i), (uint8_t)(i + 1), kNames[i], grids[i]};
  return p;
}

// Grid of the fused histogram.  Every workgroup ends with up to 1024 global atomics on the same 1024 words, so few, long-lived
// workgroups win for large inputs: one per CU and at least two groups of 16384 keys each (tools/hist_grid.sh, removed, last at
// commit 3645810: 17.4 us with 256 workgroups against 21.1 us with 512 at N = 2^23; equal at 2^25).  Small inputs want the
// opposite -- the kernel is one memory latency long, so up to 128 workgroups of at least 4096 keys share it: 6.9 instead of 9.7 us
// at 2^18, 7.9 instead of 9.8 us at 2^20, same at 2^22.  The MSD plan's form takes whole tiles of up to 32768 keys per workgroup.
static inline uint32_t HistogramGrid(const PlanContext& c, const SortPlan& plan) {
  const uint32_t cap = (uint32_t)c.computeUnits * kHistWorkgroupsPerCu;
  if (plan.msdBits != 0) return std::min<uint32_t>(plan.msdTiles, cap);
  const uint32_t wide = std::min<uint32_t>(128u, RoundUp(plan.elementCount, 4096u));
  const uint32_t grid = std::max(RoundUp(plan.elementCount, 2 * kHistGroupKeys), wide);
  return std::max(std::min(grid, cap), 1u);
}

// What vrdxHipDescribePlan reports of a plan (include/vk_radix_sort.h); *info zeroed by the caller.
static inline void DescribePlan(const SortPlan& plan, VrdxHipPlanInfo* info) {
  const bool kv = plan.keyValue;
  const uint32_t fourPasses = kv ? 68u : 36u;  // 4 (histogram) + 4 x (read + write)
  const uint32_t twoTrips = kv ? 36u : 20u;    // 4 (histogram) + scatter (read + write) + buckets (read + write)
  info->fallbackBytesPerElement = fourPasses;
  info->launches = plan.launches;
  if (plan.oneWorkgroup) {
    info->plan = VRDX_HIP_PLAN_ONE_WORKGROUP;
    info->bytesPerElement = info->fallbackBytesPerElement = kv ? 16u : 8u;
  } else if (plan.msdBits != 0) {
    info->plan = VRDX_HIP_PLAN_MSD;
    info->bits = plan.msdBits;
    info->bytesPerElement = twoTrips;
  } else if (plan.hybridCap != 0) {
    info->plan = VRDX_HIP_PLAN_HYBRID8;
    info->bits = 8;
    info->bytesPerElement = twoTrips;
  } else {
    info->plan = VRDX_HIP_PLAN_FOUR_PASSES;
    info->bytesPerElement = fourPasses;
  }
}

// What vrdxHipDescribeWideValueSortPlan reports of a plan (include/vk_radix_sort.h); *info zeroed by the caller.  The inner
// sorts are priced where their own plan runs (DescribePlan).
static inline void DescribeWideValuePlan(const PlanContext& c, const WideValuePlan& plan, VrdxHipWideValuePlanInfo* info) {
  info->form = (uint32_t)plan.form;
  info->oneWorkgroupMax = c.smallSort ? kWideSmallMaxElements : 0u;
  info->twoSortsFrom = kWideValueTwoSortsFrom;
  if (plan.form == WideValueForm::kNone) return;
  if (plan.form == WideValueForm::kOneWorkgroup) {
    info->launches = 1;
    info->bytesPerElement = 24;  // 12 read, 12 written
    return;
  }
  VrdxHipPlanInfo inner{};
  DescribePlan(PlanSort(c, true, plan.elementCount, 0), &inner);
  info->innerPlan = inner.plan;
  if (plan.form == WideValueForm::kGather) {
    info->launches = 3 + inner.launches;
    info->bytesPerElement = 4 + inner.bytesPerElement + 20 + 16;  // index | sort | gather (4 + 8 at random + 8) | copy back
  } else {
    info->launches = 2 + 2 * inner.launches;
    info->bytesPerElement = 24 + 2 * inner.bytesPerElement + 16;  // split | two sorts | merge
  }
}

// What vrdxHipDescribeRangeSortPlan reports of a plan (include/vk_radix_sort.h); *info zeroed by the caller.
static inline void DescribeRangeSortPlan(const RangeSortPlan& plan, VrdxHipRangeSortPlanInfo* info) {
  info->form = (uint32_t)plan.form;
  info->launches = plan.launches;
  if (plan.form != RangeSortForm::kChunked) {
    if (plan.form == RangeSortForm::kNone) return;
    VrdxHipPlanInfo inner{};
    DescribePlan(plan.inner, &inner);
    info->chunks = 1;
    info->keysPerChunk = plan.elementCount;
    info->digits = plan.form == RangeSortForm::kOneWorkgroup ? (plan.rangeWidth + 7u) / 8u : VRDX_PASSES;
    info->bytesPerElementPerPass = inner.bytesPerElement;  // the whole sort: the digits are ranked between one load and one store
    return;
  }
  info->chunks = plan.grid;
  info->keysPerChunk = plan.chunkKeys;
  info->digits = plan.digits;
  info->bytesPerElementPerPass = plan.keyValue ? 20u : 12u;  // count (keys read) + scatter (read + write)
  info->bytesPerElementCopyBack = plan.keyValue ? 16u : 8u;
}

// What vrdxHipDescribeBalancedSegmentedPlan reports of a plan (include/vk_radix_sort.h); *info zeroed by the caller.
static inline void DescribeBalancedSegmentedPlan(const BalancedSegmentedPlan& plan, VrdxHipBalancedSegmentedPlanInfo* info) {
  info->form = (uint32_t)plan.form;
  info->launches = plan.launches;
  info->spreadFrom = kSegSpreadFrom;
  info->spreadShares = kSegSpreadShares;
  info->minPieceKeys = kSegPieceMinKeys;
  if (plan.form != BalancedForm::kBalanced) return;
  info->spreadCap = plan.layout.spreadCap;
  info->pieceCap = plan.layout.pieceCap;
}

}  // namespace vrdx

#endif  // VRDX_PLAN_H
