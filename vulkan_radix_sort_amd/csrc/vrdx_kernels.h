// Launch interface between the host recorder (vrdx_api.cpp) and the device kernels
// (vrdx_kernels.hip).  Plain pointers and integers only.
#ifndef VRDX_KERNELS_H
#define VRDX_KERNELS_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace vrdx {

constexpr uint32_t kHistThreads = 1024;
constexpr uint32_t kHistCopies = 8;
constexpr uint32_t kHistWorkgroupsPerCu = 1;
constexpr uint32_t kHistCopiesLarge = 32;  // sorts of kHistManyCopiesFrom keys and more
constexpr uint32_t kHistManyCopiesFrom = 1u << 24;
// key+value sorts of more than kStreamingLoadsAbove and at most kStreamingLoadsUpTo elements read their
// tiles with non-temporal loads (vrdx_kernels.hip, StreamingLoads): 16 B per element = 1x ... 3x the 256 MiB
// Infinity Cache of an MI355X
constexpr uint32_t kHistStreamingLoadsAbove = 1u << 25;  // histogram: keys (4 B each) of more than half that cache
constexpr uint32_t kStreamingLoadsAbove = 1u << 24;
constexpr uint32_t kStreamingLoadsUpTo = 3u << 24;
constexpr uint32_t HistLdsBytes(uint32_t copies) { return 4u * 256u * copies * 4u; }  // [pass][digit][copy]
// keys one histogram workgroup counts per GROUP (kHistThreads lanes x four 16-byte loads x 4 keys); every wave keeps
// two groups of loads in flight (vrdx_kernels.hip)
constexpr uint32_t kHistGroupKeys = kHistThreads * 4 * 4;

struct TileConfig {
  int threads;
  int keysPerThread;
  int subTiles;  // 1: onesweep_kernel; 2: onesweep_pair_kernel (two sub-tiles per workgroup and status row)
  uint32_t tileKeys() const { return (uint32_t)threads * (uint32_t)keysPerThread * (uint32_t)subTiles; }
};
constexpr int kNumTileConfigs = 4;
// Every geometry here is selected by ConfigIndex (vrdx_plan.h) for some size range; nothing else is built.
constexpr TileConfig kTileConfigs[kNumTileConfigs] = {
    {1024, 8, 1}, {1024, 16, 1}, {1024, 32, 1}, {1024, 32, 2},
};

// Every spin is bounded: a look-back that makes no progress for this many trips sets the failure word and goes on
// (result unspecified) instead of hanging the GPU.
constexpr uint32_t kSpinLimit = 1u << 18;

struct OnesweepArgs {
  // The pass reads one pair of arrays and writes the other; which is which is decided ON THE DEVICE
  // (trivial passes are skipped, see PassPlan in vrdx_kernels.hip): with four ranking passes it is
  // caller -> scratch on passes 0, 2 and scratch -> caller on 1, 3 (reference :417-427).
  uint32_t* keysCaller;
  uint32_t* keysScratch;
  uint32_t* valuesCaller;     // KV only
  uint32_t* valuesScratch;    // KV only
  uint32_t maxCount;          // element count (direct) or upper bound (indirect)
  const uint32_t* countPtr;   // device-side element count (indirect) or nullptr
  const uint32_t* histogramTable;  // uint[4][256]: raw digit counts of all four passes
  uint32_t* statusCur;        // status region of this pass: [statusRows][256]
  uint32_t* statusNext;       // region to clear for the next pass, or nullptr on the last pass
  uint32_t statusRows;
  // Block sums (sorts of one round on the four-pass plan, BlockPrefix in vrdx_kernels.hip): one row per VRDX_BLOCK_TILES
  // tiles behind the tile rows of each status region; nullptr / 0: the classic look-back.
  uint32_t* blockCur;
  uint32_t* blockNext;
  uint32_t blockRows;
  uint32_t* ticketCur;
  uint32_t* ticketNext;
  uint32_t* failure;          // word in the caller's storage: this sort's (cleared when the next sort is recorded)
  uint32_t* stickyFailure;    // the sorter's own word: OR over every sort recorded with it (vrdxHipReadSorterStatus)
  uint32_t pass;              // 0..3: digit = (key >> 8 * pass) & 255 (the hybrid plan's launch 0 ranks by byte 3)
  uint32_t hybridCap;         // 0, or the bucket capacity of the hybrid plan recorded with this sort (PassPlan)
  uint32_t spinLimit;         // look-back trips without progress before the tile gives up (kSpinLimit)
  // Always 1 (key+value: the forms with tiles of full capacity fetch the values right after the ranking).  Kept as an
  // argument: removing it moves the argument offsets of every kernel that takes OnesweepArgs, and that build measured
  // 0.8 % slower keys-only at 2^25 with no other change to those kernels.
  uint32_t earlyValues;
  uint32_t slots;             // 0: every tile holds the kernel's capacity; otherwise (PlanTiles) the first fullTiles tiles take
                              // `slots` slots of 64 keys per wave (and sub-tile), the tiles behind them tailSlots (multiples of 4)
  uint32_t fullTiles;
  uint32_t tailSlots;
  unsigned long long* trace;  // phase stamps, 8 per tile; nullptr outside tools/trace.sh builds
  uint32_t* planWord;         // hybridCap != 0: the verdict word in the storage (VRDX_OFF_PLAN), written by launch 0
                              // (last on purpose: the argument layout of the kernels that never read it stays as it was)
  // Non-zero: the MSD plan is recorded in front of the passes, which then return when the verdict word says 3 (the plan
  // has taken the sort).
  uint32_t planInFront;
};

// Once per sorter, on the current device: raises the dynamic-LDS limit of every kernel (vrdx_launch.inc).
hipError_t PrepareKernels();

// Also zeroes the two tile tickets and status region 0 (statusClearBytes from statusClear, whole 1 KiB rows): they live
// outside the prefix of the storage that the fill in front of this kernel clears.
hipError_t LaunchHistogram(hipStream_t stream, uint32_t grid, const uint32_t* keys, uint32_t maxCount,
                           const uint32_t* countPtr, uint32_t* globalHistogram, uint32_t* tickets, void* statusClear,
                           uint32_t statusClearBytes);

// atomicRank selects the one-LDS-atomic-per-key ranking; only legal when LdsOrderCheck() said so.
hipError_t LaunchOnesweep(hipStream_t stream, int configIndex, uint32_t grid, bool keyValue, bool atomicRank,
                          const OnesweepArgs& args);

// Small sorts (maxCount <= kSmallSortMaxElements): the whole sort in one workgroup and one launch,
// in place in keys / values (values == nullptr: keys-only); of the storage only *failure is written (0).
constexpr uint32_t kSmallSortMaxElements = 16384;
hipError_t LaunchSmallSort(hipStream_t stream, bool atomicRank, uint32_t* keys, uint32_t* values, uint32_t maxCount,
                           const uint32_t* countPtr, uint32_t* failure);

// The bit-range sorts (vrdxHipCmdSortBits[KeyValue][Indirect]): small_sort_bits_kernel, the range form of the launch above.
// The order is by the field f(key) = the `width` bits of the key from bit beginBit, 1 <= width <= 31 (the range of all 32
// bits IS the whole-key sort); keys move whole.  The kernel ranks ceil(width / 8) digits, digit p the min(8, width - 8 p) bits
// of the key from bit beginBit + 8 p.  The range travels as two kernel arguments behind those of small_sort_kernel.
hipError_t LaunchSmallSortBits(hipStream_t stream, bool atomicRank, uint32_t* keys, uint32_t* values, uint32_t maxCount,
                               const uint32_t* countPtr, uint32_t* failure, uint32_t beginBit, uint32_t width);

// Mid-size sorts, hybrid plan (PassPlan in vrdx_kernels.hip): launch 0 scatters by the keys' highest byte that varies,
// bucket_sort_kernel sorts each of the 256 buckets by the bytes below it inside one workgroup.  hybridCap = 4096, 8192, 16384
// or 32768 elements per bucket (1024 threads x 4 / 8 / 16 / 32); the device decides whether the plan applies.
struct BucketSortArgs {
  const uint32_t* keysScratch;
  uint32_t* keysCaller;
  const uint32_t* valuesScratch;  // KV only
  uint32_t* valuesCaller;         // KV only
  uint32_t maxCount;               // element count (direct) or upper bound (indirect)
  const uint32_t* countPtr;        // device-side element count (indirect) or nullptr
  const uint32_t* histogramTable;  // uint[4][256]
  uint32_t hybridCap;              // elements one workgroup can take (selects the instantiation)
  const uint32_t* planWord;        // the verdict word in the storage (VRDX_OFF_PLAN), written by launch 0
};
hipError_t LaunchBucketSort(hipStream_t stream, bool keyValue, bool atomicRank, const BucketSortArgs& args);

// The MSD plan of large sorts (round 5; vrdx_kernels.hip, "MSD plan"): THREE ranking steps of 10-11 bits instead of four
// of 8, and TWO trips of the data through memory instead of four --
//   histogram_msd_kernel  CHOOSES THE WINDOW (round 6): from 64 keys sampled evenly over the input (first and last key
//                         included; every workgroup takes the same sample and reaches the same answer) it takes the bits in
//                         which they differ and puts the 2^bits-wide window right below their common prefix -- keys of 24
//                         bits, dense sorted ids, anything narrow then spread over all the buckets like uniform 32-bit keys do
//                         over the top bits -- and predicts what the plan cannot take anyway (MsdMode below).  Then the byte
//                         histograms (for the fallback) and, per tile of tileKeys keys, the counts of the keys' window bits as
//                         16-bit numbers (tileCounts); the bucket sizes; a key that breaks the sampled prefix raises the
//                         overflow word -- the sample is the guess, the count stays the proof;
//   spine_msd_kernel      turns the counts, in place, into exclusive prefixes over the tiles and leaves every bucket's base;
//                         a bucket beyond `cap` elements sets *overflowWord;
//   the scatter launch    one stable scatter by the window bits, caller -> scratch: no ticket, no look-back, no status words --
//                         a tile's bases are bucketBase[d] + its row of prefixes; keys-only sorts take TWO consecutive tiles per
//                         workgroup (round 6: runs of 256 bytes instead of 128);
//   the bucket launch     one workgroup per bucket sorts it by the bits below the window (none, one or two stable passes of
//                         up to 11 bits) inside its LDS, scratch -> caller.
// The scatter launch is also pass 0 of the fallback and the bucket launch, with full-size buckets, pass 1 (LaunchMsdFused);
// buckets of half the size take bucket_sort2_half_kernel (LaunchBucketSortHalf), and pass 1 is a launch of its own.
// All of it with wave-private counters of 16 bits, two to a word.  The device decides (the overflow word): with a bucket
// beyond the capacity or a key outside the prefix the last two run their pass instead (the half-size bucket kernel returns at
// once) and the passes recorded behind them follow.
constexpr uint32_t kMsdTileKeys = 32768;   // a scatter tile's capacity: 1024 threads x 32 keys
constexpr uint32_t kMsdMaxTiles = 2048;    // spine_msd_kernel: 64 chunks of at most 32 rows
constexpr uint32_t kMsdCapKeys = 36864;    // bucket capacity, keys-only: 1024 threads x 36 keys (144 KiB of staging)
constexpr uint32_t kMsdCapKeyValue = 36864;  // the same for pairs: keys and values take turns in the staging buffer
constexpr uint32_t kMsdHalfCap = 18432;    // buckets of the half-size bucket kernel: 512 threads x 36 elements (72 KiB of staging), two workgroups per CU
// What the histogram kernel decides travels in the OVERFLOW WORD itself (VRDX_OFF_MSD_OVERFLOW), so that every launch behind it learns
// "is the plan turned down, where is the window, what kind of input is it" from the one word it reads anyway -- a second
// word would be a second dependent memory round trip in front of the first key load of every workgroup:
//   bits 0-7   non-zero = the plan is turned down (kMsdDecline*: by the spine or by the histogram kernel)
//   bits 8-13  shift: the scatter ranks by (key >> shift) & (2^bits - 1); the bucket kernel sorts the `shift` bits below
//   bits 16-17 MsdMode
// The scatter passes the shift on in the verdict word (kMsdVerdict* | shift << 8) for the same reason.
constexpr uint32_t kMsdDeclineMask = 0xFFu;
constexpr uint32_t kMsdDeclineBucket = 1u;  // spine: a bucket holds more than the capacity
constexpr uint32_t kMsdDeclinePrefix = 2u;  // histogram: a key outside the sampled prefix / not the sampled key (all sampled keys identical)
constexpr uint32_t kMsdDeclineSample = 4u;  // histogram: the sample rules the plan out
constexpr uint32_t kMsdShiftShift = 8u, kMsdShiftMask = 63u, kMsdModeShift = 16u, kMsdModeMask = 3u;
enum MsdMode : uint32_t {
  kMsdModePlan = 0,       // counts per tile and window value; spine, scatter, buckets
  kMsdModeDeclined = 1,   // the sample shows a bucket the plan cannot hold (few distinct values, keys of fewer bits than the
                          // window over more elements than fit): the overflow word is raised at once, the four byte tables
                          // are all that is counted and the spine kernel returns
  kMsdModeIdentical = 2,  // every sampled key is the same: the histogram kernel checks that ALL are (or raises the overflow
                          // word); if so the input is sorted as it stands and every launch behind returns (verdict 4)
};
// The sample: one key per lane of wave 0 of every histogram workgroup, evenly spread, first and last key included.  (Round 6
// first took it in a one-workgroup kernel in place of the fill in front of the sort -- 4096 keys: an 11.5 us kernel, 1024 keys:
// 5.9 us, where the fill takes 4.3 and the histogram kernel cannot start before it has ended.  64 lines re-read by every
// workgroup are nothing next to the 512 KiB each of them streams.)
constexpr uint32_t kMsdSampleKeys = 64;
constexpr uint32_t kMsdSampleSkew = 8;      // sampled keys in one bucket (expected: 1 / 16 or less) from which the plan is turned down unseen
// verdict word (VRDX_OFF_PLAN), low byte, of the MSD plan; the passes behind it return on either
constexpr uint32_t kMsdVerdictMask = 0xFFu;
constexpr uint32_t kMsdVerdictRuns = 3;      // scatter and bucket launches do the sort (bits 8-13: the window's shift)
constexpr uint32_t kMsdVerdictSorted = 4;    // all keys identical: nothing to do
struct MsdArgs {
  uint32_t* keysCaller;
  uint32_t* keysScratch;
  uint32_t* valuesCaller;      // KV only
  uint32_t* valuesScratch;     // KV only
  uint32_t maxCount;           // element count (direct) or upper bound (indirect)
  const uint32_t* countPtr;    // device-side element count (indirect) or nullptr
  uint32_t* histogramTable;    // uint[4][256]
  uint32_t* tileCounts;        // [tiles][2^bits / 2] words = pairs of 16-bit numbers: counts, then prefixes over the tiles
  uint32_t* bucketBase;        // [2^bits]
  uint32_t* bucketCount;       // [2^bits]: zeroed by the fill in front of the sort; added up by the histogram kernel (windows below a prefix) or by the spine
  uint32_t* overflowWord;      // VRDX_OFF_MSD_OVERFLOW in the storage: non-zero = the plan is turned down
  uint32_t* planWord;          // VRDX_OFF_PLAN: the scatter writes kMsdVerdictRuns / kMsdVerdictSorted (the passes then return)
  uint32_t bits;               // 10 | 11
  uint32_t cap;                // elements a bucket may hold
  uint32_t tiles;              // ceil(maxCount / tileKeys) <= kMsdMaxTiles
  uint32_t tileKeys;           // keys per tile of the histogram's counts and of the scatter: a multiple of 4096, at most kMsdTileKeys
  // status region 0 of the fallback's passes (16-byte vectors): zeroed by the spine kernel, whose 32-64 workgroups have the
  // bandwidth to spare, instead of by the histogram kernel (which it cost 1.9 us at 2^25, round 4)
  void* statusClear;
  uint32_t statusVecs;
  // The bucket launch's output policy (BucketSort2Body): keys-only sorts of more than kStreamingLoadsAbove elements write
  // their buckets with non-temporal stores, all but the last plainTail buckets in the order the launch takes them (the
  // highest indices), which keep plain stores.  MsdPlainTail (2^bits: every bucket plain); in the padding behind statusVecs: no argument moves.
  uint32_t plainTail;
  uint32_t* tickets;           // zeroed by the histogram kernel
  uint32_t* declinedPlans;     // the sorter's counter of plans the device turned down (vrdxHipReadPlanCounters), or nullptr
};
hipError_t LaunchHistogramMsd(hipStream_t stream, uint32_t grid, const MsdArgs& args);
hipError_t LaunchSpineMsd(hipStream_t stream, const MsdArgs& args);
// The bucket launch of buckets of at most kMsdHalfCap (ten bits): bucket_sort2_half_kernel.
hipError_t LaunchBucketSortHalf(hipStream_t stream, bool keyValue, const MsdArgs& args);
// The scatter (bucketLaunch = false) or bucket (true) launch of the plan with pass 0 / pass 1 of its fallback as a second
// role, chosen on the device by the plan's verdict: saves two of the four returning launches.  `pass` = the arguments and
// passGrid the grid LaunchOnesweep would have been given for that pass (the two-sub-tile kernel keys-only, 1024x32
// key+value; one-atomic ranking).
hipError_t LaunchMsdFused(hipStream_t stream, bool bucketLaunch, bool keyValue, const MsdArgs& args, const OnesweepArgs& pass,
                          uint32_t passGrid);

// Segmented sort (vrdx_kernels.hip, "segmented sort"): segmentCount independent ranges [offsets[i], offsets[i + 1]) of
// one array, every range sorted on its own, in place.  The host never learns the sizes; each segment's size class is decided
// on the device:
//   segmented_small_kernel  one 256-thread workgroup per segment (a grid-stride loop above the grid's cap): checks the
//                           segment's offsets, sorts it in LDS when it holds at most kSegSmallMax elements, and otherwise
//                           appends its id to the mid list (at most kSegMidMax) or to the large list;
//   segmented_mid_kernel    1024 threads, takes the mid list by grid stride: one in-LDS sort per segment;
//   segmented_large_kernel  1024 threads, takes the large list by grid stride: one stable LSD sort through memory per
//                           segment, ping-ponging between the caller's range and the same index range of the scratch.
constexpr uint32_t kSegSmallMax = 256u * 16u;  // the 256 x 16 form of SortInWorkgroup
constexpr uint32_t kSegMidMax = 1024u * 16u;   // the 1024 x 16 form
constexpr uint32_t kSegLargeTile = 1024u * 16u;  // keys per tile of the large kernel's passes
struct SegmentedArgs {
  uint32_t* keys;
  uint32_t* values;             // KV only
  uint32_t* keysScratch;        // large segments: the same index range as in keys
  uint32_t* valuesScratch;      // KV only
  const uint32_t* offsets;      // segmentCount + 1 words, read on the device
  uint32_t segmentCount;
  uint32_t maxCount;            // no segment may end behind it
  uint32_t* midCount;           // appended to by the small kernel (zeroed by the fill in front of it)
  uint32_t* midList;            // [midCap] segment ids
  uint32_t midCap;
  uint32_t* largeCount;
  uint32_t* largeList;          // [largeCap] segment ids
  uint32_t largeCap;
  uint32_t* failure;            // the storage's failure word (word 3 of the header): VRDX_HIP_STATUS_SEGMENTS_INVALID
  uint32_t* stickyFailure;      // the sorter's word
};
// The fill in front of the first launch (one wave): header words 0-3 (failure = word 3) and both list counters.
hipError_t LaunchSegmentedClear(hipStream_t stream, const SegmentedArgs& args);
enum SegmentClass { kSegmentSmall = 0, kSegmentMid = 1, kSegmentLarge = 2 };  // segmented_small / mid / large_kernel
// width == 0: the whole key.  Otherwise the segmented sort by a bit range (vrdxHipCmdSortSegmentedBits[KeyValue]):
// segmented_small_bits / mid_bits / large_bits_kernel, the range forms of the three kernels.  Every segment is ordered by f(key) =
// the `width` bits of the key from bit beginBit, 1 <= width <= 31 (the range of all 32 bits IS the whole-key segmented sort);
// keys move whole.  The in-LDS kernels rank ceil(width / 8) digits (SortInWorkgroup's RANGE form); the large kernel counts those
// digits of the field in its one histogram read and walks the segment once per digit that varies.  The range travels as two
// kernel arguments behind SegmentedArgs, which does not change.
hipError_t LaunchSegmented(hipStream_t stream, SegmentClass sizeClass, uint32_t grid, bool keyValue, bool atomicRank,
                           const SegmentedArgs& args, uint32_t beginBit, uint32_t width);

// ---- range sorts beyond one workgroup (vrdxHipCmdRangeSort[KeyValue][Indirect]; vrdx_kernels.hip, "range sort") ----
// Count, scan, scatter per digit of the field, a copy back after an odd number of active passes (PlanRangeSort in
// vrdx_plan.h lists the launches; MakeRangeSortLayout in vrdx_layout.h places the arrays).  `grid` workgroups take the chunks
// of RangeChunkKeys (vrdx_layout.h): the host sizes it from maxCount, the kernels cut the count they read with it.
struct RangeSortArgs {
  uint32_t* keys;
  uint32_t* values;            // KV only
  uint32_t* keysScratch;
  uint32_t* valuesScratch;     // KV only
  uint32_t maxCount;           // element count (direct) or upper bound (indirect)
  const uint32_t* countPtr;    // device-side element count (indirect) or nullptr
  uint32_t* totals;            // uint[4][256]: the field's digits over the whole array (zeroed by the fill in front)
  uint32_t* counts;            // uint[grid][256]: per chunk, the pass's counts, then its positions
  uint32_t* state;             // header word 2: the mask of active passes (the first scan launch writes it)
  uint32_t grid;               // workgroups of the count and scatter launches = rows of `counts`
  uint32_t beginBit, width;    // the range: 1 <= width <= 31, beginBit + width <= 32
  uint32_t pass;               // the digit this launch works on (the copy back: unused)
};
constexpr uint32_t kRangeCopyThreads = 256;
// pass 0: also the totals of every digit; reads the caller's keys
hipError_t LaunchRangeCount(hipStream_t stream, const RangeSortArgs& args);
// one workgroup; pass 0: also the mask of active passes
hipError_t LaunchRangeScan(hipStream_t stream, const RangeSortArgs& args);
hipError_t LaunchRangeScatter(hipStream_t stream, bool keyValue, bool atomicRank, const RangeSortArgs& args);
hipError_t LaunchRangeCopyBack(hipStream_t stream, bool keyValue, const RangeSortArgs& args);

// ---- the balanced segmented sort (vrdxHipCmdBalancedSortSegmented[KeyValue]; vrdx_kernels.hip, "balanced segmented sort")
// ---- The segmented sort's fill, small and mid launches as they are; then segmented_split_kernel (one workgroup) cuts the
// large list into the SPREAD segments and the rest (vrdx_layout.h, MakeBalancedSegmentedLayout), the unchanged
// segmented_large_kernel runs on the rest list, and the pieces of the spread segments are sorted by count, scan and scatter
// launches per byte of the key and a copy back (PlanBalancedSegmentedSort in vrdx_plan.h lists the launches).
struct BalancedSegmentedArgs {
  SegmentedArgs segmented;     // what the twin's kernels take; the large launch gets restCount / restList in its place
  uint32_t* restCount;         // written by the split kernel
  uint32_t* restList;          // [segmented.largeCap] segment ids
  uint32_t* split;             // [kSegSplitWords]: listed, spread, pieces, L; written by the split kernel
  uint32_t* spreadTable;       // [spreadCap][kSegSpreadEntryWords]
  uint32_t* pieceTable;        // [pieceCap][kSegPieceEntryWords]
  uint32_t* rows;              // [pieceCap][256]: per piece, the pass's counts, then its positions
  uint32_t spreadCap, pieceCap;
  uint32_t computeUnits;       // the divisor of the share and of the piece length
  uint32_t pass;               // the byte this launch works on (the split and the copy back: unused)
};
hipError_t LaunchSegmentedSplit(hipStream_t stream, const BalancedSegmentedArgs& args);
// one workgroup per piece slot | per spread slot | per piece slot | per piece slot; a slot without a piece or a segment returns
hipError_t LaunchSegmentedPieceCount(hipStream_t stream, const BalancedSegmentedArgs& args);
hipError_t LaunchSegmentedPieceScan(hipStream_t stream, const BalancedSegmentedArgs& args);
hipError_t LaunchSegmentedPieceScatter(hipStream_t stream, bool keyValue, bool atomicRank, const BalancedSegmentedArgs& args);
hipError_t LaunchSegmentedPieceCopyBack(hipStream_t stream, bool keyValue, const BalancedSegmentedArgs& args);

// ---- key orders of the 64-bit sorts (vrdxHipCmdSort64Ordered*, vrdxHipCmdSortSegmented64Ordered*; vrdx_kernels.hip, "key
// orders of the 64-bit sorts") ----
// The order word of include/vk_radix_sort.h: a key type, VRDX_HIP_ORDER_DESCENDING or-ed in or not.  The kernels sort
// T(key) ascending as unsigned 64-bit, T(k) = k ^ flip ^ (float64 and bit 63 of k set ? 0x7FFFFFFFFFFFFFFF : 0) with flip = 0
// (uint64) or 1 << 63 (int64, float64), complemented for descending; T is a bijection, so equal keys and only they have equal
// T, and they keep their input order in both directions.
constexpr uint32_t kKeyOrderUint64 = 0, kKeyOrderInt64 = 1, kKeyOrderFloat64 = 2;
constexpr uint32_t kKeyOrderTypeMask = 0xFFu;
constexpr uint32_t kKeyOrderDescending = 0x100u;
constexpr bool KeyOrderValid(uint32_t order) {
  return (order & ~(kKeyOrderTypeMask | kKeyOrderDescending)) == 0 && (order & kKeyOrderTypeMask) <= kKeyOrderFloat64;
}

// ---- 64-bit keys (vrdxHipCmdSort64[KeyValue][Indirect]): the steps around the two 32-bit sorts (vrdx_kernels.hip, "64-bit
// keys") ----
// Every thread takes four consecutive elements; 0 < maxCount <= VRDX_MAX_ELEMENTS sizes the grid, and the kernels work on
// min(*countPtr, maxCount) elements (countPtr == nullptr: on maxCount).  keys: the caller's, 8-byte aligned; values: the
// caller's, 4-byte aligned; every other array lies inside the storage on a 16-byte boundary (MakeSort64Layout).
constexpr uint32_t kSort64Threads = 256;
// order: the order word above; kKeyOrderUint64 starts the kernels without one (split64_kernel ...), every other valid word the
// ordered forms (split64_ordered_kernel ...) with the word behind the same arguments -- one device function per step, the
// plain kernel with the constant word; an invalid word is refused with hipErrorInvalidValue.  T = the identity for kKeyOrderUint64.
// lo[i] = low word of T(keys[i]); other[i] = its high word, or i (iota)
hipError_t LaunchSplit64(hipStream_t stream, bool iota, const uint64_t* keys, uint32_t* lo, uint32_t* other, uint32_t maxCount,
                         const uint32_t* countPtr, uint32_t order);
// keys[i] = the inverse of T on hi[i] << 32 | lo[i]
hipError_t LaunchMerge64(hipStream_t stream, uint64_t* keys, const uint32_t* lo, const uint32_t* hi, uint32_t maxCount,
                         const uint32_t* countPtr, uint32_t order);
// hi[j] = high word of T(keys[index[j]]) (read: the high word of the key alone)
hipError_t LaunchGatherHi64(hipStream_t stream, const uint64_t* keys, const uint32_t* index, uint32_t* hi, uint32_t maxCount,
                            const uint32_t* countPtr, uint32_t order);
// keysOut[j] = (the key's high word, from T's high word hiThenValues[j]) << 32 | low word of keys[index[j]]; then
// hiThenValues[j] = values[index[j]]
hipError_t LaunchPermute64(hipStream_t stream, const uint64_t* keys, const uint32_t* values, const uint32_t* index,
                           uint32_t* hiThenValues, uint64_t* keysOut, uint32_t maxCount, const uint32_t* countPtr, uint32_t order);
// keys[i] = keysIn[i]; values[i] = valuesIn[i]
hipError_t LaunchCopyBack64(hipStream_t stream, uint64_t* keys, uint32_t* values, const uint64_t* keysIn,
                            const uint32_t* valuesIn, uint32_t maxCount, const uint32_t* countPtr);

// ---- segmented sort of 64-bit keys (vrdxHipCmdSortSegmented64[KeyValue]; vrdx_kernels.hip, "segmented sort of 64-bit
// keys"): the three size classes of the segmented sort, every segment moved through memory once in the in-LDS classes ----
//   segmented_small64_kernel  256 threads, one workgroup per segment by grid stride: checks the offsets, sorts segments of
//                             2 ... kSeg64SmallMax keys in LDS (SortInWorkgroup64<256, 16>), lists the bigger ones;
//   segmented_mid64_kernel    1024 threads over the mid list: SortInWorkgroup64<1024, 16> keys-only (two word planes of
//                             64 KiB), <1024, 8> key+value (three planes of 32 KiB: 12 bytes x 16384 do not fit the LDS,
//                             so the key+value mid class ends at 8192);
//   segmented_large64_kernel  1024 threads over the large list: SegmentLsd64, tiles of kSeg64LargeTile keys.
constexpr uint32_t kSeg64SmallMax = 256u * 16u;
constexpr uint32_t kSeg64MidMax = 1024u * 16u;         // keys-only
constexpr uint32_t kSeg64MidMaxKeyValue = 1024u * 8u;  // key+value
constexpr uint32_t kSeg64LargeTile = 1024u * 8u;       // keys per tile of the large kernel's passes, both forms
struct Segmented64Args {
  uint64_t* keys;
  uint32_t* values;             // KV only
  uint64_t* keysScratch;        // large segments: the same index range as in keys
  uint32_t* valuesScratch;      // KV only
  const uint32_t* offsets;      // segmentCount + 1 words, read on the device
  uint32_t segmentCount;
  uint32_t maxCount;            // no segment may end behind it
  uint32_t* midCount;           // appended to by the small kernel (zeroed by the fill in front of it)
  uint32_t* midList;            // [midCap] segment ids
  uint32_t midCap;
  uint32_t* largeCount;
  uint32_t* largeList;          // [largeCap] segment ids
  uint32_t largeCap;
  uint32_t* failure;            // the storage's failure word (word 3 of the header): VRDX_HIP_STATUS_SEGMENTS_INVALID
  uint32_t* stickyFailure;      // the sorter's word
};
// The fill in front of the first launch is segmented_clear_kernel as it is: the same header words and list counters.
hipError_t LaunchSegmentedClear(hipStream_t stream, const Segmented64Args& args);
// order as above: kKeyOrderUint64 starts segmented_small64 / mid64 / large64_kernel, every other valid word their ordered forms
// (every segment in ascending order of T(key))
hipError_t LaunchSegmented64(hipStream_t stream, SegmentClass sizeClass, uint32_t grid, bool keyValue, bool atomicRank,
                             const Segmented64Args& args, uint32_t order);

// ---- key orders of the 32-bit sorts (vrdxHipCmdOrderedSort*; vrdx_kernels.hip, "key orders of the 32-bit sorts") ----
// The same order word on 32 bits: the key types are uint32, int32 and float32 (KeyOrderValid serves both widths).  The kernels
// sort T(key) ascending as unsigned 32-bit, T(k) = k ^ flip ^ (float32 and bit 31 of k set ? 0x7FFFFFFF : 0) with flip = 0
// (uint32) or 1 << 31 (int32, float32), complemented for descending.  Every launcher below takes a VALID word other than
// kKeyOrderUint32 (the planner hands that one to the unordered kernels) and refuses anything else with hipErrorInvalidValue.
constexpr uint32_t kKeyOrderUint32 = 0, kKeyOrderInt32 = 1, kKeyOrderFloat32 = 2;
constexpr bool KeyOrder32Launchable(uint32_t order) { return order != kKeyOrderUint32 && KeyOrderValid(order); }
// small_sort_ordered_kernel: LaunchSmallSort with every element as T(key) between the load and the store
hipError_t LaunchSmallSortOrdered(hipStream_t stream, bool atomicRank, uint32_t* keys, uint32_t* values, uint32_t maxCount,
                                  const uint32_t* countPtr, uint32_t* failure, uint32_t order);
// order32_kernel: keys[i] = T(keys[i]) (inverse: T^-1) for i < min(*countPtr, maxCount) (countPtr == nullptr: maxCount), in
// place, four keys per thread; keys: the caller's, 4-byte aligned.  Around the unchanged plan of a flat sort beyond one workgroup.
constexpr uint32_t kOrder32Threads = 256;
hipError_t LaunchOrder32(hipStream_t stream, bool inverse, uint32_t* keys, uint32_t maxCount, const uint32_t* countPtr,
                         uint32_t order);
// segmented_small_ordered / mid_ordered / large_ordered_kernel: the whole-key segmented kernels with every segment in
// ascending order of T(key); the order word travels behind SegmentedArgs, which does not change.
hipError_t LaunchSegmentedOrdered(hipStream_t stream, SegmentClass sizeClass, uint32_t grid, bool keyValue, bool atomicRank,
                                  const SegmentedArgs& args, uint32_t order);

// ---- 32-bit keys with 64-bit values (vrdxHipCmdWideValueSort[Indirect]; vrdx_kernels.hip, "32-bit keys with 64-bit
// values") ----
// small_sort_wide_kernel: up to kWideSmallMaxElements elements in one workgroup, key and both value words through three
// staging planes (the body of SortInWorkgroup64 with only the key ranked): 256 threads x 16 up to 4096 elements, 1024 x 8
// beyond.  keys: 4-byte aligned; values: 8-byte aligned, one 8-byte access per element; failure: word 3 of the header.
constexpr uint32_t kWideSmall256Max = 256u * 16u;
constexpr uint32_t kWideSmallMaxElements = 1024u * 8u;
hipError_t LaunchSmallSortWide(hipStream_t stream, bool atomicRank, uint32_t* keys, uint64_t* values, uint32_t maxCount,
                               const uint32_t* countPtr, uint32_t* failure);
// The streaming steps of the two larger forms, in the shape of the 64-bit sorts' (kSort64Threads threads, four consecutive
// elements per thread, min(*countPtr, maxCount) elements).  keys: the caller's, 4-byte aligned; values: the caller's, 8-byte
// aligned; every other array lies inside the storage on a 16-byte boundary (MakeWideValueLayout).
// index[i] = i
hipError_t LaunchIotaWide(hipStream_t stream, uint32_t* index, uint32_t maxCount, const uint32_t* countPtr);
// out[j] = values[index[j]]
hipError_t LaunchGatherWide(hipStream_t stream, const uint64_t* values, const uint32_t* index, uint64_t* out, uint32_t maxCount,
                            const uint32_t* countPtr);
// values[j] = in[j]
hipError_t LaunchCopyBackWide(hipStream_t stream, uint64_t* values, const uint64_t* in, uint32_t maxCount,
                              const uint32_t* countPtr);
// keysCopy[i] = keys[i]; lo[i], hi[i] = the words of values[i]
hipError_t LaunchSplitWide(hipStream_t stream, const uint32_t* keys, const uint64_t* values, uint32_t* keysCopy, uint32_t* lo,
                           uint32_t* hi, uint32_t maxCount, const uint32_t* countPtr);
// values[i] = hi[i] << 32 | lo[i]
hipError_t LaunchMergeWide(hipStream_t stream, uint64_t* values, const uint32_t* lo, const uint32_t* hi, uint32_t maxCount,
                           const uint32_t* countPtr);

// ---- segmented sort of 32-bit keys with 64-bit values (vrdxHipCmdWideValueSortSegmented; vrdx_kernels.hip, "segmented sort
// of 32-bit keys with 64-bit values"): the three size classes of the key+value segmented 64-bit sort with the planes (key,
// value low, value high); every segment moves through memory once in the in-LDS classes ----
//   segmented_small_wide_kernel  256 threads, one workgroup per segment by grid stride: checks the offsets, sorts segments of
//                                2 ... kSegWideSmallMax elements in LDS (256 x 16), lists the bigger ones;
//   segmented_mid_wide_kernel    1024 threads over the mid list: 1024 x 8, three planes of 32 KiB;
//   segmented_large_wide_kernel  1024 threads over the large list: SegmentLsdWide, tiles of kSegWideLargeTile elements.
// keys, offsets: 4-byte aligned; values: 8-byte aligned, one 8-byte access per element and pass.
constexpr uint32_t kSegWideSmallMax = 256u * 16u;
constexpr uint32_t kSegWideMidMax = 1024u * 8u;
constexpr uint32_t kSegWideLargeTile = 1024u * 8u;
struct SegmentedWideArgs {
  uint32_t* keys;
  uint64_t* values;
  uint32_t* keysScratch;        // large segments: the same index range as in keys
  uint64_t* valuesScratch;      //                 and as in values
  const uint32_t* offsets;      // segmentCount + 1 words, read on the device
  uint32_t segmentCount;
  uint32_t maxCount;            // no segment may end behind it
  uint32_t* midCount;           // appended to by the small kernel (zeroed by the fill in front of it)
  uint32_t* midList;            // [midCap] segment ids
  uint32_t midCap;
  uint32_t* largeCount;
  uint32_t* largeList;          // [largeCap] segment ids
  uint32_t largeCap;
  uint32_t* failure;            // the storage's failure word (word 3 of the header): VRDX_HIP_STATUS_SEGMENTS_INVALID
  uint32_t* stickyFailure;      // the sorter's word
};
// The fill in front of the first launch is segmented_clear_kernel as it is: the same header words and list counters.
hipError_t LaunchSegmentedClear(hipStream_t stream, const SegmentedWideArgs& args);
hipError_t LaunchSegmentedWide(hipStream_t stream, SegmentClass sizeClass, uint32_t grid, bool atomicRank,
                               const SegmentedWideArgs& args);

// ---- the kernels' dynamic LDS and the MSD plan's grids: one definition for the kernels (vrdx_kernels.hip) and for both
// launch backends (vrdx_launch.inc) ----
// Key+value tiles replay the permutation for the values through the SAME staging buffer after the
// keys have left it (like the reference, downsweep.slang:208-224): the LDS footprint equals the
// keys-only one, so two workgroups fit per CU (keys and values staged together would need 128 KiB
// at T = 16384: one workgroup per CU and nothing to overlap its waits with).
constexpr size_t OnesweepLdsWords(int threads, int kpt) {
  // staging buffer (keys, then values) | per-wave digit counters.  Everything else lives inside
  // those two at times when they are idle: ticket + scan scratch at the front of the staging
  // buffer (before the regroup), look-back scratch at the bottom and the per-digit scatter offsets
  // in the top 256 words of the counters (after the regroup).  1024 x 16 is then exactly 80 KiB:
  // two workgroups per CU.
  return (size_t)threads * kpt + (size_t)(threads / 64) * 256;
}

// onesweep_pair_kernel: staging (THREADS*KPT) | wave counters (WAVES*256) | look-back scratch + scan scratch +
// ticket | digit offsets of A and of B (2 x 256).
constexpr size_t PairLdsWords(int threads, int kpt) {
  return (size_t)threads * kpt + (size_t)(threads / 64) * 256 + (size_t)256 * (2 + 2 * (threads / 256)) + 512;
}

// SortInWorkgroup (small_sort_kernel, bucket_sort_kernel, the segmented sort's in-LDS forms).  Key+value with THREADS * KPT
// = 32768 elements: two staging buffers of that size do not fit the CU's LDS, so keys and values take turns in ONE (like the
// pass kernels, and like the reference, downsweep.slang:208-224): two more barriers per pass, the same LDS traffic.
constexpr bool SharedStage(int threads, int kpt, bool kv) {
  return kv && (size_t)threads * kpt * 2 * 4 + (size_t)(threads / 64) * 1024 + 64 > 160 * 1024;
}

constexpr size_t SmallSortLdsWords(int threads, int kpt, bool kv) {
  return (size_t)threads * kpt * (kv && !SharedStage(threads, kpt, kv) ? 2 : 1) + (size_t)(threads / 64) * 256 + 16;
}

constexpr size_t SegmentLargeLdsWords(bool kv) {
  // staging (keys, values) | wave counters 16 x 256 | scan scratch 16 | bases 4 x 256 | tile starts 256 | tile counts 256 | 16
  return (size_t)kSegLargeTile * (kv ? 2 : 1) + 16 * 256 + 16 + 4 * 256 + 256 + 256 + 16;
}

constexpr size_t RangeScatterLdsWords(bool kv) {
  // staging (keys, values) | wave counters 16 x 256 | scan scratch 16 | base 256 | tile starts 256 | tile counts 256 | 16
  return (size_t)kSegLargeTile * (kv ? 2 : 1) + 16 * 256 + 16 + 256 + 256 + 256 + 16;
}

// SortInWorkgroup64: one staging plane per key word (and one for the values) | wave counters | scan scratch and the two
// masks of varying bytes.  256 x 16: 36 KiB keys-only, 52 KiB key+value; 1024 x 16 keys-only: 144 KiB; 1024 x 8 key+value:
// 112 KiB.
constexpr size_t SortInWorkgroup64LdsWords(int threads, int kpt, bool kv) {
  return (size_t)threads * kpt * (kv ? 3 : 2) + (size_t)(threads / 64) * 256 + 16;
}
constexpr int Seg64MidKpt(bool kv) { return (int)((kv ? kSeg64MidMaxKeyValue : kSeg64MidMax) / 1024u); }

constexpr size_t Segment64LargeLdsWords(bool kv) {
  // staging (low words, high words, values) | wave counters 16 x 256 | scan scratch 32 | bases 8 x 256 | tile starts 256 |
  // tile counts 256 | 16: 90 KiB keys-only, 122 KiB key+value
  return (size_t)kSeg64LargeTile * (kv ? 3 : 2) + 16 * 256 + 32 + 8 * 256 + 256 + 256 + 16;
}

constexpr size_t SegmentWideLargeLdsWords() {
  // staging (keys, value low words, value high words) | wave counters 16 x 256 | scan scratch 32 | bases 4 x 256 | tile
  // starts 256 | tile counts 256 | 16: 118.2 KiB
  return (size_t)kSegWideLargeTile * 3 + 16 * 256 + 32 + 4 * 256 + 256 + 256 + 16;
}

// histogram_msd_kernel
constexpr uint32_t kMsdTopBinWords = 8192;  // 32 KiB: 1024 bins x 8 replicas | 2048 x 4
constexpr uint32_t HistMsdByte3Copies(uint32_t copies) { return copies < 16u ? copies : 16u; }
constexpr uint32_t HistMsdLdsBytes(uint32_t copies, uint32_t bits) {
  return (3u * 256u * copies + kMsdTopBinWords + (1u << bits) + 256u * HistMsdByte3Copies(copies) + 4u) * 4u;
}

constexpr size_t ScatterMsdLdsWords(uint32_t bits) { return (size_t)kMsdTileKeys + ((size_t)1 << bits) + 32; }

// the bucket role of msd_buckets_or_pass1_kernel (THREADS = 1024) and bucket_sort2_half_kernel (512)
constexpr size_t BucketSort2LdsWords(int kpt, int threads = 1024) { return (size_t)threads * kpt + 32; }

// msd_scatter_or_pass0_kernel / msd_buckets_or_pass1_kernel: the larger of the two roles'
constexpr size_t MsdFusedLdsWords(bool kv, uint32_t bits, bool bucketLaunch) {
  const size_t pass = kv ? OnesweepLdsWords(1024, 32) : PairLdsWords(1024, 32);
  const size_t plan = bucketLaunch ? BucketSort2LdsWords((int)((kv ? kMsdCapKeyValue : kMsdCapKeys) / 1024))
                                   : ScatterMsdLdsWords(bits);
  return pass > plan ? pass : plan;
}

// lds_order_check_packed_kernel
constexpr size_t kOrderCheckPackedLdsBytes = 2 * 16 * 1024 * sizeof(uint32_t);

// workgroups of the plan's scatter: one per tile, or per two tiles (keys-only, ten bits), rounded up to a multiple of 8
constexpr uint32_t MsdScatterGrid(uint32_t tiles, bool keyValue, uint32_t bits) {
  const uint32_t units = !keyValue && bits == 10 ? (tiles + 1u) / 2u : tiles;
  return 8u * ((units + 7u) / 8u);
}

// Workgroups of the plan's bucket launch.  The full-size kernel (one workgroup per CU): 2^bits / 2, the grid of round 6, when
// a workgroup took TWO fixed buckets one after the other -- half as many workgroups to start and to drain, 107.4 instead of
// 110.9 us keys-only at 2^25, 175-178 instead of 179-180 key+value (tools/r06/bucket_grid.sh, bucket_grid2.sh, removed, last
// at commit 3645810).  Since round 8 its workgroups draw their buckets by ticket (BucketSort2Body) and the grid only bounds how
// many may draw: the ones resident first, one per CU, take all 2^bits buckets, the others draw once and return.
// The half-size kernel (two workgroups per CU) keeps one fixed bucket per workgroup: 47.7 against 47.0 us keys-only at 2^24
// with two, and 6-7 % of a sort of 2^24 lost with drawn ones (profiles/r08_bucket_tickets.txt).
constexpr uint32_t MsdBucketGrid(uint32_t bits, bool halfSizeKernel) { return halfSizeKernel ? 1u << bits : (1u << bits) / 2u; }

// MsdArgs::plainTail: the buckets at the end of the bucket launch that keep plain output stores -- one per CU, the last
// bucket each CU sorts (buckets are handed out in index order, bucket = ticket, so the last `CUs` tickets drawn are the
// highest indices, one for each resident workgroup).  Only their stores lie on the kernel's tail; the write-back of every earlier bucket streams out
// behind the LDS work of the buckets that follow it on the same CU (vrdx_kernels.hip, BucketSort2Body).  Only from
// kMsdStreamedOutputFrom = 2^25 elements, the size the rule was measured at, to the end of the ten-bit plan: buckets of
// 32 K keys and more, whose LDS work is at least as long as the measured one.  Below it (18.1 M ... 2^25: buckets down to
// 18 K keys, half the LDS work to hide a write-back behind) nothing was measured and every bucket keeps plain stores
// (DESIGN.md 5.B).
constexpr uint32_t kMsdStreamedOutputFrom = 1u << 25;
constexpr uint32_t kMsdStreamedOutputUpTo = 36649984u;  // the ten-bit plan's last size (MsdBits; asserted in vrdx_plan.h)
constexpr uint32_t MsdPlainTail(uint32_t computeUnits, uint32_t elementCount, uint32_t bits) {
  return elementCount >= kMsdStreamedOutputFrom && elementCount <= kMsdStreamedOutputUpTo ? computeUnits : 1u << bits;
}

// Runs the device self-check of the LDS same-address atomic ordering on the current device
// (synchronous, ~1 ms).  *laneOrdered = true when returning atomics are served in lane order.
hipError_t LdsOrderCheck(bool* laneOrdered);
// The same check, small (8 workgroups, ~20 us) and stream-ordered: a mismatch sets bit 1 of *sticky.  Never blocks.
hipError_t LaunchLdsOrderRecheck(hipStream_t stream, uint32_t* sticky);
// One wave that runs for `ticks` ticks of the device's constant-rate wall clock and stores its first and last reading.
hipError_t LaunchSpin(hipStream_t stream, unsigned long long* out, uint32_t ticks);

}  // namespace vrdx

#endif  // VRDX_KERNELS_H
