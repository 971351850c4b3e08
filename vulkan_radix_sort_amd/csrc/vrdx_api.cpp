// Host recorder of the HIP backend: the vrdx* entry points of include/vk_radix_sort.h.
//
// Mirrors the reference's host side (src/vk_radix_sort.h.in:141-507) in behaviour:
//   * vrdxCreateSorter builds an immutable sorter and is the only call that can fail;
//   * the storage calculators are the reference's integer formulas, bit for bit;
//   * vrdxCmdSort* validate nothing, allocate nothing, never block the host: they append
//     stream-ordered work to the hipStream_t passed as VkCommandBuffer, the way gpuSort()
//     (:344-507) appends commands to a VkCommandBuffer.
// What differs is the recorded work: 1 clear + 1 fused histogram + 4 onesweep launches (+ the one or two launches of a
// hybrid plan for mid-size sorts) instead of 2 transfers + 12 dispatches + 12 barriers.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vk_radix_sort.h"
#include "../../include/vk_radix_sort_balanced.h"
#include "vrdx_kernels.h"
#include "vrdx_layout.h"
#include "vrdx_plan.h"

struct VrdxSorter_T {
  int device = 0;
  int computeUnits = 0;
  // (tile geometry is chosen per sort from the element count, see ConfigIndex in vrdx_plan.h)
  // LDS returning atomics proven lane-ordered on this device (at creation; vrdxHipRecheck may revise it)
  std::atomic<bool> atomicRank{false};
  // sorts recorded on the general path: behind every 65536th one a small, stream-ordered repeat of the lane-order check
  // is recorded (bit 1 of the sticky word) -- the property is not in the ISA manual, a driver or firmware update under a
  // long-lived process must not turn into silently unstable sorts
  mutable std::atomic<uint32_t> sortsRecorded{0};
  // One device word owned by the sorter: kernels OR their failure bit into it and nothing but
  // vrdxHipReadSorterStatus clears it, so a caller that reuses ONE storage buffer for many sorts (each
  // of which clears the storage's own failure word) still learns about a failure in any of them.
  uint32_t* stickyStatus = nullptr;
  // Second device word, right behind it: MSD plans the DEVICE turned down (a bucket beyond the capacity, a key outside the
  // sampled prefix, a sample that ruled the plan out) -- those sorts ran the four passes recorded behind the plan.  Next to
  // it the number of sorts recorded with the plan in front (host side).  vrdxHipReadPlanCounters.
  uint32_t* declinedPlans = nullptr;
  mutable std::atomic<uint32_t> plansRecorded{0};
  // Host side of the same diagnosis: set when an enqueue of a sort (fill, copy or kernel launch) was
  // refused by the runtime -- the entry points return void, so this is the only place it can go.
  // Reported as bit 31 by vrdxHipReadSorterStatus, which clears it.
  mutable std::atomic<uint32_t> enqueueFailed{0};
  // A sort was recorded with more than VRDX_MAX_ELEMENTS elements and clamped (bit 30 of vrdxHipReadSorterStatus).
  mutable std::atomic<uint32_t> countClamped{0};
  // reference: VrdxSorter_T::minStorageBufferOffsetAlignment (src/vk_radix_sort.h.in:134)
  uint32_t minStorageBufferOffsetAlignment = VRDX_STORAGE_ALIGN;
};

struct VrdxHipQueryPool {
  struct Slot {
    hipEvent_t event = nullptr;
    bool recorded = false;
    // the slot whose event holds this slot's time.  Slots the sort writes back to back, with no device work between
    // them, share ONE event record (an event record costs the stream ~3 us).
    uint32_t source = 0;
  };
  uint32_t count = 0;  // slots whose event exists
  Slot* slots = nullptr;
};

namespace {

int DeviceOrdinalFromHandle(const void* handle, int* ordinal) {
  if (handle == nullptr) return hipGetDevice(ordinal) == hipSuccess ? 0 : -1;
  *ordinal = (int)((uintptr_t)handle - 1);
  return 0;
}

// The environment knobs (tuning / testing only), read once.  VRDX_RANK is not among them: it is read
// whenever a sorter is created or re-checked (RankModeIs).
struct Knobs {
  int forcedConfig = -1;   // VRDX_TILE_CONFIG, e.g. "1024x16": one geometry for everything, and the general path at every size
  bool hybrid = true;      // VRDX_HYBRID=0: always the four-pass plan
  bool msd = true;         // VRDX_MSD=0 (or VRDX_HYBRID=0): no MSD plan
  bool smallSort = true;   // VRDX_SMALL_SORT=0: always the general path
  bool blockSums = true;   // VRDX_BLOCK_SUMS=0: sorts of one round keep the classic look-back (measurements)
  bool debug = false;      // VRDX_DEBUG: report HIP errors of the enqueues on stderr (the entry points themselves return
                           // void and validate nothing, like the reference's vrdxCmd*)
#ifdef VRDX_TESTING
  // test build only.  VRDX_TEST_INJECT_ENQUEUE_ERROR: every EnqueueCheck reports a refusal, the work itself is enqueued as
  // usual (tests/enqueue_error_check.py).  VRDX_TEST_SPIN_LIMIT >= 0: the passes' spin limit; 0 makes the first look-back trip
  // that has to wait give up, how tests/sticky_status_check.py sees the device-side failure path (failure + sticky word)
  bool injectEnqueueError = false;
  int testSpinLimit = -1;
#endif
};

const Knobs& EnvKnobs() {
  static const Knobs knobs = [] {
    Knobs k;
    const auto off = [](const char* name) {
      const char* env = std::getenv(name);
      return env != nullptr && env[0] == '0';
    };
    if (const char* env = std::getenv("VRDX_TILE_CONFIG")) {
      for (int i = 0; i < vrdx::kNumTileConfigs && k.forcedConfig < 0; ++i) {
        char name[32];
        vrdx::ConfigName(vrdx::kTileConfigs[i], name, sizeof(name));
        if (std::strcmp(env, name) == 0) k.forcedConfig = i;
      }
      if (k.forcedConfig < 0) std::fprintf(stderr, "vrdx-hip: unknown VRDX_TILE_CONFIG '%s', using the defaults\n", env);
    }
    k.hybrid = !off("VRDX_HYBRID");
    k.msd = k.hybrid && !off("VRDX_MSD");
    k.smallSort = !off("VRDX_SMALL_SORT");
    if (const char* env = std::getenv("VRDX_BLOCK_SUMS")) k.blockSums = std::atoi(env) != 0;
    k.debug = std::getenv("VRDX_DEBUG") != nullptr;
#ifdef VRDX_TESTING
    k.injectEnqueueError = std::getenv("VRDX_TEST_INJECT_ENQUEUE_ERROR") != nullptr;
    if (const char* env = std::getenv("VRDX_TEST_SPIN_LIMIT")) k.testSpinLimit = std::atoi(env);
#endif
    return k;
  }();
  return knobs;
}

#ifdef VRDX_TRACE
// tools/trace.sh only: one device buffer of 8 stamps per (pass, tile), dumped to $VRDX_TRACE_FILE
// by vrdxDestroySorter.  Holds the LAST sort recorded before the dump.
unsigned long long* g_trace = nullptr;
uint32_t g_traceTiles = 0;
constexpr uint32_t kTraceMaxTiles = 1u << 16;
unsigned long long* TraceBuffer(uint32_t pass, uint32_t tiles) {
  if (g_trace == nullptr) {
    if (hipMalloc(reinterpret_cast<void**>(&g_trace), 4ull * kTraceMaxTiles * 8 * sizeof(unsigned long long)) !=
        hipSuccess)
      return nullptr;
  }
  if (tiles > kTraceMaxTiles) return nullptr;
  g_traceTiles = tiles;
  return g_trace + (size_t)pass * kTraceMaxTiles * 8;
}
void DumpTrace() {
  const char* path = std::getenv("VRDX_TRACE_FILE");
  if (g_trace == nullptr || path == nullptr) return;
  (void)hipDeviceSynchronize();
  const size_t words = 4ull * kTraceMaxTiles * 8;
  unsigned long long* host = new unsigned long long[words];
  if (hipMemcpy(host, g_trace, words * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
    if (FILE* f = std::fopen(path, "wb")) {
      std::fwrite(&g_traceTiles, sizeof(g_traceTiles), 1, f);
      for (uint32_t pass = 0; pass < 4; ++pass)
        std::fwrite(host + (size_t)pass * kTraceMaxTiles * 8, sizeof(unsigned long long), (size_t)g_traceTiles * 8, f);
      std::fclose(f);
    }
  }
  delete[] host;
}
#endif

// What the planner (vrdx_plan.h) is told about this sorter and the environment; built once per recorded sort, with ONE load
// of the ranking mode: one answer for the whole sort.
vrdx::PlanContext PlanContextOf(const VrdxSorter_T* sorter) {
  const Knobs& k = EnvKnobs();
  vrdx::PlanContext c;
  c.computeUnits = sorter->computeUnits;
  c.atomicRank = sorter->atomicRank.load(std::memory_order_relaxed);
  c.minStorageBufferOffsetAlignment = sorter->minStorageBufferOffsetAlignment;
  c.forcedConfig = k.forcedConfig;
  c.hybrid = k.hybrid;
  c.msd = k.msd;
  c.smallSort = k.smallSort;
  c.blockSums = k.blockSums;
  return c;
}

using vrdx::SortPlan;
using vrdx::SortStep;
using vrdx::Step;

inline uint8_t* BufferAddress(VkBuffer buffer, VkDeviceSize offset) {
  return reinterpret_cast<uint8_t*>(buffer) + offset;
}

// After every enqueue of a sort: a launch / fill / copy the runtime REFUSED is latched in the sorter (and
// printed under VRDX_DEBUG).  Only the value returned by that very call is looked at -- never the calling
// thread's last-error state, which is sticky on ROCm and may hold an unrelated, older failure of the caller's.
void EnqueueCheck(const VrdxSorter_T* sorter, const char* what, hipError_t returned) {
#ifdef VRDX_TESTING
  if (EnvKnobs().injectEnqueueError) returned = hipErrorUnknown;
#endif
  if (returned == hipSuccess) return;
  sorter->enqueueFailed.store(1u, std::memory_order_relaxed);
  if (EnvKnobs().debug) std::fprintf(stderr, "vrdx-hip: %s -> %s\n", what, hipGetErrorString(returned));
}

// The 15 timestamp slots of one sort, [query, query + 15) of the pool, written front to back: every slot is either
// stamped by an event of its own behind the step that ends there, or is the same point of the stream as the slot before
// it (nothing enqueued since) and shares that slot's event.
constexpr uint32_t kTimestampSlots = 15;
class StampCursor {
 public:
  StampCursor(VrdxHipQueryPool* pool, uint32_t query, hipStream_t stream) : pool_(pool), query_(query), stream_(stream) { Stamp(0); }
  // everything enqueued so far ends at `slot`: the slots in between coincide with their predecessor
  void AdvanceTo(uint32_t slot) {
    while (++slot_ < slot) StampSame(slot_);
    Stamp(slot);
  }
  void Finish() {  // the end of the sort = the end of its last step
    while (++slot_ < kTimestampSlots) StampSame(slot_);
  }
 private:
  void Stamp(uint32_t slot) {
    const uint32_t q = query_ + slot;
    if (pool_ == nullptr || q >= pool_->count) return;
    if (hipEventRecord(pool_->slots[q].event, stream_) == hipSuccess) {
      pool_->slots[q].recorded = true;
      pool_->slots[q].source = q;
    }
  }
  void StampSame(uint32_t slot) {
    const uint32_t q = query_ + slot;
    if (pool_ == nullptr || q >= pool_->count || !pool_->slots[q - 1].recorded) return;
    pool_->slots[q].recorded = true;
    pool_->slots[q].source = pool_->slots[q - 1].source;
  }
  VrdxHipQueryPool* pool_;
  uint32_t query_;
  hipStream_t stream_;
  uint32_t slot_ = 0;
};

// Launches go to the sorter's device (a Vulkan command buffer belongs to one device too); the
// calling thread's current device is put back afterwards.
struct DeviceScope {
  int previous = -1;
  bool onDevice = false;  // the calling thread's current device is the wanted one
  explicit DeviceScope(int wanted) {
    int current = -1;
    if (hipGetDevice(&current) != hipSuccess) return;
    onDevice = current == wanted;
    if (!onDevice && hipSetDevice(wanted) == hipSuccess) {
      previous = current;
      onDevice = true;
    }
  }
  ~DeviceScope() {
    if (previous >= 0) (void)hipSetDevice(previous);
  }
};

// VRDX_RANK=ballot|atomic|auto, read whenever a sorter is created or re-checked: a process may set it between two sorters.
bool RankModeIs(const char* mode) {
  const char* env = std::getenv("VRDX_RANK");
  return env != nullptr && std::strcmp(env, mode) == 0;
}

// One device word, copied behind everything enqueued on the stream so far (and then cleared in the same stream, if asked
// to), and waited for: the copy targets the caller's variable, so this never returns while it may still be in flight.
// All ones and false when anything failed.
bool ReadDeviceWord(hipStream_t stream, uint32_t* address, uint32_t* word, bool clear = false) {
  const bool copied = hipMemcpyAsync(word, address, sizeof(*word), hipMemcpyDeviceToHost, stream) == hipSuccess;
  const bool cleared = copied && (!clear || hipMemsetAsync(address, 0, sizeof(*word), stream) == hipSuccess);
  const bool ok = copied && hipStreamSynchronize(stream) == hipSuccess && cleared;
  if (!ok) *word = 0xFFFFFFFFu;
  return ok;
}

// Behind every 65536th sort: 8 workgroups repeat the lane-order check of vrdxCreateSorter (~20 us, never blocks; a
// mismatch sets VRDX_HIP_STATUS_RANK_ORDER in the sorter's status word, which vrdxHipReadSorterStatus and
// vrdxDestroySorter report).
// Not into a stream capture: the check would be baked into the graph and run with every replay.  The count is not
// advanced then, so the first sort recorded outside a capture makes up for it.
void MaybeRecheckOrder(VrdxSorter sorter, hipStream_t stream, bool atomicRank) {
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (atomicRank && (sorter->sortsRecorded.load(std::memory_order_relaxed) & 0xFFFFu) == 0xFFFFu &&
      (hipStreamIsCapturing(stream, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone))
    return;
  if (atomicRank && (sorter->sortsRecorded.fetch_add(1u, std::memory_order_relaxed) & 0xFFFFu) == 0xFFFFu)
    EnqueueCheck(sorter, "lds_order_check_kernel", vrdx::LaunchLdsOrderRecheck(stream, sorter->stickyStatus));
}

// The addresses a sort works on: the caller's arrays, the regions of its storage (vrdx_layout.h) and the sorter's two
// device words.  values / valuesScratch: nullptr for a keys-only sort.
struct SortBuffers {
  uint8_t* storage;
  uint32_t *keys, *values;
  const uint32_t* countPtr;  // device-side element count (indirect) or nullptr
  uint32_t *histogram, *status, *tickets, *failure, *planWord, *keysScratch, *valuesScratch;  // regions of the storage
  uint32_t *stickyStatus, *declinedPlans;                                                     // the sorter's device words
};

SortBuffers ResolveBuffers(const VrdxSorter_T* sorter, const vrdx::StorageLayout& layout, uint8_t* storage, uint32_t* keys,
                           uint32_t* values, const uint32_t* countPtr) {
  const auto at = [storage](uint64_t offset) { return reinterpret_cast<uint32_t*>(storage + offset); };
  SortBuffers b;
  b.storage = storage;
  b.keys = keys;
  b.values = values;
  b.countPtr = countPtr;
  b.histogram = at(layout.histogramOffset);
  b.status = at(layout.statusOffset);
  b.tickets = at(layout.ticketOffset);
  b.failure = at(layout.failureOffset);
  b.planWord = at(VRDX_OFF_PLAN);
  b.keysScratch = at(layout.inoutOffset);
  b.valuesScratch = values != nullptr ? at(layout.valuesOffset) : nullptr;
  b.stickyStatus = sorter->stickyStatus;
  b.declinedPlans = sorter->declinedPlans;
  return b;
}

// The arguments of pass `pass` of the four passes (also handed to the MSD plan's launches, whose second role they are).
vrdx::OnesweepArgs PassArgs(const SortPlan& plan, const SortBuffers& b, uint32_t pass) {
  vrdx::OnesweepArgs args;
  // which pair of arrays the pass reads is settled on the device (vrdx_kernels.h); the reference
  // switches in->out to out->in for pass 1, pass 3 (:417-427) and so do four ranking passes here
  args.keysCaller = b.keys;
  args.keysScratch = b.keysScratch;
  args.valuesCaller = b.values;
  args.valuesScratch = b.valuesScratch;
  args.maxCount = plan.elementCount;
  args.countPtr = b.countPtr;
  args.histogramTable = b.histogram;
  // region r of the two: [statusRows tile rows][blockRows block rows]
  const size_t regionWords = (size_t)(plan.layout.regionBytes / sizeof(uint32_t));
  const uint32_t statusRows = (uint32_t)plan.layout.statusRows;
  uint32_t* const regionCur = b.status + (size_t)(pass & 1u) * regionWords;
  uint32_t* const regionNext = b.status + (size_t)((pass + 1) & 1u) * regionWords;
  args.statusCur = regionCur;
  args.statusNext = pass + 1 < VRDX_PASSES ? regionNext : nullptr;
  args.statusRows = statusRows;
  args.blockCur = plan.blockSums ? regionCur + (size_t)statusRows * VRDX_RADIX : nullptr;
  args.blockNext = plan.blockSums ? regionNext + (size_t)statusRows * VRDX_RADIX : nullptr;
  args.blockRows = plan.blockSums ? (uint32_t)plan.layout.blockRows : 0u;
  args.ticketCur = b.tickets + (pass & 1u);
  args.ticketNext = b.tickets + ((pass + 1) & 1u);
  args.failure = b.failure;
  args.stickyFailure = b.stickyStatus;
  args.pass = pass;
  args.hybridCap = plan.hybridCap;
  args.planWord = b.planWord;
  args.spinLimit = vrdx::kSpinLimit;
#ifdef VRDX_TESTING
  if (EnvKnobs().testSpinLimit >= 0) args.spinLimit = (uint32_t)EnvKnobs().testSpinLimit;
#endif
  args.earlyValues = 1u;
  args.planInFront = plan.msdBits != 0 ? 1u : 0u;  // the MSD plan in front may have taken the sort (verdict 3)
  args.slots = plan.tilePlan.slots;
  args.fullTiles = plan.tilePlan.fullTiles;
  args.tailSlots = plan.tilePlan.tailSlots;
  args.trace = nullptr;
#ifdef VRDX_TRACE
  args.trace = TraceBuffer(pass, plan.tilePlan.tiles);
#endif
  return args;
}

// The MSD plan's arguments: spine (prefixes over the tiles, bucket table, verdict), scatter by the window bits, one
// workgroup per bucket; the histogram kernel takes the same structure.
vrdx::MsdArgs MsdArgsOf(const VrdxSorter_T* sorter, const SortPlan& plan, const SortBuffers& b) {
  vrdx::MsdArgs m{};
  m.keysCaller = b.keys;
  m.keysScratch = b.keysScratch;
  m.valuesCaller = b.values;
  m.valuesScratch = b.valuesScratch;
  m.maxCount = plan.elementCount;
  m.countPtr = b.countPtr;
  m.histogramTable = b.histogram;
  m.tileCounts = reinterpret_cast<uint32_t*>(b.storage + plan.layout.msdCountsOffset);
  m.bucketCount = reinterpret_cast<uint32_t*>(b.storage + plan.layout.msdBucketOffset);
  m.bucketBase = m.bucketCount + ((size_t)1 << plan.msdBits);
  m.overflowWord = reinterpret_cast<uint32_t*>(b.storage + VRDX_OFF_MSD_OVERFLOW);
  m.planWord = b.planWord;
  m.bits = plan.msdBits;
  m.cap = plan.msdCap;
  m.tiles = plan.msdTiles;
  m.tileKeys = plan.msdTileKeys;
  m.statusClear = b.storage + plan.layout.statusClearOffset;
  m.statusVecs = (uint32_t)(plan.layout.statusClearBytes / 16u);
  m.plainTail = vrdx::MsdPlainTail((uint32_t)sorter->computeUnits, plan.elementCount, plan.msdBits);
  m.tickets = b.tickets;
  m.declinedPlans = b.declinedPlans;
  return m;
}

vrdx::BucketSortArgs BucketSortArgsOf(const SortPlan& plan, const SortBuffers& b) {
  vrdx::BucketSortArgs a;
  a.keysScratch = b.keysScratch;
  a.keysCaller = b.keys;
  a.valuesScratch = b.valuesScratch;
  a.valuesCaller = b.values;
  a.maxCount = plan.elementCount;
  a.countPtr = b.countPtr;
  a.histogramTable = b.histogram;
  a.hybridCap = plan.hybridCap;
  a.planWord = b.planWord;
  return a;
}

// Enqueues one step of the list; the value the runtime returned for it goes to EnqueueCheck.
hipError_t EnqueueStep(const VrdxSorter_T* sorter, const vrdx::PlanContext& context, hipStream_t stream, const SortPlan& plan, const SortBuffers& b,
                       const vrdx::MsdArgs& msd, const SortStep& step) {
  const bool keyValue = plan.keyValue, atomicRank = plan.atomicRank;
  const uint32_t tiles = plan.tilePlan.tiles;
  switch (step.what) {
    case Step::kFill:
      // Clear count / plan / failure word and the 4x256 global histogram (reference :382) in one fill of 4112 bytes;
      // status region 0 is zeroed by the histogram kernel behind it (MSD plan: by the spine kernel).  With the MSD plan
      // recorded the fill also covers the plan's bucket sizes, 4-8 KiB behind the table: its histogram kernel adds them up.
      // Indirect: also copy the device-side count to where the reference keeps it (:368-379); the kernels themselves
      // read it straight from the caller's buffer.  (Direct: the count travels as a kernel argument, the slot stays 0 --
      // storage contents are scratch.)
      EnqueueCheck(sorter, "hipMemsetAsync(state)", hipMemsetAsync(b.storage, 0, plan.layout.clearBytes, stream));
      if (b.countPtr == nullptr) return hipSuccess;
      return hipMemcpyAsync(b.storage + plan.layout.countOffset, b.countPtr, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
    case Step::kHistogram:
      return vrdx::LaunchHistogram(stream, vrdx::HistogramGrid(context, plan), b.keys, plan.elementCount, b.countPtr, b.histogram, b.tickets,
                                   b.storage + plan.layout.statusClearOffset, (uint32_t)plan.layout.statusClearBytes);
    case Step::kHistogramMsd: return vrdx::LaunchHistogramMsd(stream, vrdx::HistogramGrid(context, plan), msd);
    case Step::kSpineMsd: return vrdx::LaunchSpineMsd(stream, msd);
    case Step::kMsdScatterOrPass0: return vrdx::LaunchMsdFused(stream, false, keyValue, msd, PassArgs(plan, b, 0), tiles);
    case Step::kMsdBucketsOrPass1: return vrdx::LaunchMsdFused(stream, true, keyValue, msd, PassArgs(plan, b, 1), tiles);
    case Step::kBucketSortHalf: return vrdx::LaunchBucketSortHalf(stream, keyValue, msd);
    case Step::kBucketSort: return vrdx::LaunchBucketSort(stream, keyValue, atomicRank, BucketSortArgsOf(plan, b));
    case Step::kPass: return vrdx::LaunchOnesweep(stream, plan.configIndex, tiles, keyValue, atomicRank, PassArgs(plan, b, step.pass));
    case Step::kSmallSort:
      return vrdx::LaunchSmallSort(stream, atomicRank, b.keys, b.values, plan.elementCount, b.countPtr, b.failure);
    // a bit-range sort: the range behind the arguments of the whole-key kernel
    case Step::kSmallSortBits:
      return vrdx::LaunchSmallSortBits(stream, atomicRank, b.keys, b.values, plan.elementCount, b.countPtr, b.failure,
                                       plan.rangeBegin, plan.rangeWidth);
    // an ordered sort: the order word behind the arguments of the one-workgroup kernel | the transforms around the plan
    case Step::kSmallSortOrdered:
      return vrdx::LaunchSmallSortOrdered(stream, atomicRank, b.keys, b.values, plan.elementCount, b.countPtr, b.failure,
                                          plan.order);
    case Step::kOrderForward: return vrdx::LaunchOrder32(stream, false, b.keys, plan.elementCount, b.countPtr, plan.order);
    case Step::kOrderInverse: return vrdx::LaunchOrder32(stream, true, b.keys, plan.elementCount, b.countPtr, plan.order);
  }
  return hipErrorInvalidValue;
}

// What every recorder starts with: the stream, the count clamped to VRDX_MAX_ELEMENTS, the sorter's device and slot 0.
struct Recording {
  hipStream_t stream;
  uint32_t count;  // elementCount / maxElementCount, clamped
  DeviceScope deviceScope;
  StampCursor stamps;
  Recording(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t requested, VkQueryPool queryPool, uint32_t query)
      : stream(reinterpret_cast<hipStream_t>(commandBuffer)),
        count(std::min<uint32_t>(requested, VRDX_MAX_ELEMENTS)),
        deviceScope(sorter->device),
        stamps(reinterpret_cast<VrdxHipQueryPool*>(queryPool), query, stream) {
    // The reference's uint32 byte math wraps above 2^30 - 4 elements (src/vk_radix_sort.h.in:105-115): no storage
    // requirement exists for such a count.  The first 2^30 - 4 elements are sorted, the tail is left alone (segments ending
    // behind the clamped bound are left alone and flagged on the device), and the sorter's status word says so
    // (VRDX_HIP_STATUS_COUNT_CLAMPED) -- like every other failure mode, never silently.
    if (requested > VRDX_MAX_ELEMENTS) sorter->countClamped.store(1u, std::memory_order_relaxed);
  }
  // A refused plan (refusal != nullptr) and an empty one have no step and touch nothing, but every slot of the timestamp
  // contract is recorded whatever the plan (reference: zero partitions -> every dispatch is empty, :353,448,465,487): a
  // caller that reads the pool afterwards must not wait on events that never were.  true: the recorder returns.
  bool NothingToRecord(const VrdxSorter_T* sorter, const char* refusal, uint32_t stepCount) {
    if (refusal == nullptr && stepCount != 0) return false;
    stamps.Finish();
    if (refusal != nullptr) EnqueueCheck(sorter, refusal, hipErrorInvalidValue);
    return true;
  }
};

// reference: gpuSort, src/vk_radix_sort.h.in:344-507
// beginBit, endBit: the whole key for vrdxCmdSort*; vrdxHipCmdSortBits* hand their range on (include/vk_radix_sort.h) -- the
// full range takes the whole-key plan (PlanSortBits forwards it), an empty one has no step, an invalid one and one beyond one
// workgroup's reach are refused.
// order: VRDX_HIP_KEY32_UINT32 for all of those; vrdxHipCmdOrderedSort* hand their order word on (with the whole key):
// PlanOrderedSort, whose transform steps share slot 1 with the fill behind the first and end slot 14 behind pass 3.
void RecordSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount,
                VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                uint32_t query, uint32_t beginBit = 0, uint32_t endBit = 32, uint32_t order = VRDX_HIP_KEY32_UINT32) {
  Recording r(commandBuffer, sorter, elementCount, queryPool, query);
  const bool keyValue = valuesBuffer != nullptr;
  uint8_t* const storage = BufferAddress(storageBuffer, storageOffset);
  const vrdx::PlanContext context = PlanContextOf(sorter);
  const uint64_t storageAddress = (uint64_t)reinterpret_cast<uintptr_t>(storage);
  const SortPlan plan = order != VRDX_HIP_KEY32_UINT32 ? vrdx::PlanOrderedSort(context, keyValue, r.count, order, storageAddress)
                                                       : vrdx::PlanSortBits(context, keyValue, r.count, beginBit, endBit, storageAddress);
  if (r.NothingToRecord(sorter, plan.refusal, plan.stepCount)) return;
  const SortBuffers b = ResolveBuffers(
      sorter, plan.layout, storage, reinterpret_cast<uint32_t*>(BufferAddress(keysBuffer, keysOffset)),
      keyValue ? reinterpret_cast<uint32_t*>(BufferAddress(valuesBuffer, valuesOffset)) : nullptr,
      indirectBuffer != nullptr ? reinterpret_cast<const uint32_t*>(BufferAddress(indirectBuffer, indirectOffset)) : nullptr);
  vrdx::MsdArgs msd{};
  if (plan.msdBits != 0) {
    msd = MsdArgsOf(sorter, plan, b);
    sorter->plansRecorded.fetch_add(1u, std::memory_order_relaxed);
  }
  for (uint32_t i = 0; i < plan.stepCount; ++i) {
    EnqueueCheck(sorter, plan.steps[i].name, EnqueueStep(sorter, context, r.stream, plan, b, msd, plan.steps[i]));
    // (a step that shares its slot with the next one -- the forward transform in front of the fill -- leaves the stamp to it)
    if (i + 1 == plan.stepCount || plan.steps[i + 1].slot != plan.steps[i].slot) r.stamps.AdvanceTo(plan.steps[i].slot);
  }
  r.stamps.Finish();
  if (plan.stepCount > 1) MaybeRecheckOrder(sorter, r.stream, plan.atomicRank);  // (the general path)
}

static_assert(VRDX_HIP_RANGE_SORT_NONE == (uint32_t)vrdx::RangeSortForm::kNone &&
                  VRDX_HIP_RANGE_SORT_ONE_WORKGROUP == (uint32_t)vrdx::RangeSortForm::kOneWorkgroup &&
                  VRDX_HIP_RANGE_SORT_WHOLE_KEY == (uint32_t)vrdx::RangeSortForm::kWholeKey &&
                  VRDX_HIP_RANGE_SORT_CHUNKED == (uint32_t)vrdx::RangeSortForm::kChunked,
              "the forms of the header are the planner's");

// The range sorts at every size (include/vk_radix_sort.h, vrdxHipCmdRangeSort[KeyValue][Indirect]): PlanRangeSort
// (vrdx_plan.h).  Every form but the chunked one IS what vrdxHipCmdSortBits* records and goes through RecordSort, refusals
// included; the chunked form records its own step list on the storage of MakeRangeSortLayout.  Indirect: elementCount is the
// bound; layout and grids come from it alone, and every launch reads the count from the caller's word when it runs.
void RecordRangeSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer indirectBuffer,
                     VkDeviceSize indirectOffset, VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                     VkDeviceSize valuesOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                     VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  const bool keyValue = valuesBuffer != nullptr;
  uint8_t* const storage = BufferAddress(storageBuffer, storageOffset);
  const vrdx::RangeSortPlan plan =
      vrdx::PlanRangeSort(PlanContextOf(sorter), keyValue, std::min<uint32_t>(elementCount, VRDX_MAX_ELEMENTS), beginBit, endBit,
                          (uint64_t)reinterpret_cast<uintptr_t>(storage));
  if (plan.form != vrdx::RangeSortForm::kChunked && plan.refusal == nullptr)
    return RecordSort(commandBuffer, sorter, elementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, valuesBuffer,
                      valuesOffset, storageBuffer, storageOffset, queryPool, query, beginBit, endBit);
  Recording r(commandBuffer, sorter, elementCount, queryPool, query);
  if (r.NothingToRecord(sorter, plan.refusal, plan.stepCount)) return;
  const auto words = [storage](uint64_t offset) { return reinterpret_cast<uint32_t*>(storage + offset); };
  vrdx::RangeSortArgs a;
  a.keys = reinterpret_cast<uint32_t*>(BufferAddress(keysBuffer, keysOffset));
  a.values = keyValue ? reinterpret_cast<uint32_t*>(BufferAddress(valuesBuffer, valuesOffset)) : nullptr;
  a.keysScratch = words(plan.layout.keysScratchOffset);
  a.valuesScratch = keyValue ? words(plan.layout.valuesScratchOffset) : nullptr;
  a.maxCount = r.count;
  a.countPtr = indirectBuffer != nullptr ? reinterpret_cast<const uint32_t*>(BufferAddress(indirectBuffer, indirectOffset)) : nullptr;
  a.totals = words(plan.layout.totalsOffset);
  a.counts = words(plan.layout.countsOffset);
  a.state = words(VRDX_OFF_MSD_OVERFLOW);
  a.grid = plan.grid;
  a.beginBit = plan.rangeBegin;
  a.width = plan.rangeWidth;
  a.pass = 0;
  for (uint32_t i = 0; i < plan.stepCount; ++i) {
    const vrdx::RangeSortStep& step = plan.steps[i];
    a.pass = step.pass;
    hipError_t e = hipErrorInvalidValue;
    switch (step.what) {
      case vrdx::StepRange::kFill:
        // header (count, VRDX_HIP_VERDICT_NONE, the mask of active passes, failure word) and the totals, as RecordSort fills
        // them; indirect: the count is copied to where the reference keeps it
        EnqueueCheck(sorter, "hipMemsetAsync(state)", hipMemsetAsync(storage, 0, plan.layout.clearBytes, r.stream));
        e = a.countPtr == nullptr ? hipSuccess
                                  : hipMemcpyAsync(storage + VRDX_OFF_COUNT, a.countPtr, sizeof(uint32_t), hipMemcpyDeviceToDevice, r.stream);
        break;
      case vrdx::StepRange::kCount: e = vrdx::LaunchRangeCount(r.stream, a); break;
      case vrdx::StepRange::kScan: e = vrdx::LaunchRangeScan(r.stream, a); break;
      case vrdx::StepRange::kScatter: e = vrdx::LaunchRangeScatter(r.stream, keyValue, plan.atomicRank, a); break;
      case vrdx::StepRange::kCopyBack: e = vrdx::LaunchRangeCopyBack(r.stream, keyValue, a); break;
    }
    EnqueueCheck(sorter, step.name, e);
    r.stamps.AdvanceTo(step.slot);
  }
  r.stamps.Finish();
  MaybeRecheckOrder(sorter, r.stream, plan.atomicRank);
}

static_assert(VRDX_HIP_KEY_UINT64 == vrdx::kKeyOrderUint64 && VRDX_HIP_KEY_INT64 == vrdx::kKeyOrderInt64 &&
                  VRDX_HIP_KEY_FLOAT64 == vrdx::kKeyOrderFloat64 && VRDX_HIP_ORDER_DESCENDING == vrdx::kKeyOrderDescending,
              "the order word of the header is the kernels'");
static_assert(VRDX_HIP_KEY32_UINT32 == vrdx::kKeyOrderUint32 && VRDX_HIP_KEY32_INT32 == vrdx::kKeyOrderInt32 &&
                  VRDX_HIP_KEY32_FLOAT32 == vrdx::kKeyOrderFloat32,
              "the 32-bit key types of the header are the kernels'");

// The segmented sorts (include/vk_radix_sort.h, vrdxHipCmdSortSegmented*), all eight entry points: the steps of
// PlanSegmentedSort (vrdx_plan.h) -- a fill and up to three launches -- on the 32-bit storage (Args = SegmentedArgs, Key =
// uint32_t; key: the whole key or the bit range of vrdxHipCmdSortSegmentedBits*) or on the 64-bit storage (Segmented64Args,
// uint64_t; key: the order word, VRDX_HIP_KEY_UINT64 or that of vrdxHipCmdSortSegmented64Ordered*).  On the 32-bit storage the
// whole key may come with an order word too (vrdxHipCmdOrderedSortSegmented*): the ordered forms of the three kernels.
template <typename Args, typename Key>
void RecordSegmentedSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount, uint32_t segmentCount,
                         VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset, VkBuffer keysBuffer, VkDeviceSize keysOffset,
                         VkBuffer valuesBuffer, VkDeviceSize valuesOffset, const vrdx::SegmentedKey& key, VkBuffer storageBuffer,
                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  Recording r(commandBuffer, sorter, maxElementCount, queryPool, query);
  const bool keyValue = valuesBuffer != nullptr;
  uint8_t* const storage = BufferAddress(storageBuffer, storageOffset);
  const vrdx::SegmentedPlan plan = vrdx::PlanSegmentedSort(PlanContextOf(sorter), sizeof(Key), keyValue, r.count, segmentCount, key,
                                                           (uint64_t)reinterpret_cast<uintptr_t>(storage));
  if (r.NothingToRecord(sorter, plan.refusal, plan.stepCount)) return;
  const auto words = [storage](uint64_t offset) { return reinterpret_cast<uint32_t*>(storage + offset); };
  Args a;
  a.keys = reinterpret_cast<Key*>(BufferAddress(keysBuffer, keysOffset));
  a.values = keyValue ? reinterpret_cast<uint32_t*>(BufferAddress(valuesBuffer, valuesOffset)) : nullptr;
  a.keysScratch = reinterpret_cast<Key*>(storage + plan.layout.keysScratchOffset);
  a.valuesScratch = keyValue ? words(plan.layout.valuesScratchOffset) : nullptr;
  a.offsets = reinterpret_cast<const uint32_t*>(BufferAddress(offsetsBuffer, offsetsOffset));
  a.segmentCount = segmentCount;
  a.maxCount = r.count;
  a.midCount = words(plan.layout.midCountOffset);
  a.midList = words(plan.layout.midListOffset);
  a.midCap = plan.layout.midCap;
  a.largeCount = words(plan.layout.largeCountOffset);
  a.largeList = words(plan.layout.largeListOffset);
  a.largeCap = plan.layout.largeCap;
  a.failure = words(VRDX_OFF_FAILURE);
  a.stickyFailure = sorter->stickyStatus;
  for (uint32_t i = 0; i < plan.stepCount; ++i) {
    const vrdx::SegmentedSortStep& step = plan.steps[i];
    const vrdx::SegmentClass sizeClass = vrdx::SegmentClass((int)step.what - (int)vrdx::SegmentedStep::kSmall);
    hipError_t e;
    // header (plan verdict = VRDX_HIP_VERDICT_NONE, failure word) and the two list counters, in front of the first launch
    if (step.what == vrdx::SegmentedStep::kClear)
      e = vrdx::LaunchSegmentedClear(r.stream, a);
    else if constexpr (sizeof(Key) == 8)
      e = vrdx::LaunchSegmented64(r.stream, sizeClass, step.grid, keyValue, plan.atomicRank, a, plan.order);
    else if (plan.order != vrdx::kKeyOrderUint32)
      e = vrdx::LaunchSegmentedOrdered(r.stream, sizeClass, step.grid, keyValue, plan.atomicRank, a, plan.order);
    else
      e = vrdx::LaunchSegmented(r.stream, sizeClass, step.grid, keyValue, plan.atomicRank, a, plan.rangeBegin, plan.rangeWidth);
    EnqueueCheck(sorter, step.name, e);
    r.stamps.AdvanceTo(step.slot);
  }
  r.stamps.Finish();
  MaybeRecheckOrder(sorter, r.stream, plan.atomicRank);
}
constexpr auto RecordSegmentedSort32 = RecordSegmentedSort<vrdx::SegmentedArgs, uint32_t>;
constexpr auto RecordSegmentedSort64 = RecordSegmentedSort<vrdx::Segmented64Args, uint64_t>;

static_assert(VRDX_HIP_BALANCED_NONE == (uint32_t)vrdx::BalancedForm::kNone &&
                  VRDX_HIP_BALANCED_TWIN == (uint32_t)vrdx::BalancedForm::kTwin &&
                  VRDX_HIP_BALANCED_BALANCED == (uint32_t)vrdx::BalancedForm::kBalanced &&
                  VRDX_HIP_BALANCED_SPREAD_FROM == vrdx::kSegSpreadFrom && VRDX_HIP_BALANCED_SPREAD_SHARES == vrdx::kSegSpreadShares,
              "the forms and constants of the header are the planner's");

// The balanced segmented sorts (include/vk_radix_sort.h, vrdxHipCmdBalancedSortSegmented[KeyValue]):
// PlanBalancedSegmentedSort (vrdx_plan.h).  Every form but the balanced one IS what vrdxHipCmdSortSegmented* records and goes
// through RecordSegmentedSort32; the balanced form records its own step list on the storage of MakeBalancedSegmentedLayout.
void RecordBalancedSegmentedSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount, uint32_t segmentCount,
                                 VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset, VkBuffer keysBuffer, VkDeviceSize keysOffset,
                                 VkBuffer valuesBuffer, VkDeviceSize valuesOffset, VkBuffer storageBuffer,
                                 VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  const bool keyValue = valuesBuffer != nullptr;
  uint8_t* const storage = BufferAddress(storageBuffer, storageOffset);
  const vrdx::BalancedSegmentedPlan plan =
      vrdx::PlanBalancedSegmentedSort(PlanContextOf(sorter), keyValue, std::min<uint32_t>(maxElementCount, VRDX_MAX_ELEMENTS),
                                      segmentCount, (uint64_t)reinterpret_cast<uintptr_t>(storage));
  if (plan.form != vrdx::BalancedForm::kBalanced && plan.refusal == nullptr)
    return RecordSegmentedSort32(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer,
                                 keysOffset, valuesBuffer, valuesOffset, {}, storageBuffer, storageOffset, queryPool, query);
  Recording r(commandBuffer, sorter, maxElementCount, queryPool, query);
  if (r.NothingToRecord(sorter, plan.refusal, plan.stepCount)) return;
  const auto words = [storage](uint64_t offset) { return reinterpret_cast<uint32_t*>(storage + offset); };
  const vrdx::SegmentedLayout& lists = plan.layout.lists;
  vrdx::BalancedSegmentedArgs a;
  vrdx::SegmentedArgs& s = a.segmented;
  s.keys = reinterpret_cast<uint32_t*>(BufferAddress(keysBuffer, keysOffset));
  s.values = keyValue ? reinterpret_cast<uint32_t*>(BufferAddress(valuesBuffer, valuesOffset)) : nullptr;
  s.keysScratch = words(lists.keysScratchOffset);
  s.valuesScratch = keyValue ? words(lists.valuesScratchOffset) : nullptr;
  s.offsets = reinterpret_cast<const uint32_t*>(BufferAddress(offsetsBuffer, offsetsOffset));
  s.segmentCount = segmentCount;
  s.maxCount = r.count;
  s.midCount = words(lists.midCountOffset);
  s.midList = words(lists.midListOffset);
  s.midCap = lists.midCap;
  s.largeCount = words(lists.largeCountOffset);
  s.largeList = words(lists.largeListOffset);
  s.largeCap = lists.largeCap;
  s.failure = words(VRDX_OFF_FAILURE);
  s.stickyFailure = sorter->stickyStatus;
  a.split = words(plan.layout.splitOffset);
  a.restCount = a.split + 4;
  a.restList = words(plan.layout.restListOffset);
  a.spreadTable = words(plan.layout.spreadTableOffset);
  a.pieceTable = words(plan.layout.pieceTableOffset);
  a.rows = words(plan.layout.rowsOffset);
  a.spreadCap = plan.layout.spreadCap;
  a.pieceCap = plan.layout.pieceCap;
  a.computeUnits = plan.computeUnits;
  a.pass = 0;
  // the twin's large kernel, unchanged, on the segments that are not spread: only the list and its count differ
  vrdx::SegmentedArgs rest = s;
  rest.largeCount = a.restCount;
  rest.largeList = a.restList;
  for (uint32_t i = 0; i < plan.stepCount; ++i) {
    const vrdx::BalancedSegmentedStep& step = plan.steps[i];
    a.pass = step.pass;
    hipError_t e = hipErrorInvalidValue;
    switch (step.what) {
      case vrdx::StepBalanced::kClear: e = vrdx::LaunchSegmentedClear(r.stream, s); break;
      case vrdx::StepBalanced::kSmall:
        e = vrdx::LaunchSegmented(r.stream, vrdx::kSegmentSmall, step.grid, keyValue, plan.atomicRank, s, 0, 0);
        break;
      case vrdx::StepBalanced::kMid:
        e = vrdx::LaunchSegmented(r.stream, vrdx::kSegmentMid, step.grid, keyValue, plan.atomicRank, s, 0, 0);
        break;
      case vrdx::StepBalanced::kSplit: e = vrdx::LaunchSegmentedSplit(r.stream, a); break;
      case vrdx::StepBalanced::kLargeRest:
        e = vrdx::LaunchSegmented(r.stream, vrdx::kSegmentLarge, step.grid, keyValue, plan.atomicRank, rest, 0, 0);
        break;
      case vrdx::StepBalanced::kCount: e = vrdx::LaunchSegmentedPieceCount(r.stream, a); break;
      case vrdx::StepBalanced::kScan: e = vrdx::LaunchSegmentedPieceScan(r.stream, a); break;
      case vrdx::StepBalanced::kScatter: e = vrdx::LaunchSegmentedPieceScatter(r.stream, keyValue, plan.atomicRank, a); break;
      case vrdx::StepBalanced::kCopyBack: e = vrdx::LaunchSegmentedPieceCopyBack(r.stream, keyValue, a); break;
    }
    EnqueueCheck(sorter, step.name, e);
    // (a step that shares its slot with the next one -- the split, a count -- leaves the stamp to it)
    if (i + 1 == plan.stepCount || plan.steps[i + 1].slot != step.slot) r.stamps.AdvanceTo(step.slot);
  }
  r.stamps.Finish();
  MaybeRecheckOrder(sorter, r.stream, plan.atomicRank);
}

// The 64-bit sorts (include/vk_radix_sort.h, vrdxHipCmdSort64[Ordered][KeyValue][Indirect]): the steps of PlanSort64
// (vrdx_plan.h).  The inner sorts go through RecordSort, without a query pool, on word arrays inside the storage.
// Indirect (indirectBuffer != nullptr): elementCount is the bound; layout, plans and grids come from it alone, and every
// step -- the streaming kernels and, through RecordSort, the inner sorts -- reads the count from the caller's word when it
// runs, so a captured call can be replayed on any count up to the bound.
// order: VRDX_HIP_KEY_UINT64 for vrdxHipCmdSort64*; vrdxHipCmdSort64Ordered* hand their order word on.
void RecordSort64(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer indirectBuffer,
                  VkDeviceSize indirectOffset, VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                  VkDeviceSize valuesOffset, uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                  VkQueryPool queryPool, uint32_t query) {
  Recording r(commandBuffer, sorter, elementCount, queryPool, query);
  const bool keyValue = valuesBuffer != nullptr;
  uint8_t* const storage = BufferAddress(storageBuffer, storageOffset);
  const vrdx::Sort64Plan plan =
      vrdx::PlanSort64(PlanContextOf(sorter), keyValue, r.count, order, (uint64_t)reinterpret_cast<uintptr_t>(storage));
  if (r.NothingToRecord(sorter, plan.refusal, plan.stepCount)) return;
  const vrdx::Sort64Layout& layout = plan.layout;
  const uint32_t n = r.count;
  uint64_t* const keys = reinterpret_cast<uint64_t*>(BufferAddress(keysBuffer, keysOffset));
  uint32_t* const values = keyValue ? reinterpret_cast<uint32_t*>(BufferAddress(valuesBuffer, valuesOffset)) : nullptr;
  uint32_t* const lo = reinterpret_cast<uint32_t*>(storage + layout.loOffset);
  uint32_t* const other = reinterpret_cast<uint32_t*>(storage + layout.otherOffset);
  uint64_t* const keysTemp = reinterpret_cast<uint64_t*>(storage + layout.keysTempOffset);
  const uint32_t* const countPtr =
      indirectBuffer != nullptr ? reinterpret_cast<const uint32_t*>(BufferAddress(indirectBuffer, indirectOffset)) : nullptr;
  // an inner sort: the words at `sortKeys` with those at `payload` as their values, in the storage's front part
  const auto sortWords = [&](uint64_t sortKeys, uint64_t payload) {
    RecordSort(commandBuffer, sorter, n, indirectBuffer, indirectOffset, storageBuffer, storageOffset + sortKeys, storageBuffer,
               storageOffset + payload, storageBuffer, storageOffset, nullptr, 0);
    return hipSuccess;  // (the inner sort has reported its own enqueues)
  };
  for (uint32_t i = 0; i < plan.stepCount; ++i) {
    hipError_t e = hipErrorInvalidValue;
    switch (plan.steps[i].what) {
      case vrdx::Step64::kSplit: e = vrdx::LaunchSplit64(r.stream, keyValue, keys, lo, other, n, countPtr, order); break;
      case vrdx::Step64::kSortLoOther: e = sortWords(layout.loOffset, layout.otherOffset); break;
      case vrdx::Step64::kSortOtherLo: e = sortWords(layout.otherOffset, layout.loOffset); break;
      case vrdx::Step64::kGatherHi: e = vrdx::LaunchGatherHi64(r.stream, keys, other, lo, n, countPtr, order); break;
      case vrdx::Step64::kPermute: e = vrdx::LaunchPermute64(r.stream, keys, values, other, lo, keysTemp, n, countPtr, order); break;
      case vrdx::Step64::kCopyBack: e = vrdx::LaunchCopyBack64(r.stream, keys, values, keysTemp, lo, n, countPtr); break;
      case vrdx::Step64::kMerge: e = vrdx::LaunchMerge64(r.stream, keys, lo, other, n, countPtr, order); break;
    }
    EnqueueCheck(sorter, plan.steps[i].name, e);
    r.stamps.AdvanceTo(plan.steps[i].slot);
  }
  r.stamps.Finish();
}

static_assert(VRDX_HIP_WIDE_VALUE_NONE == (uint32_t)vrdx::WideValueForm::kNone &&
                  VRDX_HIP_WIDE_VALUE_ONE_WORKGROUP == (uint32_t)vrdx::WideValueForm::kOneWorkgroup &&
                  VRDX_HIP_WIDE_VALUE_GATHER == (uint32_t)vrdx::WideValueForm::kGather &&
                  VRDX_HIP_WIDE_VALUE_TWO_SORTS == (uint32_t)vrdx::WideValueForm::kTwoSorts,
              "the forms of the header are the planner's");

// The sorts of 32-bit keys with 64-bit values (include/vk_radix_sort.h, vrdxHipCmdWideValueSort[Indirect]): the steps of
// PlanWideValueSort (vrdx_plan.h).  The inner sorts go through RecordSort, without a query pool, on the caller's keys or on
// their copy, with a word array inside the storage as their values.  Indirect (indirectBuffer != nullptr): elementCount is the
// bound; layout, plan and grids come from it alone, and every step reads the count from the caller's word when it runs.
void RecordWideValueSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer indirectBuffer,
                         VkDeviceSize indirectOffset, VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                         VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                         uint32_t query) {
  Recording r(commandBuffer, sorter, elementCount, queryPool, query);
  uint8_t* const storage = BufferAddress(storageBuffer, storageOffset);
  const vrdx::WideValuePlan plan =
      vrdx::PlanWideValueSort(PlanContextOf(sorter), r.count, (uint64_t)reinterpret_cast<uintptr_t>(storage));
  if (r.NothingToRecord(sorter, nullptr, plan.stepCount)) return;
  const vrdx::WideValueLayout& layout = plan.layout;
  const uint32_t n = r.count;
  uint32_t* const keys = reinterpret_cast<uint32_t*>(BufferAddress(keysBuffer, keysOffset));
  uint64_t* const values = reinterpret_cast<uint64_t*>(BufferAddress(valuesBuffer, valuesOffset));
  uint32_t* const a = reinterpret_cast<uint32_t*>(storage + layout.aOffset);
  uint32_t* const b = reinterpret_cast<uint32_t*>(storage + layout.bOffset);
  uint32_t* const c = reinterpret_cast<uint32_t*>(storage + layout.cOffset);
  uint64_t* const t = reinterpret_cast<uint64_t*>(storage + layout.tOffset);
  const uint32_t* const countPtr =
      indirectBuffer != nullptr ? reinterpret_cast<const uint32_t*>(BufferAddress(indirectBuffer, indirectOffset)) : nullptr;
  // an inner sort: the caller's keys, or the words at `sortKeys` of the storage, with those at `payload` as their values
  const auto sortCallerKeys = [&](uint64_t payload) {
    RecordSort(commandBuffer, sorter, n, indirectBuffer, indirectOffset, keysBuffer, keysOffset, storageBuffer,
               storageOffset + payload, storageBuffer, storageOffset, nullptr, 0);
    return hipSuccess;  // (the inner sort has reported its own enqueues)
  };
  const auto sortWords = [&](uint64_t sortKeys, uint64_t payload) {
    RecordSort(commandBuffer, sorter, n, indirectBuffer, indirectOffset, storageBuffer, storageOffset + sortKeys, storageBuffer,
               storageOffset + payload, storageBuffer, storageOffset, nullptr, 0);
    return hipSuccess;
  };
  for (uint32_t i = 0; i < plan.stepCount; ++i) {
    hipError_t e = hipErrorInvalidValue;
    switch (plan.steps[i].what) {
      case vrdx::StepWide::kSmallSort:
        e = vrdx::LaunchSmallSortWide(r.stream, plan.atomicRank, keys, values, n, countPtr,
                                      reinterpret_cast<uint32_t*>(storage + VRDX_OFF_FAILURE));
        break;
      case vrdx::StepWide::kIota: e = vrdx::LaunchIotaWide(r.stream, a, n, countPtr); break;
      case vrdx::StepWide::kSortKeysA: e = sortCallerKeys(layout.aOffset); break;
      case vrdx::StepWide::kGather: e = vrdx::LaunchGatherWide(r.stream, values, a, t, n, countPtr); break;
      case vrdx::StepWide::kCopyBack: e = vrdx::LaunchCopyBackWide(r.stream, values, t, n, countPtr); break;
      case vrdx::StepWide::kSplit: e = vrdx::LaunchSplitWide(r.stream, keys, values, a, b, c, n, countPtr); break;
      case vrdx::StepWide::kSortAB: e = sortWords(layout.aOffset, layout.bOffset); break;
      case vrdx::StepWide::kSortKeysC: e = sortCallerKeys(layout.cOffset); break;
      case vrdx::StepWide::kMerge: e = vrdx::LaunchMergeWide(r.stream, values, b, c, n, countPtr); break;
    }
    EnqueueCheck(sorter, plan.steps[i].name, e);
    r.stamps.AdvanceTo(plan.steps[i].slot);
  }
  r.stamps.Finish();
}

// The segmented sort of 32-bit keys with 64-bit values (include/vk_radix_sort.h, vrdxHipCmdWideValueSortSegmented): the steps
// of PlanWideValueSortSegmented (vrdx_plan.h) -- a fill and up to three launches -- on the wide-value storage, recorded the
// way RecordSegmentedSort records its own.
void RecordWideValueSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                  uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset, VkBuffer keysBuffer,
                                  VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                  VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  Recording r(commandBuffer, sorter, maxElementCount, queryPool, query);
  uint8_t* const storage = BufferAddress(storageBuffer, storageOffset);
  const vrdx::WideValueSegmentedPlan plan = vrdx::PlanWideValueSortSegmented(
      PlanContextOf(sorter), r.count, segmentCount, (uint64_t)reinterpret_cast<uintptr_t>(storage));
  if (r.NothingToRecord(sorter, plan.refusal, plan.stepCount)) return;
  const auto words = [storage](uint64_t offset) { return reinterpret_cast<uint32_t*>(storage + offset); };
  vrdx::SegmentedWideArgs a;
  a.keys = reinterpret_cast<uint32_t*>(BufferAddress(keysBuffer, keysOffset));
  a.values = reinterpret_cast<uint64_t*>(BufferAddress(valuesBuffer, valuesOffset));
  a.keysScratch = words(plan.layout.keysScratchOffset);
  a.valuesScratch = reinterpret_cast<uint64_t*>(storage + plan.layout.valuesScratchOffset);
  a.offsets = reinterpret_cast<const uint32_t*>(BufferAddress(offsetsBuffer, offsetsOffset));
  a.segmentCount = segmentCount;
  a.maxCount = r.count;
  a.midCount = words(plan.layout.midCountOffset);
  a.midList = words(plan.layout.midListOffset);
  a.midCap = plan.layout.midCap;
  a.largeCount = words(plan.layout.largeCountOffset);
  a.largeList = words(plan.layout.largeListOffset);
  a.largeCap = plan.layout.largeCap;
  a.failure = words(VRDX_OFF_FAILURE);
  a.stickyFailure = sorter->stickyStatus;
  for (uint32_t i = 0; i < plan.stepCount; ++i) {
    const vrdx::SegmentedSortStep& step = plan.steps[i];
    const vrdx::SegmentClass sizeClass = vrdx::SegmentClass((int)step.what - (int)vrdx::SegmentedStep::kSmall);
    // header (plan verdict = VRDX_HIP_VERDICT_NONE, failure word) and the two list counters, in front of the first launch
    const hipError_t e = step.what == vrdx::SegmentedStep::kClear
                             ? vrdx::LaunchSegmentedClear(r.stream, a)
                             : vrdx::LaunchSegmentedWide(r.stream, sizeClass, step.grid, plan.atomicRank, a);
    EnqueueCheck(sorter, step.name, e);
    r.stamps.AdvanceTo(step.slot);
  }
  r.stamps.Finish();
  MaybeRecheckOrder(sorter, r.stream, plan.atomicRank);
}

}  // namespace

extern "C" {

VkResult vrdxCreateSorter(const VrdxSorterCreateInfo* pCreateInfo, VrdxSorter* pSorter) {
  if (pCreateInfo == nullptr || pSorter == nullptr) return VK_ERROR_INITIALIZATION_FAILED;

  int deviceCount = 0;
  if (hipGetDeviceCount(&deviceCount) != hipSuccess || deviceCount <= 0)
    return VK_ERROR_INITIALIZATION_FAILED;

  int ordinal = 0;
  const void* handle = pCreateInfo->device != nullptr ? (const void*)pCreateInfo->device
                                                      : (const void*)pCreateInfo->physicalDevice;
  if (DeviceOrdinalFromHandle(handle, &ordinal) != 0) return VK_ERROR_INITIALIZATION_FAILED;
  if (ordinal < 0 || ordinal >= deviceCount) return VK_ERROR_INITIALIZATION_FAILED;

  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, ordinal) != hipSuccess) return VK_ERROR_INITIALIZATION_FAILED;
  // The code object holds gfx950 ISA only (wave64, 160 KiB LDS, sc1 status protocol).
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return VK_ERROR_FEATURE_NOT_PRESENT;

  VrdxSorter sorter = new (std::nothrow) VrdxSorter_T;
  if (sorter == nullptr) return VK_ERROR_OUT_OF_HOST_MEMORY;
  sorter->device = ordinal;
  sorter->computeUnits = prop.multiProcessorCount;

  DeviceScope deviceScope(ordinal);
  hipError_t e = deviceScope.onDevice ? vrdx::PrepareKernels() : hipErrorInvalidDevice;
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&sorter->stickyStatus), 2 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(sorter->stickyStatus, 0, 2 * sizeof(uint32_t));
  if (e == hipSuccess) sorter->declinedPlans = sorter->stickyStatus + 1;
  if (e == hipSuccess) {
    // Ranking mode: the single-atomic form needs a hardware property the ISA manual does not
    // promise, so it is verified here, once, on this very device; VRDX_RANK=ballot|atomic|auto.
    if (RankModeIs("ballot")) {
      sorter->atomicRank = false;
    } else {
      bool ordered = false;
      e = vrdx::LdsOrderCheck(&ordered);
      sorter->atomicRank = ordered;
      if (e == hipSuccess && !ordered) {
        // Never silent: the ballot form is correct everywhere but 1.2-1.7x slower (profiles/r03_ballot_ranking.txt).
        std::fprintf(stderr,
                     "vrdx-hip: LDS returning atomics are not lane-ordered on device %d: ranking with wave ballots "
                     "instead (same results, 1.2-1.7x the time)%s\n",
                     ordinal, RankModeIs("atomic") ? "; VRDX_RANK=atomic refused" : "");
      }
    }
  }
  if (e != hipSuccess) {
    if (sorter->stickyStatus != nullptr) (void)hipFree(sorter->stickyStatus);
    delete sorter;  // reference cleanup(): nothing half-built survives (:153-158)
    return VK_ERROR_INITIALIZATION_FAILED;
  }

  *pSorter = sorter;
  return VK_SUCCESS;
}

void vrdxDestroySorter(VrdxSorter sorter) {
  if (sorter == nullptr) return;  // reference :268
#ifdef VRDX_TRACE
  DumpTrace();
#endif
  // Last chance to be heard: the vrdxCmdSort* entry points return void like the reference's, so a caller that never
  // asks vrdxHipReadSorterStatus would not learn that a sort gave up a look-back (result unspecified), that the
  // lane-order re-check failed or that the runtime refused an enqueue.  One line on stderr, only if something did.
  if (sorter->stickyStatus != nullptr) {
    // on the sorter's device, whatever the calling thread's current one is (one thread may own a sorter per GPU)
    DeviceScope deviceScope(sorter->device);
    uint32_t word = 0;
    if (hipMemcpy(&word, sorter->stickyStatus, sizeof(word), hipMemcpyDeviceToHost) != hipSuccess) word = 0;  // (synchronises)
    if (sorter->enqueueFailed.load(std::memory_order_relaxed) != 0) word |= VRDX_HIP_STATUS_ENQUEUE_REFUSED;
    if (sorter->countClamped.load(std::memory_order_relaxed) != 0) word |= VRDX_HIP_STATUS_COUNT_CLAMPED;
    if (word != 0)
      std::fprintf(stderr,
                   "vrdx-hip: sorter destroyed with unreported failures (status 0x%08x:%s%s%s%s%s) -- see vrdxHipReadSorterStatus\n",
                   word, (word & VRDX_HIP_STATUS_LOOKBACK_GAVE_UP) ? " a look-back spin expired, that sort's result is unspecified;" : "",
                   (word & VRDX_HIP_STATUS_RANK_ORDER) ? " LDS atomics were seen out of lane order, call vrdxHipRecheck;" : "",
                   (word & VRDX_HIP_STATUS_SEGMENTS_INVALID) ? " a segmented sort met offsets that decrease or end behind maxElementCount, those segments were left alone;" : "",
                   (word & VRDX_HIP_STATUS_COUNT_CLAMPED) ? " an element count beyond 2^30 - 4 was clamped, that sort's tail is unsorted;" : "",
                   (word & VRDX_HIP_STATUS_ENQUEUE_REFUSED) ? " the HIP runtime refused an enqueue;" : "");
    (void)hipFree(sorter->stickyStatus);
  }
  delete sorter;
}

void vrdxGetSorterStorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                      VrdxSorterStorageRequirements* requirements) {
  const vrdx::StorageLayout layout =
      vrdx::MakeLayout(maxElementCount, sorter->minStorageBufferOffsetAlignment, 0);  // the size is the reference's formula
  requirements->size = layout.keysOnlySize;
  requirements->usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT | VK_BUFFER_USAGE_TRANSFER_DST_BIT;
}

void vrdxGetSorterKeyValueStorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                              VrdxSorterStorageRequirements* requirements) {
  const vrdx::StorageLayout layout =
      vrdx::MakeLayout(maxElementCount, sorter->minStorageBufferOffsetAlignment, 0);
  requirements->size = layout.keyValueSize;
  requirements->usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT | VK_BUFFER_USAGE_TRANSFER_DST_BIT;
}

void vrdxCmdSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount,
                 VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer storageBuffer,
                 VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, nullptr, 0,
             storageBuffer, storageOffset, queryPool, query);
}

void vrdxCmdSortIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                         VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                         VkDeviceSize keysOffset, VkBuffer storageBuffer,
                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer,
             keysOffset, nullptr, 0, storageBuffer, storageOffset, queryPool, query);
}

void vrdxCmdSortKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount,
                         VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                         VkDeviceSize valuesOffset, VkBuffer storageBuffer,
                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, valuesBuffer,
             valuesOffset, storageBuffer, storageOffset, queryPool, query);
}

void vrdxCmdSortKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter,
                                 uint32_t maxElementCount, VkBuffer indirectBuffer,
                                 VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                 VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                 VkDeviceSize valuesOffset, VkBuffer storageBuffer,
                                 VkDeviceSize storageOffset, VkQueryPool queryPool,
                                 uint32_t query) {
  RecordSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer,
             keysOffset, valuesBuffer, valuesOffset, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                             uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                             VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer storageBuffer,
                             VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort32(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer, keysOffset,
                        nullptr, 0, {}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSortSegmentedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                     uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                     VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                     VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                     VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort32(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer, keysOffset,
                        valuesBuffer, valuesOffset, {}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdBalancedSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                     uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                     VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer storageBuffer,
                                     VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordBalancedSegmentedSort(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer,
                              keysOffset, nullptr, 0, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdBalancedSortSegmentedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                             uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                             VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                             VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                             VkQueryPool queryPool, uint32_t query) {
  RecordBalancedSegmentedSort(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer,
                              keysOffset, valuesBuffer, valuesOffset, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipDescribeBalancedSegmentedPlan(VrdxSorter sorter, uint32_t maxElementCount, uint32_t segmentCount, int keyValue,
                                          VrdxHipBalancedSegmentedPlanInfo* info) {
  if (info == nullptr) return;
  std::memset(info, 0, sizeof(*info));
  if (sorter == nullptr) return;
  if (maxElementCount > VRDX_MAX_ELEMENTS) maxElementCount = VRDX_MAX_ELEMENTS;
  vrdx::DescribeBalancedSegmentedPlan(
      vrdx::PlanBalancedSegmentedSort(PlanContextOf(sorter), keyValue != 0, maxElementCount, segmentCount, 0), info);
}

VkResult vrdxHipReadBalancedSplit(VkCommandBuffer commandBuffer, VrdxSorter sorter, VkBuffer storageBuffer,
                                  VkDeviceSize storageOffset, uint32_t maxElementCount, VrdxHipBalancedSplitInfo* info) {
  if (info == nullptr || sorter == nullptr) return VK_ERROR_INITIALIZATION_FAILED;
  std::memset(info, 0, sizeof(*info));
  if (maxElementCount > VRDX_MAX_ELEMENTS) maxElementCount = VRDX_MAX_ELEMENTS;
  uint8_t* const storage = BufferAddress(storageBuffer, storageOffset);
  // (the offset of the words depends on neither the form of the values nor the segment count)
  const vrdx::BalancedSegmentedPlan plan = vrdx::PlanBalancedSegmentedSort(PlanContextOf(sorter), false, maxElementCount, 1,
                                                                           (uint64_t)reinterpret_cast<uintptr_t>(storage));
  if (plan.form != vrdx::BalancedForm::kBalanced) return VK_SUCCESS;
  DeviceScope deviceScope(sorter->device);
  hipStream_t stream = reinterpret_cast<hipStream_t>(commandBuffer);
  uint32_t words[4];
  if (hipMemcpyAsync(words, storage + plan.layout.splitOffset, sizeof(words), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return VK_ERROR_DEVICE_LOST;
  info->listedSegments = words[0];
  info->spreadSegments = words[1];
  info->pieces = words[2];
  info->pieceKeys = words[3];
  return VK_SUCCESS;
}

void vrdxHipCmdSortSegmentedBits(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                 uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                 VkBuffer keysBuffer, VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit,
                                 VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort32(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer, keysOffset,
                        nullptr, 0, {beginBit, endBit}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSortSegmentedBitsKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                         uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                         VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                         VkDeviceSize valuesOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort32(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer, keysOffset,
                        valuesBuffer, valuesOffset, {beginBit, endBit}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSortSegmented64(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                               uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                               VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer storageBuffer,
                               VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort64(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer,
                        keysOffset, nullptr, 0, {}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSortSegmented64KeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                       uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                       VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                       VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                       VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort64(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer,
                        keysOffset, valuesBuffer, valuesOffset, {}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSortSegmented64Ordered(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                      uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                      VkBuffer keysBuffer, VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer,
                                      VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort64(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer,
                        keysOffset, nullptr, 0, {0, 32, order}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSortSegmented64OrderedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                              uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                              VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                              VkDeviceSize valuesOffset, uint32_t order, VkBuffer storageBuffer,
                                              VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort64(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer,
                        keysOffset, valuesBuffer, valuesOffset, {0, 32, order}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSortBits(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                        VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                        VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, nullptr, 0, storageBuffer, storageOffset,
             queryPool, query, beginBit, endBit);
}

void vrdxHipCmdSortBitsKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                                VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset, uint32_t beginBit,
                                uint32_t endBit, VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                                uint32_t query) {
  RecordSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, valuesBuffer, valuesOffset, storageBuffer,
             storageOffset, queryPool, query, beginBit, endBit);
}

void vrdxHipCmdSortBitsIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                                VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, nullptr, 0,
             storageBuffer, storageOffset, queryPool, query, beginBit, endBit);
}

void vrdxHipCmdSortBitsKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                        VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                        VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                        uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                        VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, valuesBuffer,
             valuesOffset, storageBuffer, storageOffset, queryPool, query, beginBit, endBit);
}

void vrdxHipCmdRangeSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                         VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordRangeSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, nullptr, 0, beginBit, endBit,
                  storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdRangeSortKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                                 VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset, uint32_t beginBit,
                                 uint32_t endBit, VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                                 uint32_t query) {
  RecordRangeSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, valuesBuffer, valuesOffset, beginBit,
                  endBit, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdRangeSortIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                 VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                 VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                                 VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordRangeSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, nullptr, 0,
                  beginBit, endBit, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdRangeSortKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                         VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                         VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                         uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                         VkQueryPool queryPool, uint32_t query) {
  RecordRangeSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, valuesBuffer,
                  valuesOffset, beginBit, endBit, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipGetSorter64StorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                           VrdxSorterStorageRequirements* requirements) {
  requirements->size = vrdx::MakeSort64Layout(maxElementCount, sorter->minStorageBufferOffsetAlignment).keysOnlySize;
  requirements->usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT | VK_BUFFER_USAGE_TRANSFER_DST_BIT;
}

void vrdxHipGetSorter64KeyValueStorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                                   VrdxSorterStorageRequirements* requirements) {
  requirements->size = vrdx::MakeSort64Layout(maxElementCount, sorter->minStorageBufferOffsetAlignment).keyValueSize;
  requirements->usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT | VK_BUFFER_USAGE_TRANSFER_DST_BIT;
}

void vrdxHipCmdSort64(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                      VkDeviceSize keysOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                      uint32_t query) {
  RecordSort64(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, nullptr, 0, VRDX_HIP_KEY_UINT64,
               storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSort64KeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                              VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                              VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort64(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, valuesBuffer, valuesOffset,
               VRDX_HIP_KEY_UINT64, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSort64Indirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                              VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                              VkDeviceSize keysOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                              VkQueryPool queryPool, uint32_t query) {
  RecordSort64(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, nullptr, 0,
               VRDX_HIP_KEY_UINT64, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSort64KeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                      VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                      VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                      VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                                      uint32_t query) {
  RecordSort64(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, valuesBuffer,
               valuesOffset, VRDX_HIP_KEY_UINT64, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSort64Ordered(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                             VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                             VkQueryPool queryPool, uint32_t query) {
  RecordSort64(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, nullptr, 0, order, storageBuffer,
               storageOffset, queryPool, query);
}

void vrdxHipCmdSort64OrderedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount,
                                     VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                     VkDeviceSize valuesOffset, uint32_t order, VkBuffer storageBuffer,
                                     VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort64(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, valuesBuffer, valuesOffset, order,
               storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSort64OrderedIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                     VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                     VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer,
                                     VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort64(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, nullptr, 0,
               order, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdSort64OrderedKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                             VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                             VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                             uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                             VkQueryPool queryPool, uint32_t query) {
  RecordSort64(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, valuesBuffer,
               valuesOffset, order, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdOrderedSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                           VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                           VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, nullptr, 0, storageBuffer, storageOffset,
             queryPool, query, 0, 32, order);
}

void vrdxHipCmdOrderedSortKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                                   VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset, uint32_t order,
                                   VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, valuesBuffer, valuesOffset, storageBuffer,
             storageOffset, queryPool, query, 0, 32, order);
}

void vrdxHipCmdOrderedSortIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                   VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                   VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                   VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, nullptr, 0,
             storageBuffer, storageOffset, queryPool, query, 0, 32, order);
}

void vrdxHipCmdOrderedSortKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                           VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                           VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                           uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                           VkQueryPool queryPool, uint32_t query) {
  RecordSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset, valuesBuffer,
             valuesOffset, storageBuffer, storageOffset, queryPool, query, 0, 32, order);
}

void vrdxHipCmdOrderedSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                    uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                    VkBuffer keysBuffer, VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer,
                                    VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort32(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer, keysOffset,
                        nullptr, 0, {0, 32, order}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdOrderedSortSegmentedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                            uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                            VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                            VkDeviceSize valuesOffset, uint32_t order, VkBuffer storageBuffer,
                                            VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordSegmentedSort32(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer, keysOffset,
                        valuesBuffer, valuesOffset, {0, 32, order}, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipGetSorterWideValueStorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                                  VrdxSorterStorageRequirements* requirements) {
  requirements->size = vrdx::MakeWideValueLayout(maxElementCount, sorter->minStorageBufferOffsetAlignment).size;
  requirements->usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT | VK_BUFFER_USAGE_TRANSFER_DST_BIT;
}

void vrdxHipCmdWideValueSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                             VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                             VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query) {
  RecordWideValueSort(commandBuffer, sorter, elementCount, nullptr, 0, keysBuffer, keysOffset, valuesBuffer, valuesOffset,
                      storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipCmdWideValueSortIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                     VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                     VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                     VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                                     uint32_t query) {
  RecordWideValueSort(commandBuffer, sorter, maxElementCount, indirectBuffer, indirectOffset, keysBuffer, keysOffset,
                      valuesBuffer, valuesOffset, storageBuffer, storageOffset, queryPool, query);
}

void vrdxHipDescribeWideValueSortPlan(VrdxSorter sorter, uint32_t elementCount, VrdxHipWideValuePlanInfo* info) {
  if (info == nullptr) return;
  std::memset(info, 0, sizeof(*info));
  if (sorter == nullptr) return;
  if (elementCount > VRDX_MAX_ELEMENTS) elementCount = VRDX_MAX_ELEMENTS;
  const vrdx::PlanContext context = PlanContextOf(sorter);
  vrdx::DescribeWideValuePlan(context, vrdx::PlanWideValueSort(context, elementCount, 0), info);
}

void vrdxHipCmdWideValueSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                      uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                      VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                      VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                      VkQueryPool queryPool, uint32_t query) {
  RecordWideValueSortSegmented(commandBuffer, sorter, maxElementCount, segmentCount, offsetsBuffer, offsetsOffset, keysBuffer,
                               keysOffset, valuesBuffer, valuesOffset, storageBuffer, storageOffset, queryPool, query);
}

VkResult vrdxHipCreateQueryPool(uint32_t queryCount, VkQueryPool* pQueryPool) {
  if (pQueryPool == nullptr || queryCount == 0) return VK_ERROR_INITIALIZATION_FAILED;
  VrdxHipQueryPool* pool = new (std::nothrow) VrdxHipQueryPool;
  if (pool != nullptr) pool->slots = new (std::nothrow) VrdxHipQueryPool::Slot[queryCount];
  VkResult result = pool != nullptr && pool->slots != nullptr ? VK_SUCCESS : VK_ERROR_OUT_OF_HOST_MEMORY;
  for (uint32_t i = 0; result == VK_SUCCESS && i < queryCount; ++i) {
    pool->slots[i].source = i;
    if (hipEventCreate(&pool->slots[i].event) == hipSuccess)
      pool->count = i + 1;
    else
      result = VK_ERROR_INITIALIZATION_FAILED;
  }
  if (result != VK_SUCCESS) {
    vrdxHipDestroyQueryPool(reinterpret_cast<VkQueryPool>(pool));  // (whatever part of it exists)
    return result;
  }
  *pQueryPool = reinterpret_cast<VkQueryPool>(pool);
  return VK_SUCCESS;
}

void vrdxHipDestroyQueryPool(VkQueryPool queryPool) {
  VrdxHipQueryPool* pool = reinterpret_cast<VrdxHipQueryPool*>(queryPool);
  if (pool == nullptr) return;
  for (uint32_t i = 0; i < pool->count; ++i) (void)hipEventDestroy(pool->slots[i].event);
  delete[] pool->slots;
  delete pool;
}

VkResult vrdxHipGetQueryPoolResults(VkQueryPool queryPool, uint32_t firstQuery, uint32_t queryCount,
                                    uint64_t* pData) {
  VrdxHipQueryPool* pool = reinterpret_cast<VrdxHipQueryPool*>(queryPool);
  if (pool == nullptr || pData == nullptr || firstQuery + queryCount > pool->count)
    return VK_ERROR_INITIALIZATION_FAILED;
  for (uint32_t i = 0; i < queryCount; ++i) {
    if (!pool->slots[firstQuery + i].recorded) return VK_NOT_READY;
    float ms = 0.0f;
    const hipError_t e = hipEventElapsedTime(&ms, pool->slots[pool->slots[firstQuery].source].event,
                                             pool->slots[pool->slots[firstQuery + i].source].event);
    if (e == hipErrorNotReady) return VK_NOT_READY;
    if (e != hipSuccess) return VK_ERROR_DEVICE_LOST;
    pData[i] = ms <= 0.0f ? 0ull : (uint64_t)((double)ms * 1.0e6 + 0.5);
  }
  return VK_SUCCESS;
}

uint32_t vrdxHipReadStatus(VkCommandBuffer commandBuffer, VkBuffer storageBuffer,
                           VkDeviceSize storageOffset) {
  uint32_t word;
  ReadDeviceWord(reinterpret_cast<hipStream_t>(commandBuffer),
                 reinterpret_cast<uint32_t*>(BufferAddress(storageBuffer, storageOffset) + VRDX_OFF_FAILURE), &word);
  return word;
}

uint32_t vrdxHipReadSorterStatus(VrdxSorter sorter, VkCommandBuffer commandBuffer) {
  if (sorter == nullptr || sorter->stickyStatus == nullptr) return 0xFFFFFFFFu;
  uint32_t word;
  if (!ReadDeviceWord(reinterpret_cast<hipStream_t>(commandBuffer), sorter->stickyStatus, &word, true)) return word;
  if (sorter->enqueueFailed.exchange(0u, std::memory_order_relaxed) != 0) word |= VRDX_HIP_STATUS_ENQUEUE_REFUSED;
  if (sorter->countClamped.exchange(0u, std::memory_order_relaxed) != 0) word |= VRDX_HIP_STATUS_COUNT_CLAMPED;
  return word;
}

VkResult vrdxHipRecheck(VrdxSorter sorter) {
  if (sorter == nullptr) return VK_ERROR_INITIALIZATION_FAILED;
  if (RankModeIs("ballot")) return VK_SUCCESS;  // nothing rests on the property
  DeviceScope deviceScope(sorter->device);
  bool ordered = false;
  if (!deviceScope.onDevice || vrdx::LdsOrderCheck(&ordered) != hipSuccess) return VK_ERROR_DEVICE_LOST;
  const bool was = sorter->atomicRank.exchange(ordered, std::memory_order_relaxed);
  if (was && !ordered)
    std::fprintf(stderr,
                 "vrdx-hip: LDS returning atomics are no longer lane-ordered on device %d: sorts recorded from now on rank "
                 "with wave ballots (same results, 1.2-1.7x the time); results of earlier sorts may be unstable\n",
                 sorter->device);
  return VK_SUCCESS;
}

uint64_t vrdxHipEventOverheadNs(VkCommandBuffer commandBuffer) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(commandBuffer);
  int device = 0, clockKhz = 0;
  unsigned long long* stamps = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint64_t result = ~0ull;
  // the stream's device, not the calling thread's current one (the null stream: the current device)
  if ((stream != nullptr ? hipStreamGetDevice(stream, &device) : hipGetDevice(&device)) != hipSuccess ||
      hipDeviceGetAttribute(&clockKhz, hipDeviceAttributeWallClockRate, device) != hipSuccess || clockKhz <= 0)
    return result;
  DeviceScope deviceScope(device);
  if (hipMalloc(reinterpret_cast<void**>(&stamps), 2 * sizeof(unsigned long long)) != hipSuccess) return result;
  if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
    // a kernel that demonstrably runs 40 us, right behind another one (a busy stream, like the passes of a sort)
    const uint32_t ticks = (uint32_t)(40ull * (uint64_t)clockKhz / 1000ull);
    std::vector<uint64_t> extra;
    for (int run = 0; run < 9; ++run) {
      unsigned long long host[2] = {0, 0};
      float ms = 0.0f;
      if (vrdx::LaunchSpin(stream, stamps, ticks) != hipSuccess || hipEventRecord(e0, stream) != hipSuccess ||
          vrdx::LaunchSpin(stream, stamps, ticks) != hipSuccess || hipEventRecord(e1, stream) != hipSuccess ||
          hipStreamSynchronize(stream) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess ||
          hipMemcpy(host, stamps, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess)
        break;
      const double ran = (double)(host[1] - host[0]) * 1.0e6 / (double)clockKhz;  // ns
      const double between = (double)ms * 1.0e6;
      if (run > 0) extra.push_back(between > ran ? (uint64_t)(between - ran + 0.5) : 0ull);
    }
    if (!extra.empty()) {
      std::sort(extra.begin(), extra.end());
      result = extra[extra.size() / 2];
    }
  }
  if (e0 != nullptr) (void)hipEventDestroy(e0);
  if (e1 != nullptr) (void)hipEventDestroy(e1);
  (void)hipFree(stamps);
  return result;
}

void vrdxHipDescribePlan(VrdxSorter sorter, uint32_t elementCount, int keyValue, VrdxHipPlanInfo* info) {
  if (info == nullptr) return;
  std::memset(info, 0, sizeof(*info));
  if (sorter == nullptr || elementCount == 0) return;
  if (elementCount > VRDX_MAX_ELEMENTS) elementCount = VRDX_MAX_ELEMENTS;
  // the recorder's own planning function (storage address 0: the alignment at which the least fits)
  vrdx::DescribePlan(vrdx::PlanSort(PlanContextOf(sorter), keyValue != 0, elementCount, 0), info);
}

void vrdxHipDescribeSortBitsPlan(VrdxSorter sorter, uint32_t elementCount, int keyValue, uint32_t beginBit, uint32_t endBit,
                                 VrdxHipPlanInfo* info) {
  if (info == nullptr) return;
  std::memset(info, 0, sizeof(*info));
  if (sorter == nullptr) return;
  if (elementCount > VRDX_MAX_ELEMENTS) elementCount = VRDX_MAX_ELEMENTS;
  const SortPlan plan = vrdx::PlanSortBits(PlanContextOf(sorter), keyValue != 0, elementCount, beginBit, endBit, 0);
  if (plan.stepCount != 0) vrdx::DescribePlan(plan, info);  // (no step: refused -- an invalid range, one beyond one workgroup -- or empty)
}

void vrdxHipDescribeRangeSortPlan(VrdxSorter sorter, uint32_t elementCount, int keyValue, uint32_t beginBit, uint32_t endBit,
                                  VrdxHipRangeSortPlanInfo* info) {
  if (info == nullptr) return;
  std::memset(info, 0, sizeof(*info));
  if (sorter == nullptr) return;
  if (elementCount > VRDX_MAX_ELEMENTS) elementCount = VRDX_MAX_ELEMENTS;
  vrdx::DescribeRangeSortPlan(vrdx::PlanRangeSort(PlanContextOf(sorter), keyValue != 0, elementCount, beginBit, endBit, 0), info);
}

void vrdxHipDescribeOrderedSortPlan(VrdxSorter sorter, uint32_t elementCount, int keyValue, uint32_t order, VrdxHipPlanInfo* info) {
  if (info == nullptr) return;
  std::memset(info, 0, sizeof(*info));
  if (sorter == nullptr) return;
  if (elementCount > VRDX_MAX_ELEMENTS) elementCount = VRDX_MAX_ELEMENTS;
  const SortPlan plan = vrdx::PlanOrderedSort(PlanContextOf(sorter), keyValue != 0, elementCount, order, 0);
  if (plan.stepCount == 0) return;  // (refused -- an invalid order word -- or empty)
  vrdx::DescribePlan(plan, info);
  if (plan.order != vrdx::kKeyOrderUint32 && !plan.oneWorkgroup) {
    // the two transforms (counted among the launches): each reads and writes every key once
    info->bytesPerElement += 16u;
    info->fallbackBytesPerElement += 16u;
  }
}

uint32_t vrdxHipReadPlanVerdict(VkCommandBuffer commandBuffer, VkBuffer storageBuffer, VkDeviceSize storageOffset) {
  uint32_t word;
  if (!ReadDeviceWord(reinterpret_cast<hipStream_t>(commandBuffer),
                      reinterpret_cast<uint32_t*>(BufferAddress(storageBuffer, storageOffset) + VRDX_OFF_PLAN), &word))
    return word;
  return word & vrdx::kMsdVerdictMask;  // (the MSD plan's scatter also notes its window's shift there, bits 8-13)
}

VkResult vrdxHipReadPlanCounters(VrdxSorter sorter, VkCommandBuffer commandBuffer, uint32_t* pRecorded, uint32_t* pDeclined) {
  if (sorter == nullptr || sorter->declinedPlans == nullptr) return VK_ERROR_INITIALIZATION_FAILED;
  uint32_t declined;
  if (!ReadDeviceWord(reinterpret_cast<hipStream_t>(commandBuffer), sorter->declinedPlans, &declined)) return VK_ERROR_DEVICE_LOST;
  if (pRecorded != nullptr) *pRecorded = sorter->plansRecorded.load(std::memory_order_relaxed);
  if (pDeclined != nullptr) *pDeclined = declined;
  return VK_SUCCESS;
}

const char* vrdxHipVersionString(void) {
  // built once (thread-safe static initialisation), never rewritten: concurrent callers read one immutable buffer
  struct Text {
    char text[160];
    Text() {
      vrdx::PlanContext nominal{256, true};  // an MI355X: 256 CUs, lane-ordered LDS atomics
      nominal.forcedConfig = EnvKnobs().forcedConfig;
      char kName[32], kvName[32];
      vrdx::ConfigName(vrdx::kTileConfigs[vrdx::ConfigIndex(nominal, false, 1u << 25)], kName, sizeof(kName));
      vrdx::ConfigName(vrdx::kTileConfigs[vrdx::ConfigIndex(nominal, true, 1u << 25)], kvName, sizeof(kvName));
      std::snprintf(text, sizeof(text), "vrdx-hip %d.%d.%d gfx950 tiles at 2^25: keys=%s key-value=%s%s",
                    VRDX_VERSION_MAJOR, VRDX_VERSION_MINOR, VRDX_VERSION_PATCH, kName, kvName,
                    EnvKnobs().forcedConfig >= 0 ? " (forced)" : " (size-adaptive)");
    }
  };
  static const Text once;
  return once.text;
}

}  // extern "C"
