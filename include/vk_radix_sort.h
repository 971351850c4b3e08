/*
 * vk_radix_sort.h -- MI355X (gfx950 / HIP) backend behind the VrdxSorter / vrdxCmdSort* surface.
 *
 * This is the drop-in boundary: a C-ABI shared library (libvrdx_hip.so) exporting the eight
 * entry points the reference declares at src/vk_radix_sort.h.in:24-81 (generated copy
 * include/vk_radix_sort.h:24-81), with the same names, parameter order and parameter types.
 * The reference is a header-only C++ library whose declarations have C++ linkage; here they are
 * `extern "C"` so that any FFI (ctypes, cgo, JNI, N-API) can bind them.
 *
 * Vulkan handle types keep their reference spelling.  When <vulkan/vulkan_core.h> is available it
 * is used; otherwise the minimal shim below supplies ABI-identical typedefs (every dispatchable
 * and non-dispatchable handle is an 8-byte pointer on 64-bit targets).
 *
 * HIP meaning of each handle:
 *   VkPhysicalDevice / VkDevice : HIP device ordinal, encoded with VRDX_HIP_DEVICE(ordinal);
 *                                 VK_NULL_HANDLE = the calling thread's current HIP device.
 *   VkPipelineCache             : ignored (kernels are precompiled for gfx950; no JIT).
 *   VkCommandBuffer             : hipStream_t.  "Recording" is a stream-ordered enqueue; nothing
 *                                 blocks the host, and the calls are legal inside
 *                                 hipStreamBeginCapture/EndCapture (hipGraph) when queryPool is NULL.
 *   VkBuffer + VkDeviceSize     : device pointer + byte offset.
 *   VkQueryPool                 : VrdxHipQueryPool (array of hipEvent_t), see vrdxHipCreateQueryPool.
 *
 * All arithmetic on this path is 32-bit unsigned integer; keys are sorted ascending, the sort is
 * stable, and results land back in keysBuffer / valuesBuffer.  How many trips through memory a sort
 * makes is the library's business and depends on its size (vrdxHipDescribePlan): one workgroup up to
 * 16384 elements; one scatter + one in-LDS sort per bucket (two trips) up to 67.1 M elements when the
 * device finds that every bucket fits; four ping-pong passes like the reference's otherwise.
 */
#ifndef VK_RADIX_SORT_H
#define VK_RADIX_SORT_H

#include <stdint.h>

#if defined(__has_include)
#if __has_include(<vulkan/vulkan_core.h>)
#include <vulkan/vulkan_core.h>
#define VRDX_HAVE_VULKAN_CORE 1
#endif
#endif

#ifndef VRDX_HAVE_VULKAN_CORE
/* ---- minimal Vulkan type shim (ABI-identical to vulkan_core.h on LP64) ---- */
#ifndef VK_DEFINE_HANDLE
#define VK_DEFINE_HANDLE(object) typedef struct object##_T* object;
#endif
#ifndef VK_NULL_HANDLE
#define VK_NULL_HANDLE 0
#endif
typedef struct VkPhysicalDevice_T* VkPhysicalDevice;
typedef struct VkDevice_T* VkDevice;
typedef struct VkPipelineCache_T* VkPipelineCache;
typedef struct VkCommandBuffer_T* VkCommandBuffer;
typedef struct VkBuffer_T* VkBuffer;
typedef struct VkQueryPool_T* VkQueryPool;
typedef uint64_t VkDeviceSize;
typedef uint32_t VkFlags;
typedef VkFlags VkBufferUsageFlags;
typedef enum VkResult {
  VK_SUCCESS = 0,
  VK_NOT_READY = 1,
  VK_ERROR_OUT_OF_HOST_MEMORY = -1,
  VK_ERROR_OUT_OF_DEVICE_MEMORY = -2,
  VK_ERROR_INITIALIZATION_FAILED = -3,
  VK_ERROR_DEVICE_LOST = -4,
  VK_ERROR_FEATURE_NOT_PRESENT = -8,
  VK_RESULT_MAX_ENUM = 0x7FFFFFFF
} VkResult;
#define VK_BUFFER_USAGE_TRANSFER_DST_BIT 0x00000002
#define VK_BUFFER_USAGE_STORAGE_BUFFER_BIT 0x00000020
#endif /* !VRDX_HAVE_VULKAN_CORE */

/* reference: src/vk_radix_sort.h.in:6-9 (v0.4.0, CMakeLists.txt:3) */
#define VRDX_VERSION_MAJOR 0
#define VRDX_VERSION_MINOR 4
#define VRDX_VERSION_PATCH 0
#define VRDX_VERSION ((VRDX_VERSION_MAJOR << 22) | (VRDX_VERSION_MINOR << 12) | VRDX_VERSION_PATCH)

/* HIP device ordinal <-> VkDevice / VkPhysicalDevice encoding (ordinal + 1 so that 0 stays NULL). */
#define VRDX_HIP_DEVICE(ordinal) ((VkDevice)(uintptr_t)((ordinal) + 1))
#define VRDX_HIP_PHYSICAL_DEVICE(ordinal) ((VkPhysicalDevice)(uintptr_t)((ordinal) + 1))

#ifdef __cplusplus
extern "C" {
#endif

struct VrdxSorter_T;

/* reference: src/vk_radix_sort.h.in:11-16 -- VrdxSorter owns the (precompiled) kernels' launch
 * configuration for one device; immutable after creation. */
VK_DEFINE_HANDLE(VrdxSorter)

/* reference: src/vk_radix_sort.h.in:18-22 */
typedef struct VrdxSorterCreateInfo {
  VkPhysicalDevice physicalDevice;
  VkDevice device;
  VkPipelineCache pipelineCache;
} VrdxSorterCreateInfo;

/* reference: src/vk_radix_sort.h.in:24,141-265.  Returns VK_SUCCESS, or
 * VK_ERROR_INITIALIZATION_FAILED (no usable HIP device / ordinal out of range),
 * VK_ERROR_FEATURE_NOT_PRESENT (device is not gfx950), VK_ERROR_OUT_OF_HOST_MEMORY.
 * On failure *pSorter is left untouched and nothing is leaked (reference cleanup(), :153-158). */
VkResult vrdxCreateSorter(const VrdxSorterCreateInfo* pCreateInfo, VrdxSorter* pSorter);

/* reference: src/vk_radix_sort.h.in:26,267-277.  NULL-safe. */
void vrdxDestroySorter(VrdxSorter sorter);

/* reference: src/vk_radix_sort.h.in:28-31 */
typedef struct VrdxSorterStorageRequirements {
  VkDeviceSize size;
  VkBufferUsageFlags usage;
} VrdxSorterStorageRequirements;

/* reference: src/vk_radix_sort.h.in:33,279-292.  Same formula, bit for bit:
 *   size = Align(4,A) + HistogramSize(N,A) + InoutSize(N,A), usage = STORAGE_BUFFER|TRANSFER_DST. */
void vrdxGetSorterStorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                      VrdxSorterStorageRequirements* requirements);

/* reference: src/vk_radix_sort.h.in:36,294-308.
 *   size = Align(4,A) + HistogramSize + Align(InoutSize,A) + InoutSize. */
void vrdxGetSorterKeyValueStorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                              VrdxSorterStorageRequirements* requirements);

/**
 * reference: src/vk_radix_sort.h.in:39-54,310-315.
 *
 * if queryPool is not VK_NULL_HANDLE, it records timestamps into N entries [query..query+N-1].
 *
 * N=15 (same slot contract as the reference):
 * query + 0: start
 * query + 1: after the state clear ("transfer")
 * query + 2 + (3 * i) + 0: upsweep of pass i
 * query + 2 + (3 * i) + 1: spine of pass i
 * query + 2 + (3 * i) + 2: downsweep of pass i
 * query + 14: sort end
 *
 * What lies between two slots here, by the plan vrdxHipDescribePlan reports (slots that have no stage of
 * their own coincide with the slot before them, so every difference is >= 0 and ts[14] - ts[0] is the sort):
 *   FOUR_PASSES   [1,2] the fused 4-digit histogram; [3 i + 3, 3 i + 4] pass i (rank + look-back + scatter in
 *                 one kernel: the "spine" slot 3 i + 3 coincides with the "upsweep" slot 3 i + 2, and that one
 *                 with the previous pass's "downsweep" slot for i > 0)
 *   HYBRID8       the same, plus [4,5] = one workgroup per bucket (pass 1's "upsweep"); passes 1-3 return at once
 *                 when the device takes the plan
 *   MSD           [1,2] histogram (it also chooses the window); [2,3] spine; [3,4] scatter by the
 *                 window bits; [4,5] one workgroup per bucket; the passes that are launches of their own follow
 *                 and return at once when the device takes the plan: [9,10] pass 2, [12,13] pass 3, and [6,7] pass 1
 *                 where it is a launch (sorts of up to 18.1 M elements: the half-size bucket kernel has no second
 *                 role).  Pass 0 is a second role of the scatter launch, and beyond 18.1 M pass 1 one of the bucket
 *                 launch -- when the device turns the plan down, [3,4] IS pass 0 and [4,5] pass 1
 *   ONE_WORKGROUP [13,14] the one kernel
 *
 * Alignment and bounds, for vrdxCmdSort, vrdxCmdSortIndirect, vrdxCmdSortKeyValue and vrdxCmdSortKeyValueIndirect alike:
 *   keysBuffer + keysOffset, valuesBuffer + valuesOffset and indirectBuffer + indirectOffset are multiples of 4.  Nothing
 *   more is required of them: an array may start at any uint32 of a larger allocation (keys + 1, a packed batch), and keys,
 *   values and the count need not share a residue mod 16.
 *   storageBuffer + storageOffset is a multiple of 16.
 *   Nothing outside [0, elementCount) of the caller's arrays is written -- with a device-side count, nothing from
 *   min(count, maxElementCount) on -- and nothing outside the storage requirement; the count word is only read.
 */
void vrdxCmdSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount,
                 VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer storageBuffer,
                 VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);

/* reference: src/vk_radix_sort.h.in:55-58,317-323 */
void vrdxCmdSortIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                         VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                         VkDeviceSize keysOffset, VkBuffer storageBuffer,
                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);

/* reference: src/vk_radix_sort.h.in:60-63,325-331 */
void vrdxCmdSortKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount,
                         VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                         VkDeviceSize valuesOffset, VkBuffer storageBuffer,
                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);

/**
 * reference: src/vk_radix_sort.h.in:65-81,333-342.
 *
 * indirectBuffer contains elementCount: a uint32_t read on the device from
 * indirectBuffer + indirectOffset when the sort executes.  It must not exceed maxElementCount
 * (values above it are clamped).  Keys, values and the count may live in one buffer at different
 * offsets (bench/vulkan_benchmark.cc:386-388).
 */
void vrdxCmdSortKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter,
                                 uint32_t maxElementCount, VkBuffer indirectBuffer,
                                 VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                 VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                 VkDeviceSize valuesOffset, VkBuffer storageBuffer,
                                 VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);

/**
 * Segmented sort (not part of the reference API): segmentCount independent arrays in one recorded call.
 *
 * Offsets: offsetsBuffer + offsetsOffset holds segmentCount + 1 uint32 offsets o[] in CSR form; segment i is the elements
 * [o[i], o[i+1]) of keysBuffer (and valuesBuffer).  The offsets are read ON THE DEVICE when the sort runs, never by the host:
 * the call does not block, and a sort captured into a hipGraph may be replayed on another segmentation with the same
 * segmentCount.
 * Order: every segment is sorted ascending as uint32, stably; values travel with their keys.  Elements before o[0] and from
 * o[segmentCount] on are not touched.
 * Storage: what vrdxGetSorter[KeyValue]StorageRequirements(maxElementCount) returns; one sort in flight per storage.
 * Alignment: keysBuffer + keysOffset, valuesBuffer + valuesOffset and offsetsBuffer + offsetsOffset are multiples of 4, and
 * nothing more is required of them; storageBuffer + storageOffset is a multiple of 16.
 * Bad offsets: a segment with o[i] > o[i+1] or o[i+1] > maxElementCount is left alone and the sort raises
 * VRDX_HIP_STATUS_SEGMENTS_INVALID in the storage's failure word (vrdxHipReadStatus) and in the sorter's word
 * (vrdxHipReadSorterStatus).  Any offsets that are not monotone raise it, so a clear bit means every segment was sorted (with
 * the bit raised, valid segments that overlap each other are unspecified).  Nothing is ever written outside
 * [0, maxElementCount) of the caller's arrays or outside the storage requirement.
 * segmentCount == 0 or maxElementCount == 0 records nothing but the timestamps; maxElementCount > 2^30 - 4 is clamped
 * (VRDX_HIP_STATUS_COUNT_CLAMPED).  Word 1 of the storage reads VRDX_HIP_VERDICT_NONE after the sort.
 * Sizes are classed on the device: up to 4096 elements one 256-thread workgroup sorts the segment in LDS, up to 16384 one
 * 1024-thread workgroup, beyond that one workgroup runs an LSD sort through memory (the segment's index range of the
 * storage's scratch arrays) -- a few segments of millions of keys are faster with one vrdxCmdSort each.
 *
 * Timestamps (all 15 slots recorded; ts[14] - ts[0] is the sort):
 *   [0,1] the fill of the storage header and list counters
 *   [1,2] the 256-thread launch over every segment (sorts those of <= 4096 elements, lists the others)
 *   [2,3] the 1024-thread in-LDS launch over the listed segments of 4097 ... 16384 elements (3 == 2 when maxElementCount < 4097)
 *   [3,4] the launch over the listed segments of more than 16384 elements (4 == 3 when maxElementCount < 16385)
 *   slots 5 ... 14 coincide with slot 4
 */
void vrdxHipCmdSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                             uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                             VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer storageBuffer,
                             VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSortSegmentedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                     uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                     VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                     VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                     VkQueryPool queryPool, uint32_t query);

/**
 * 64-bit keys (not part of the reference API): elementCount uint64 keys, with or without one uint32 value each.
 *
 * Keys and values: keysBuffer + keysOffset holds uint64 keys and is a multiple of 8; valuesBuffer + valuesOffset holds uint32
 * values and is a multiple of 4.
 * Order: ascending as unsigned 64-bit, stable; results land back in the caller's arrays.  Elements from elementCount on are
 * never touched, and nothing is written outside the storage requirement.
 * How: two of this library's stable 32-bit key+value sorts, the low words first and the high words second, each carrying the
 * other word (keys-only) or the element's index (key+value) as its value -- four trips through memory where the plans of
 * vrdxHipDescribePlan(elementCount, 1) take two each, and a word that is the same in every key costs next to nothing.
 *   keys-only   split (A = low words, B = high words); sort (A, B); sort (B, A); merge (keys = B << 32 | A)
 *   key+value   split (A = low words, I = 0, 1, 2, ...); sort (A, I); gather (A = high word of keys[I]); sort (A, I);
 *               permute (T = A << 32 | low word of keys[I], A = values[I]); copy back (keys = T, values = A)
 * Storage: vrdxHipGetSorter64[KeyValue]StorageRequirements(maxElementCount); storageOffset is a multiple of 16 as for every
 * sort, one sort in flight per storage.  It is vrdxGetSorterKeyValueStorageRequirements(maxElementCount) bytes, used by
 * both inner sorts, then up to 112 bytes of padding, then the word arrays on 128-byte lines: A and B / I (4 bytes per
 * element each), and for key+value T (8 bytes per element).  On top of the 32-bit key+value requirement that is 8 bytes per
 * element keys-only and 16 bytes per element key+value.
 * Recording: the call never blocks and reads no data on the host; with a NULL query pool it is legal inside a stream capture,
 * and the captured graph may be replayed on other data of the same count.
 * Counts: elementCount == 0 records nothing but the timestamps; elementCount > 2^30 - 4 is clamped
 * (VRDX_HIP_STATUS_COUNT_CLAMPED).
 * Status: the inner sorts' header is the front of this storage, and each inner sort clears it, so vrdxHipReadStatus and
 * vrdxHipReadPlanVerdict on this storage report the SECOND inner sort (the high words).  vrdxHipReadSorterStatus covers both,
 * as it does for any two sorts.
 *
 * Timestamps (all 15 slots recorded; ts[14] - ts[0] is the call; the inner sorts are recorded without a pool):
 *   [0,1] the split
 *   [1,2] the first sort (low words)
 *   [2,3] key+value: the gather of the high words (keys-only: 3 == 2)
 *   [3,4] the second sort (high words)
 *   [4,5] keys-only: the merge; key+value: the permutation of keys and values into the storage
 *   [5,6] key+value: the copy back into the caller's arrays (keys-only: 6 == 5)
 *   slots 7 ... 14 coincide with slot 6
 *
 * Signed, float64 and descending orders: vrdxHipCmdSort64Ordered* below, in the same kernels and at no extra trip over the
 * keys.
 * Out of scope, each left to the caller: values wider than 32 bits (sort an index as the value and gather by it); keys wider
 * than 64 bits (sort by the low 64 bits, then by the high ones: every sort here is stable).
 * Many independent arrays of 64-bit keys: vrdxHipCmdSortSegmented64 below.
 */
void vrdxHipGetSorter64StorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                           VrdxSorterStorageRequirements* requirements);
void vrdxHipGetSorter64KeyValueStorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                                   VrdxSorterStorageRequirements* requirements);
void vrdxHipCmdSort64(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                      VkDeviceSize keysOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                      uint32_t query);
void vrdxHipCmdSort64KeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                              VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                              VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);

/**
 * 64-bit keys by a device-side count: vrdxHipCmdSort64[KeyValue] with the element count read on the device, parameters in
 * the order of vrdxCmdSort[KeyValue]Indirect.  A pipeline that learns its count on the GPU (a prefix sum, a compaction) sorts
 * without reading it back, and one captured call serves every count up to the bound.
 *
 * Count: one uint32 at indirectBuffer + indirectOffset, a multiple of 4.  Every step reads it on the device when it runs; the
 * host never reads it.  Values above maxElementCount are clamped to it, silently, as vrdxCmdSort*Indirect does.  The word may
 * share a buffer with the keys or the values at another offset; it must not lie inside the storage range.  Nothing writes
 * it.
 * Effect: with n = min(count, maxElementCount), elements [0, n) of the keys (and values) end up sorted ascending as unsigned
 * 64-bit and stable -- exactly what vrdxHipCmdSort64[KeyValue](..., n, ...) leaves.  Elements from n on are neither read nor
 * written, also where n == 0, and nothing is written outside the storage requirement.
 * Storage: vrdxHipGetSorter64[KeyValue]StorageRequirements(maxElementCount), carved as for the direct forms.
 * Plans and grids depend on maxElementCount only: the inner sorts take the plan of maxElementCount, as vrdxCmdSort*Indirect
 * does, and the steps around them start one thread per four elements of the bound, of which those from n on return.  With a
 * NULL query pool the call is legal inside a stream capture, and the captured graph may be replayed on any count up to the
 * bound and any data.
 * Counts: maxElementCount == 0 records nothing but the timestamps; maxElementCount > 2^30 - 4 is clamped
 * (VRDX_HIP_STATUS_COUNT_CLAMPED).
 * Timestamps and status: as for the direct forms -- the same assignment of slots [0,6], all 15 recorded; vrdxHipReadStatus and
 * vrdxHipReadPlanVerdict on this storage report the second inner sort.
 */
void vrdxHipCmdSort64Indirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                              VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                              VkDeviceSize keysOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                              VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSort64KeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                      VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                      VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                      VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                                      uint32_t query);

/**
 * Segmented sort of 64-bit keys (not part of the reference API): vrdxHipCmdSortSegmented[KeyValue] with uint64 keys,
 * parameters in the same order.  Native kernels, not a chain of the 32-bit entry points: a segment that fits a workgroup's
 * LDS is loaded once, ranked by up to eight bytes inside the workgroup and stored once.
 *
 * Data: keysBuffer + keysOffset holds uint64 keys and is a multiple of 8; valuesBuffer + valuesOffset holds one uint32 value
 * per key and is a multiple of 4; offsetsBuffer + offsetsOffset holds segmentCount + 1 uint32 offsets o[] in CSR form, read on
 * the device only; nothing writes them.
 * Order: every segment [o[i], o[i+1]) is sorted ascending as unsigned 64-bit, stably; values travel with their keys.
 * Untouched elements: elements before o[0], from o[segmentCount] on, and in segments of fewer than 2 elements are not written
 * at all (not rewritten with their own value).
 * Bad offsets: as for the 32-bit form -- a segment with o[i] > o[i+1] or o[i+1] > maxElementCount is left alone and raises
 * VRDX_HIP_STATUS_SEGMENTS_INVALID in the storage's failure word and in the sorter's word; any offsets that are not monotone
 * raise it (with the bit raised, valid segments that overlap each other are unspecified).  Nothing is ever written outside
 * [0, maxElementCount) of the caller's arrays or outside the storage requirement.
 * Storage: vrdxHipGetSorter64[KeyValue]StorageRequirements(maxElementCount); storageOffset is a multiple of 16, one sort in
 * flight per storage.  Header words 0-3, the two list counters and the lists lie where the 32-bit segmented sort keeps them
 * (inside the front part, vrdxGetSorterKeyValueStorageRequirements(maxElementCount) bytes); behind that, on 128-byte lines, one
 * 8-byte scratch key per element where the 64-bit sorts keep A and B, and for key+value one 4-byte scratch value per element
 * where they keep T.  Word 1 reads VRDX_HIP_VERDICT_NONE after the sort.
 * Recording: the call never blocks and reads nothing on the host; grids depend on segmentCount, maxElementCount and the CU
 * count only; with a NULL query pool it is legal inside a stream capture, and the captured graph may be replayed on other keys
 * and another segmentation with the same segmentCount.  segmentCount == 0 or maxElementCount == 0 records nothing but the
 * timestamps; maxElementCount > 2^30 - 4 is clamped (VRDX_HIP_STATUS_COUNT_CLAMPED).
 * Sizes are classed on the device.  Up to 4096 keys one 256-thread workgroup sorts the segment in LDS; up to 16384 keys
 * (keys-only) or 8192 elements (key+value: 12 bytes x 16384 do not fit the LDS) one 1024-thread workgroup does; beyond that one
 * workgroup runs an LSD sort through memory in tiles of 8192 elements, between the segment and its index range of the
 * scratch arrays.  In every class a byte that is the same in all keys of a segment costs no pass, so keys of fewer than 64
 * significant bits (tile id << 32 | depth) take fewer than eight.  One workgroup sorts a large segment, so a few huge
 * segments leave most of the device idle: 64 segments of 262144 keys take 1.4 ms on an MI355X, a third of one
 * vrdxHipCmdSort64 per segment, and the loop wins once the segments are far larger.
 *
 * Timestamps (all 15 slots recorded; ts[14] - ts[0] is the sort):
 *   [0,1] the fill of the storage header and list counters
 *   [1,2] the 256-thread launch over every segment (sorts those of <= 4096 elements, lists the others)
 *   [2,3] the 1024-thread in-LDS launch over the listed mid segments (3 == 2 when maxElementCount < 4097)
 *   [3,4] the launch over the listed large segments (4 == 3 when maxElementCount < 16385 keys-only, < 8193 key+value)
 *   slots 5 ... 14 coincide with slot 4
 */
void vrdxHipCmdSortSegmented64(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                               uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                               VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer storageBuffer,
                               VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSortSegmented64KeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                       uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                       VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                       VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                       VkQueryPool queryPool, uint32_t query);

/**
 * Key orders of the 64-bit sorts (not part of the reference API): the six 64-bit calls above with one order word, `order`,
 * right behind the keys (and values) arguments -- the position beginBit / endBit have in vrdxHipCmdSortBits* -- and
 * everything else in the order of the matching call.  int64 and float64 keys, ascending or descending, at no extra trip
 * over the keys: the kernels that take the keys apart and put them together, and the segmented kernels between their load
 * and their store, apply the order where the key is in registers anyway.
 *
 * The order word: one key type, VRDX_HIP_KEY_UINT64, VRDX_HIP_KEY_INT64 or VRDX_HIP_KEY_FLOAT64, with
 * VRDX_HIP_ORDER_DESCENDING or-ed in or not.
 * Order: let T(k) = k ^ flip ^ (FLOAT64 and bit 63 of k set ? 0x7FFFFFFFFFFFFFFF : 0) on the key's 64 bits, with flip = 0 for
 * UINT64, 1 << 63 for INT64 and FLOAT64, and the complement of that for descending.  After the call the elements (of every
 * segment) are in ascending unsigned order of T(key).  T is a bijection, so:
 *   UINT64, INT64   ascending (descending) as unsigned, as two's-complement signed integers;
 *   FLOAT64         IEEE-754 totalOrder on the bits: NaNs with the sign bit set first, then -inf ... -0.0, then +0.0 ... +inf,
 *                   NaNs with the sign bit clear last, NaNs among themselves by their payload bits; descending is the reverse;
 *   stability       elements of EQUAL key keep their input order, for descending too (not the reverse of the ascending
 *                   result): what CUB's SortKeysDescending / SortPairsDescending and a stable torch.sort(descending=True) give;
 *   keys come back bit for bit as they went in, values travel with their keys.
 * FLOAT64 differs from torch.sort (and numpy.sort) in two ways: torch.sort puts ALL NaNs last (first when descending),
 * whatever their sign bit, and treats -0.0 and +0.0 as equal, leaving them in input order; here -0.0 sorts in front of +0.0.
 * On keys without NaNs and without zeros of both signs the two agree.
 * Everything else is the twin's, word for word: the storage (vrdxHipGetSorter64[KeyValue]StorageRequirements), the alignment
 * rules, the device-side count of the indirect forms and its clamp, untouched elements, bad offsets
 * (VRDX_HIP_STATUS_SEGMENTS_INVALID), the clamp at 2^30 - 4, the timestamp slots, the status and verdict words, capture and
 * replay.
 *   order == VRDX_HIP_KEY_UINT64 records exactly what the twin records: the same kernels, bit for bit the same work.
 *   An order word with any other bit set, or a key type above VRDX_HIP_KEY_FLOAT64, is refused like an invalid bit range: the
 *   timestamps are recorded, nothing else is touched, and the sorter's word raises VRDX_HIP_STATUS_ENQUEUE_REFUSED.
 * Out of scope: orders for the bit-range sorts; ranges for the 64-bit sorts.  Orders for the 32-bit sorts (int32, float32,
 * descending): vrdxHipCmdOrderedSort* below.
 */
#define VRDX_HIP_KEY_UINT64 0u
#define VRDX_HIP_KEY_INT64 1u
#define VRDX_HIP_KEY_FLOAT64 2u
#define VRDX_HIP_ORDER_DESCENDING 0x100u
void vrdxHipCmdSort64Ordered(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                             VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                             VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSort64OrderedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount,
                                     VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                     VkDeviceSize valuesOffset, uint32_t order, VkBuffer storageBuffer,
                                     VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSort64OrderedIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                     VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                     VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer,
                                     VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSort64OrderedKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                             VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                             VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                             uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                             VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSortSegmented64Ordered(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                      uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                      VkBuffer keysBuffer, VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer,
                                      VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSortSegmented64OrderedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                              uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                              VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                              VkDeviceSize valuesOffset, uint32_t order, VkBuffer storageBuffer,
                                              VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);

/**
 * Sort by a bit range of the key (not part of the reference API; the begin_bit / end_bit of CUB, hipCUB and rocPRIM): the
 * four whole-key calls with beginBit and endBit right behind the keys (and values) arguments, everything else in the
 * order of the matching whole-key call.
 *
 * Order: let f(k) = (k >> beginBit) & (2^(endBit - beginBit) - 1).  After the call, elements [0, n) are the input elements in
 * ascending order of f(key); elements with equal f keep their input order; keys are moved WHOLE -- the bits outside the
 * range are carried along untouched and never compared -- and values travel with their keys.  The keys-only calls are
 * stable in the same sense, which is observable: the bits outside the range tell keys of equal field apart.  (Sorting
 * masked keys is not the same thing: a key that packs its sort field next to a payload or a second field -- cell id |
 * flags, depth | id, a class bit above an index -- has to come back whole, and equal fields in input order are what makes
 * multi-field LSD compositions and stable partitions by a flag work.)
 * Valid ranges: 0 <= beginBit <= endBit <= 32.
 *   beginBit == endBit is the empty range: like elementCount == 0 it records nothing but the timestamps and touches neither
 *   the arrays nor the storage.
 *   beginBit == 0 and endBit == 32 IS the matching whole-key call: every plan applies, behaviour is the same bit for bit.
 *   beginBit > endBit or endBit > 32 is refused like a storage layout that does not fit: the timestamps are recorded, nothing
 *   else is touched, and the sorter's word raises VRDX_HIP_STATUS_ENQUEUE_REFUSED.
 * Storage, alignment and bounds: exactly as for the whole-key calls -- vrdxGetSorter[KeyValue]StorageRequirements(
 * maxElementCount), the same alignment rules, nothing written outside [0, n) of the caller's arrays or outside the
 * storage requirement.
 * Count: the indirect forms read the count on the device and clamp it to the bound; the count word is only read.
 * maxElementCount > 2^30 - 4 is clamped (VRDX_HIP_STATUS_COUNT_CLAMPED).
 * Capture: with a NULL query pool the calls are legal inside a stream capture; the graph may be replayed on other data and,
 * for the indirect forms, on other counts up to the bound.
 * Status: vrdxHipReadStatus works on the storage.  Word 1 reads VRDX_HIP_VERDICT_NONE after any range sort that had
 * elements, also on storage where an MSD sort left its verdict.
 * Size: range sorts run in ONE workgroup and one launch, which ranks the P = ceil((endBit - beginBit) / 8) digits of the
 * range (the last one of the bits that are left) -- up to 16384 elements (maxElementCount for the indirect forms).  A call
 * with more elements and a range other than [0, 32) is REFUSED like an invalid range: the timestamps are recorded, nothing
 * else is touched, VRDX_HIP_STATUS_ENQUEUE_REFUSED is raised.  vrdxHipDescribeSortBitsPlan reports ONE_WORKGROUP (8 / 16 bytes
 * per element) for what is sorted and VRDX_HIP_PLAN_NONE for what is refused.  Range sorts ignore VRDX_SMALL_SORT and
 * VRDX_TILE_CONFIG: size alone decides; only the range [0, 32), which is the whole-key sort, follows them.
 * Timestamps: the 15-slot contract as for ONE_WORKGROUP above.
 *
 * Beyond 16384 elements: vrdxHipCmdRangeSort* below take the same arguments and sort every size (these calls keep their
 * refusal: the range forms of the histogram and pass kernels are not part of this library).
 * Out of scope: ranges for the 64-bit sorts; a range combined with a descending, signed or
 * floating-point order (whole 32-bit keys have those orders: vrdxHipCmdOrderedSort* below).
 * Ranges for the segmented sort: vrdxHipCmdSortSegmentedBits below.
 */
void vrdxHipCmdSortBits(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                        VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                        VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSortBitsKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                                VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset, uint32_t beginBit,
                                uint32_t endBit, VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                                uint32_t query);
void vrdxHipCmdSortBitsIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                                VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSortBitsKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                        VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                        VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                        uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                        VkQueryPool queryPool, uint32_t query);

/**
 * Range sort at every size (not part of the reference API): vrdxHipCmdSortBits[KeyValue][Indirect]
 * with no size at which a range is refused.  The argument lists are those of vrdxHipCmdSortBits*, name for name and position
 * for position, and so are the semantics, word for word: ascending and stable by f(k) = (k >> beginBit) & (2^(endBit -
 * beginBit) - 1); keys move whole and values travel with their keys; storage
 * vrdxGetSorter[KeyValue]StorageRequirements(maxElementCount); the same alignment rules and bounds (nothing written outside
 * [0, n) of the caller's arrays or outside the storage requirement); the indirect count read on the device, clamped to the
 * bound and never written; the clamp at 2^30 - 4; capture and replay on other data and, indirect, on other counts up to the
 * bound; all 15 timestamp slots; word 1 of the storage reading VRDX_HIP_VERDICT_NONE afterwards; [0, 32) recording the
 * matching whole-key call, the empty range only the timestamps, an invalid range refused
 * (VRDX_HIP_STATUS_ENQUEUE_REFUSED) with nothing else touched.
 * Two differences:
 *   up to 16384 elements (maxElementCount for the indirect forms) the call records exactly what vrdxHipCmdSortBits* records:
 *   the same one-workgroup launch in the same slot, byte-identical results;
 *   beyond 16384 elements it records the CHUNKED form instead of refusing: the array is cut into up to one contiguous chunk
 *   per compute unit (at least 8192 keys each), and every digit of the range (P = ceil((endBit - beginBit) / 8), the last one
 *   of the bits that are left) takes three launches -- count per chunk, scan, stable scatter per chunk -- between the
 *   caller's arrays and the storage's scratch arrays, with one streaming copy back at the end when the number of passes that
 *   moved keys is odd.  A digit that is the same in every key moves nothing (its launches return at once); a field that is the
 *   same in every key writes neither the arrays nor the scratch arrays.  No launch waits for another workgroup.
 * Timestamps of the chunked form: slot 1 the fill, slots 2 + 3 p / 3 + 3 p / 4 + 3 p the count, scan and scatter of digit p,
 * slot 14 the copy back; the slots no step ends coincide with the one before.
 * vrdxHipDescribeRangeSortPlan reports the form, the chunks, the launches (3 P + 1) and the HBM bytes per element.
 * Range sorts ignore the planning knobs (VRDX_SMALL_SORT, VRDX_TILE_CONFIG, VRDX_HYBRID, VRDX_MSD): size alone decides; only
 * the range [0, 32), which is the whole-key sort, follows them.
 */
void vrdxHipCmdRangeSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                         VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdRangeSortKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                                 VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset, uint32_t beginBit,
                                 uint32_t endBit, VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                                 uint32_t query);
void vrdxHipCmdRangeSortIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                 VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                 VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                                 VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdRangeSortKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                         VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                         VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                         uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                         VkQueryPool queryPool, uint32_t query);
#define VRDX_HIP_RANGE_SORT_NONE 0u          /* nothing is recorded: no elements, an empty range; refused: an invalid range */
#define VRDX_HIP_RANGE_SORT_ONE_WORKGROUP 1u /* up to 16384 elements: what vrdxHipCmdSortBits* records */
#define VRDX_HIP_RANGE_SORT_WHOLE_KEY 2u     /* the range [0, 32): what vrdxCmdSort* records (vrdxHipDescribePlan says which plan) */
#define VRDX_HIP_RANGE_SORT_CHUNKED 3u       /* beyond 16384 elements: count, scan, scatter per digit */
typedef struct VrdxHipRangeSortPlanInfo {
  uint32_t form;                    /* VRDX_HIP_RANGE_SORT_* */
  uint32_t chunks;                  /* CHUNKED: workgroups of the count and scatter launches; otherwise 1 */
  uint32_t keysPerChunk;            /* CHUNKED: keys per chunk (a multiple of 256; the last chunk holds the rest); otherwise the count */
  uint32_t digits;                  /* P: digits ranked (WHOLE_KEY: 4) */
  uint32_t launches;                /* kernels recorded (CHUNKED: 3 P + 1) */
  uint32_t bytesPerElementPerPass;  /* CHUNKED: HBM bytes per element of one ACTIVE pass (12 keys-only, 20 key+value: the count
                                       reads the keys, the scatter reads and writes everything); otherwise of the whole sort */
  uint32_t bytesPerElementCopyBack; /* CHUNKED: of the copy back, which runs after an odd number of active passes; otherwise 0 */
} VrdxHipRangeSortPlanInfo;
/* What vrdxHipCmdRangeSort[KeyValue][Indirect] records on `sorter` for elementCount (the bound of an indirect call). */
void vrdxHipDescribeRangeSortPlan(VrdxSorter sorter, uint32_t elementCount, int keyValue, uint32_t beginBit, uint32_t endBit,
                                  VrdxHipRangeSortPlanInfo* info);

/**
 * Segmented sort by a bit range of the key (not part of the reference API; CUB's DeviceSegmentedRadixSort with begin_bit /
 * end_bit): vrdxHipCmdSortSegmented[KeyValue] with beginBit and endBit in front of storageBuffer, the position they have in
 * vrdxHipCmdSortBits*.
 *
 * Order: with f(k) = (k >> beginBit) & (2^(endBit - beginBit) - 1), every segment [o[i], o[i+1]) ends up in ascending order
 * of f(key); elements of equal f keep their input order; keys are moved WHOLE and values travel with their keys, as
 * vrdxHipCmdSortBits defines it.  A whole-key segmented sort of masked keys gives a different result.
 * Everything else is vrdxHipCmdSortSegmented[KeyValue]'s, word for word: the storage
 * (vrdxGetSorter[KeyValue]StorageRequirements(maxElementCount)), the alignment rules, offsets read on the device only, bad
 * offsets (VRDX_HIP_STATUS_SEGMENTS_INVALID, the segment left alone, nothing written outside [0, maxElementCount) or outside
 * the storage requirement), the clamp at 2^30 - 4, word 1 reading VRDX_HIP_VERDICT_NONE afterwards, the timestamp slots
 * (fill, small, mid, large, the rest coincide), and capture and replay on another segmentation with the same segmentCount.
 * Ranges, as for vrdxHipCmdSortBits: 0 <= beginBit <= endBit <= 32.
 *   [0, 32) records exactly what vrdxHipCmdSortSegmented[KeyValue] records: the same kernels, bit for bit the same work.
 *   beginBit == endBit records the timestamps and nothing else.
 *   beginBit > endBit or endBit > 32 records the timestamps, touches nothing and raises VRDX_HIP_STATUS_ENQUEUE_REFUSED in
 *   the sorter's word.
 * Sizes: there is none at which a range is refused.  Segments of up to 4096 and up to 16384 elements are sorted in LDS by the
 * P = ceil((endBit - beginBit) / 8) digits of the range; a larger segment is sorted by one workgroup through memory, one walk
 * of the segment per digit of the range that differs between its keys (at most P, where the whole-key form takes up to four).
 * So a single array of more than 16384 elements CAN be range-sorted as one segment, but then by one workgroup: correct, and
 * slow: vrdxHipCmdRangeSort above sorts such an array with every compute unit.  vrdxHipCmdSortBits beyond 16384 elements
 * stays refused.
 */
void vrdxHipCmdSortSegmentedBits(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                 uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                 VkBuffer keysBuffer, VkDeviceSize keysOffset, uint32_t beginBit, uint32_t endBit,
                                 VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdSortSegmentedBitsKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                         uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                         VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                         VkDeviceSize valuesOffset, uint32_t beginBit, uint32_t endBit, VkBuffer storageBuffer,
                                         VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);

/* The balanced segmented sort -- vrdxHipCmdSortSegmented[KeyValue] with huge segments spread over every compute unit -- is
 * declared in vk_radix_sort_balanced.h, next to this file. */

/**
 * Key orders of the 32-bit sorts (not part of the reference API): int32 and float32 keys, ascending or descending.  The four
 * flat calls and the two segmented calls with one order word, `order`, in front of storageBuffer -- the position it has in
 * vrdxHipCmdSort64Ordered* -- and everything else in the order of the matching call (the twin):
 *   vrdxHipCmdOrderedSort[KeyValue][Indirect]      vrdxCmdSort[KeyValue][Indirect]
 *   vrdxHipCmdOrderedSortSegmented[KeyValue]       vrdxHipCmdSortSegmented[KeyValue]
 *
 * The order word: one key type, VRDX_HIP_KEY32_UINT32, VRDX_HIP_KEY32_INT32 or VRDX_HIP_KEY32_FLOAT32, with
 * VRDX_HIP_ORDER_DESCENDING or-ed in or not.
 * Order: let T(k) = k ^ flip ^ (FLOAT32 and bit 31 of k set ? 0x7FFFFFFF : 0) on the key's 32 bits, with flip = 0 for UINT32,
 * 1 << 31 for INT32 and FLOAT32, and the complement of that for descending.  After the call the elements (of every segment)
 * are in ascending unsigned order of T(key).  T is a bijection, so:
 *   UINT32, INT32   ascending (descending) as unsigned, as two's-complement signed integers;
 *   FLOAT32         IEEE-754 totalOrder on the bits: NaNs with the sign bit set first, then -inf ... -0.0, then +0.0 ... +inf,
 *                   NaNs with the sign bit clear last, NaNs among themselves by their payload bits; descending is the reverse;
 *   stability       elements of EQUAL key keep their input order, for descending too (not the reverse of the ascending
 *                   result): what CUB's SortKeysDescending / SortPairsDescending and a stable torch.sort(descending=True) give;
 *   keys come back bit for bit as they went in, values travel with their keys.
 * FLOAT32 differs from torch.sort (and numpy.sort) in two ways: torch.sort puts ALL NaNs last (first when descending),
 * whatever their sign bit, and treats -0.0 and +0.0 as equal, leaving them in input order; here -0.0 sorts in front of +0.0.
 * On keys without NaNs and without zeros of both signs the two agree.
 * Everything else is the twin's, word for word: the storage (vrdxGetSorter[KeyValue]StorageRequirements), the alignment
 * rules (keys, values, count and offsets on 4 bytes, the storage on 16), the clamp at 2^30 - 4, the device-side count of the
 * indirect forms and its clamp to the bound -- elements from the count on are neither read nor written --, bad offsets
 * (VRDX_HIP_STATUS_SEGMENTS_INVALID), the status and verdict words, capture and replay with a NULL pool.
 *   order == VRDX_HIP_KEY32_UINT32 records exactly what the twin records: the same kernels, the same steps.
 *   An order word with any other bit set, or a key type above VRDX_HIP_KEY32_FLOAT32, is refused like an invalid bit range:
 *   the timestamps are recorded, nothing else is touched, and the sorter's word raises VRDX_HIP_STATUS_ENQUEUE_REFUSED.
 * How: up to 16384 elements, and in every segment of the segmented calls, the order costs a few instructions -- the kernels
 * apply T behind their loads and its inverse in front of their stores (a large segment: in its first and its last pass
 * through memory); measured at 0-3 % of the twin in LDS and up to 6 % on large segments.  A flat sort of MORE than 16384 elements runs one streaming launch that rewrites keys[0, n) with
 * T(key) in place, then the twin's plan unchanged (MSD, hybrid or four passes, verdict and fallback on the device as ever),
 * then one launch that rewrites keys[0, n) with the keys: two launches and 16 bytes per key on top of the twin, which
 * vrdxHipDescribeOrderedSortPlan reports.  While such a call runs the caller's key array holds T(key).
 * Timestamps: up to 16384 elements the ONE_WORKGROUP contract, the segmented calls their twin's.  Beyond 16384 elements the
 * forward transform lies in [0,1] in front of the fill, the inverse in [13,14] (which no step of the twin ends), and everything
 * between is the twin's contract.
 * Out of scope: T fused into the plan's first reader and last writer (the histogram, scatter, bucket and pass kernels):
 * which launch reads the caller's keys first and writes them last is settled on the device, and those kernels are tuned to
 * the register.  An order combined with a bit range.
 */
#define VRDX_HIP_KEY32_UINT32 0u
#define VRDX_HIP_KEY32_INT32 1u
#define VRDX_HIP_KEY32_FLOAT32 2u
void vrdxHipCmdOrderedSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                           VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                           VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdOrderedSortKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                                   VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset, uint32_t order,
                                   VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdOrderedSortIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                   VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                   VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                   VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdOrderedSortKeyValueIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                           VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                           VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                           uint32_t order, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                           VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdOrderedSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                    uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                    VkBuffer keysBuffer, VkDeviceSize keysOffset, uint32_t order, VkBuffer storageBuffer,
                                    VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdOrderedSortSegmentedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                            uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                            VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                            VkDeviceSize valuesOffset, uint32_t order, VkBuffer storageBuffer,
                                            VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);

/* ------------------------------------------------------------------------------------------
 * 32-bit keys with 64-bit values (HIP backend only)
 *
 * vrdxHipCmdWideValueSort is vrdxCmdSortKeyValue with values of 8 bytes: a pointer or handle, a pair of uint32 ids, a
 * float64, an int64 index.  Elements [0, n) of the uint32 keys come back ascending and stable; element i of the values is
 * 8 OPAQUE bytes at valuesBuffer + valuesOffset + 8 i, valuesOffset a multiple of 8, and every value travels with its key.
 * Keys and the count word need 4-byte alignment, the storage 16.
 * Storage: vrdxHipGetSorterWideValueStorageRequirements(maxElementCount) bytes -- the key+value storage of
 * vrdxGetSorterKeyValueStorageRequirements for that count (its header is this call's header) plus 12 bytes per element
 * plus a fixed pad; the size does not depend on the address.
 * As for vrdxCmdSortKeyValue[Indirect]: elementCount == 0 records nothing but the timestamps; a count beyond 2^30 - 4 is
 * clamped and raises VRDX_HIP_STATUS_COUNT_CLAMPED; all 15 timestamp slots are recorded; with a NULL pool the call is legal
 * inside a stream capture; vrdxHipReadStatus and vrdxHipReadPlanVerdict read the storage's header.
 * Indirect (the contract of vrdxHipCmdSort64[KeyValue]Indirect, word for word): the count is one uint32 at indirectBuffer +
 * indirectOffset that every step reads on the device when it runs; it is clamped to maxElementCount; elements from n on are
 * neither read nor written; plans and grids come from maxElementCount alone, so one captured call replays on any count; the
 * count word must not lie inside the storage range, and nothing writes it.
 * How (vrdxHipDescribeWideValueSortPlan reports which, with the launches and the HBM bytes per element):
 *   ONE_WORKGROUP  up to 8192 elements: one launch, keys and values sorted together in LDS (the header's verdict word
 *                  reads VRDX_HIP_VERDICT_NONE); timestamps: the ONE_WORKGROUP contract, the launch ends slot 14.
 *   GATHER         an index array in the storage is sorted along the caller's keys (one vrdxCmdSortKeyValue, recorded
 *                  inside), the values are gathered through it into the storage and copied back: four steps ending slots
 *                  1 (index), 2 (sort), 3 (gather), 4 (copy back).
 *   TWO_SORTS      from twoSortsFrom elements: the values' two words are sorted along the keys in two stable sorts of the
 *                  same key sequence, which apply the same permutation: slots 1 (split), 2 (sort of the key copy with the
 *                  low words), 3 (sort of the caller's keys with the high words), 4 (merge).  No random access.
 * The slots no step ends coincide with the one before.  Beyond ONE_WORKGROUP the status and verdict words are those of the
 * last inner sort.
 * Out of scope: two-payload forms of the MSD, hybrid and pass kernels (they would slot in behind the same plan function);
 * ordered and bit-range variants, of the segmented form below too; 64-bit keys with 64-bit values.
 * ------------------------------------------------------------------------------------------ */
void vrdxHipGetSorterWideValueStorageRequirements(VrdxSorter sorter, uint32_t maxElementCount,
                                                  VrdxSorterStorageRequirements* requirements);
void vrdxHipCmdWideValueSort(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t elementCount, VkBuffer keysBuffer,
                             VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                             VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdWideValueSortIndirect(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                     VkBuffer indirectBuffer, VkDeviceSize indirectOffset, VkBuffer keysBuffer,
                                     VkDeviceSize keysOffset, VkBuffer valuesBuffer, VkDeviceSize valuesOffset,
                                     VkBuffer storageBuffer, VkDeviceSize storageOffset, VkQueryPool queryPool,
                                     uint32_t query);
#define VRDX_HIP_WIDE_VALUE_NONE 0u          /* elementCount == 0: nothing is recorded */
#define VRDX_HIP_WIDE_VALUE_ONE_WORKGROUP 1u
#define VRDX_HIP_WIDE_VALUE_GATHER 2u
#define VRDX_HIP_WIDE_VALUE_TWO_SORTS 3u
typedef struct VrdxHipWideValuePlanInfo {
  uint32_t form;             /* VRDX_HIP_WIDE_VALUE_* */
  uint32_t launches;         /* kernels recorded, those of the inner sorts included */
  uint32_t bytesPerElement;  /* HBM bytes per element the recorded form moves (inner sorts: where their plan runs) */
  uint32_t innerPlan;        /* VRDX_HIP_PLAN_* of the inner sorts (GATHER, TWO_SORTS) */
  uint32_t oneWorkgroupMax;  /* the largest count of the ONE_WORKGROUP form */
  uint32_t twoSortsFrom;     /* the smallest count of the TWO_SORTS form */
} VrdxHipWideValuePlanInfo;
/* The form vrdxHipCmdWideValueSort[Indirect] records on `sorter` for elementCount (the bound of an indirect call). */
void vrdxHipDescribeWideValueSortPlan(VrdxSorter sorter, uint32_t elementCount, VrdxHipWideValuePlanInfo* info);

/* ------------------------------------------------------------------------------------------
 * Segmented sort of 32-bit keys with 64-bit values (HIP backend only)
 *
 * vrdxHipCmdWideValueSortSegmented is vrdxHipCmdSortSegmentedKeyValue with values of 8 opaque bytes (per-row argsort with
 * int64 indices, per-tile lists of pointers, per-expert token lists): the same arguments, name for name.
 * Order: every segment [o[i], o[i+1]) of the uint32 keys comes back ascending and stable, and every value -- 8 OPAQUE bytes at
 * valuesBuffer + valuesOffset + 8 i -- travels with its key.
 * Offsets: segmentCount + 1 uint32 CSR offsets, read on the device only.  Elements in front of o[0] and from
 * o[segmentCount] on are not written at all, and neither are segments of fewer than 2 elements.
 * Alignment: keys and offsets 4 bytes; valuesBuffer + valuesOffset a multiple of 8; the storage a multiple of 16.
 * Storage: vrdxHipGetSorterWideValueStorageRequirements(maxElementCount) bytes, the calculator of vrdxHipCmdWideValueSort.
 * Bad offsets, as in the other segmented sorts: a segment with o[i] > o[i+1] or o[i+1] > maxElementCount is left alone, and
 * any offsets that are not monotone raise VRDX_HIP_STATUS_SEGMENTS_INVALID in the storage's failure word and in the
 * sorter's word; nothing is ever written outside [0, maxElementCount) of the caller's arrays or outside the storage
 * requirement.
 * segmentCount == 0 or maxElementCount == 0 records only the timestamps; maxElementCount beyond 2^30 - 4 is clamped and
 * raises VRDX_HIP_STATUS_COUNT_CLAMPED; word 1 of the header reads VRDX_HIP_VERDICT_NONE afterwards.
 * Timestamps: all 15 slots are recorded; slots 1 to 4 end the fill, the small, the mid and the large launch, as in
 * vrdxHipCmdSortSegmented64KeyValue; a launch that cannot have work under this bound is absent and its slot coincides with
 * the one before; the later slots coincide with slot 4.
 * With a NULL pool the call is legal inside a stream capture; grids depend on segmentCount, maxElementCount and the CU count
 * only, so the graph replays on other keys and on another segmentation with the same segmentCount.
 * How: three size classes decided on the device.  Segments of up to 4096 and of up to 8192 elements are sorted in LDS, key and
 * both value words together, between one load and one store (24 bytes of HBM traffic per element); a larger segment is
 * sorted by one workgroup through memory, one walk per byte of the key that differs between its keys.
 * ------------------------------------------------------------------------------------------ */
void vrdxHipCmdWideValueSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                      uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                      VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                      VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                      VkQueryPool queryPool, uint32_t query);

/* ------------------------------------------------------------------------------------------
 * HIP-side companions of the Vulkan objects the reference's callers create themselves
 * (vkCreateQueryPool / vkGetQueryPoolResults, bench/vulkan_benchmark.cc:195-198,318-321).
 * They are not part of the reference API; they exist so a caller without a Vulkan device can
 * still use the 15-slot timestamp contract.
 * ------------------------------------------------------------------------------------------ */

/* Creates a pool of `queryCount` timestamp slots (hipEvent_t each) on the current device. */
VkResult vrdxHipCreateQueryPool(uint32_t queryCount, VkQueryPool* pQueryPool);
void vrdxHipDestroyQueryPool(VkQueryPool queryPool);
/* After the stream has completed: pData[i] = nanoseconds between slot firstQuery and slot
 * firstQuery+i (so pData[0] == 0; timestampPeriod == 1.0).  Returns VK_NOT_READY if a slot was
 * never recorded or has not completed. */
VkResult vrdxHipGetQueryPoolResults(VkQueryPool queryPool, uint32_t firstQuery, uint32_t queryCount,
                                    uint64_t* pData);

/* Device-side failure word of the LAST sort recorded with this storage (recording a sort clears the
 * word): 0 = ok.  A non-zero value means a bounded look-back spin expired (the GPU never hangs; the
 * output is then unspecified).  Synchronises the given stream.  Diagnostic only.
 * "The last sort" is the last one that had elements: a call with elementCount == 0 (segmented: segmentCount == 0 or
 * maxElementCount == 0) records nothing but its timestamps and leaves the storage, this word included, as it was. */
uint32_t vrdxHipReadStatus(VkCommandBuffer commandBuffer, VkBuffer storageBuffer,
                           VkDeviceSize storageOffset);

/* The same diagnosis for EVERY sort recorded with this sorter since the previous call (or since
 * vrdxCreateSorter), whatever storage they used: the OR of their failure bits, kept in a device
 * word the sorter owns; reading it clears it.  This is what a caller that runs many sorts through
 * one storage buffer checks once at the end.  Bit 31 is the host side of it: set when the runtime
 * refused one of the sort's enqueues (fill, copy, kernel launch) -- the vrdxCmdSort* entry points return
 * void, so this is where such an error surfaces.  Synchronises the given stream (which must belong to
 * the sorter's device and be ordered after the sorts in question). */
uint32_t vrdxHipReadSorterStatus(VrdxSorter sorter, VkCommandBuffer commandBuffer);
/* Bits of that word (and of the one line vrdxDestroySorter prints on stderr when a sorter is destroyed with any of
 * them never read -- the vrdxCmdSort* entry points return void like the reference's, so nothing fails silently): */
#define VRDX_HIP_STATUS_LOOKBACK_GAVE_UP 0x00000001u /* a bounded look-back spin expired: that sort's result is unspecified */
#define VRDX_HIP_STATUS_RANK_ORDER       0x00000002u /* the periodic repeat of the LDS lane-order check failed: vrdxHipRecheck */
#define VRDX_HIP_STATUS_SEGMENTS_INVALID 0x00000004u /* a segmented sort met offsets that decrease or end behind maxElementCount: those segments were left alone */
#define VRDX_HIP_STATUS_COUNT_CLAMPED    0x40000000u /* elementCount > 2^30 - 4 (where the reference's uint32 size math wraps, src/vk_radix_sort.h.in:105-115): the first 2^30 - 4 elements were sorted, the rest left alone */
#define VRDX_HIP_STATUS_ENQUEUE_REFUSED  0x80000000u /* the HIP runtime refused a fill, copy or launch of a sort */

/* Repeats, synchronously (~1 ms), the device check vrdxCreateSorter ran for the one-atomic ranking (LDS returning atomics
 * served in lane order: measured on every MI355X so far, not promised by the ISA manual) and switches the sorter to the
 * ballot ranking for the sorts recorded from then on if it fails (one line on stderr).  A small stream-ordered repeat
 * is recorded by the library itself behind every 65536th sort (VRDX_HIP_STATUS_RANK_ORDER); call this after a driver or
 * firmware update under a long-lived process, or whenever that bit shows up.  Not thread-safe against sorts being
 * recorded with the same sorter at the same time only in the sense that those may still use the old ranking. */
VkResult vrdxHipRecheck(VrdxSorter sorter);

/* What a pair of hipEventRecords adds to the kernel between them on this stream, in nanoseconds: the median over eight
 * runs of (event interval - the time a spinning kernel demonstrably ran by the device's own wall clock).  Slot
 * differences of the 15-slot timestamp contract include this much on top of the kernel's duration; bench.py subtracts
 * it to report kernel time (synchronises the stream; ~0.5 ms).  ~0 on failure is not assumed: returns UINT64_MAX then. */
uint64_t vrdxHipEventOverheadNs(VkCommandBuffer commandBuffer);

/* Which plan vrdxCmdSort* records for a sort of `elementCount` elements with this sorter (it depends on the count, the
 * device's CU count and the ranking mode only), and the HBM bytes per element that plan moves when the device lets it
 * run -- what a roofline figure for the whole sort has to be priced with.  Plans other than FOUR_PASSES and
 * ONE_WORKGROUP are taken or turned down ON THE DEVICE (a bucket that does not fit a workgroup's LDS: skewed keys), in
 * which case the four passes recorded behind them run and `fallbackBytesPerElement` applies. */
#define VRDX_HIP_PLAN_NONE 0u          /* elementCount == 0: nothing is recorded */
#define VRDX_HIP_PLAN_ONE_WORKGROUP 1u /* <= 16384 elements: one launch, one load and one store of the data */
#define VRDX_HIP_PLAN_FOUR_PASSES 2u   /* fused histogram + four onesweep passes: 36 B/key, 68 B/pair */
#define VRDX_HIP_PLAN_HYBRID8 3u       /* histogram + one scatter by the highest varying byte + one in-LDS sort per bucket */
#define VRDX_HIP_PLAN_HYBRID9 4u       /* round 4's nine-bit hybrid plan: no longer built (the MSD plan took its sizes); never reported, the value stays reserved */
#define VRDX_HIP_PLAN_MSD 5u           /* histogram + scatter by a 10 / 11-bit window (chosen on the device below the keys' common prefix) + up to two in-LDS passes per bucket */
typedef struct VrdxHipPlanInfo {
  uint32_t plan;                    /* VRDX_HIP_PLAN_* */
  uint32_t bits;                    /* digits of the plan's scatter through memory (8, 9, 10, 11; 0 otherwise) */
  uint32_t bytesPerElement;         /* algorithmic HBM bytes per element when the plan runs */
  uint32_t fallbackBytesPerElement; /* ... when the device turns it down (== bytesPerElement for plans decided on the host) */
  uint32_t launches;                /* kernel launches recorded (fills and copies not counted) */
} VrdxHipPlanInfo;
void vrdxHipDescribePlan(VrdxSorter sorter, uint32_t elementCount, int keyValue, VrdxHipPlanInfo* info);
/* The same for vrdxHipCmdSortBits[KeyValue][Indirect] with the range [beginBit, endBit): ONE_WORKGROUP up to 16384 elements;
 * the range of all 32 bits reports what vrdxHipDescribePlan reports; an empty or invalid range, and a range sort of more
 * elements (which is refused), report VRDX_HIP_PLAN_NONE. */
void vrdxHipDescribeSortBitsPlan(VrdxSorter sorter, uint32_t elementCount, int keyValue, uint32_t beginBit, uint32_t endBit,
                                 VrdxHipPlanInfo* info);
/* The same for vrdxHipCmdOrderedSort[KeyValue][Indirect] with the order word `order`: what vrdxHipDescribePlan reports, plus,
 * beyond one workgroup and for a word other than VRDX_HIP_KEY32_UINT32, the two transform launches and their 16 bytes per
 * element (in bytesPerElement and fallbackBytesPerElement); an invalid word (which is refused) reports VRDX_HIP_PLAN_NONE. */
void vrdxHipDescribeOrderedSortPlan(VrdxSorter sorter, uint32_t elementCount, int keyValue, uint32_t order,
                                    VrdxHipPlanInfo* info);

/* What the DEVICE made of the plan of the last sort that used this storage (word 1 of the storage; synchronises the
 * stream): vrdxHipDescribePlan is the host's intention, this is the verdict.  Meaningful for the two plans that are
 * decided on the device; a sort that ran the four passes leaves one of the "turned down" values.  Every sort that has
 * elements writes the word -- the one-workgroup sort zeroes it too -- so the verdict of an earlier sort on the same storage
 * never survives one; a call with elementCount == 0 writes nothing, and the verdict stays that of the last sort that had
 * elements (as with vrdxHipReadStatus). */
#define VRDX_HIP_VERDICT_NONE 0u            /* no plan was taken: the four passes ran (also: FOUR_PASSES / ONE_WORKGROUP sorts) */
#define VRDX_HIP_VERDICT_HYBRID8_RUNS 1u    /* HYBRID8: launch 0 scattered by the highest varying byte, the buckets were sorted in LDS */
#define VRDX_HIP_VERDICT_HYBRID8_DECLINED 2u /* HYBRID8: a bucket did not fit, the four passes ran */
#define VRDX_HIP_VERDICT_MSD_RUNS 3u        /* MSD: scatter + bucket launches sorted the input (bytesPerElement applies) */
#define VRDX_HIP_VERDICT_MSD_SORTED 4u      /* MSD: all keys identical -- nothing was moved */
uint32_t vrdxHipReadPlanVerdict(VkCommandBuffer commandBuffer, VkBuffer storageBuffer, VkDeviceSize storageOffset);

/* How many sorts this sorter recorded with the MSD plan in front (*pRecorded, counted on the host when the sort is
 * recorded) and how many of those the device turned down (*pDeclined, counted on the device when the sort runs: a bucket
 * beyond the capacity, a key outside the sampled prefix, a sample that rules the plan out) -- such sorts run the four
 * passes and cost 1.3-1.5x the plan.  Uniform keys at the very top of a plan's size range are turned down with small
 * probability by design (3-4 % of headroom); a caller that sees the ratio rise knows its keys are skewed.  (A sort captured
 * into a hipGraph is recorded once and may run many times: every replay that is turned down counts.)  Synchronises the
 * stream; either pointer may be NULL. */
VkResult vrdxHipReadPlanCounters(VrdxSorter sorter, VkCommandBuffer commandBuffer, uint32_t* pRecorded, uint32_t* pDeclined);

/* Library build info: "vrdx-hip <version> gfx950 tiles at 2^25: keys=<threads>x<keys per thread>[x<sub-tiles>]
 * key-value=... (size-adaptive | forced)". */
const char* vrdxHipVersionString(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* VK_RADIX_SORT_H */

/* The reference is a single-header library activated with VRDX_IMPLEMENTATION
 * (src/vk_radix_sort.h.in:85-86, bench/vrdx_impl.cc:1-4).  The HIP backend lives in
 * libvrdx_hip.so, so the macro is accepted and ignored to keep such translation units compiling. */
#ifdef VRDX_IMPLEMENTATION
#undef VRDX_IMPLEMENTATION
#endif
