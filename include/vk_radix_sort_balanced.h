/* The balanced segmented sort of the HIP backend: an extension header next to vk_radix_sort.h, which it includes.  The
 * entry points live in the same library (libvrdx_hip.so) and in the single-header distribution. */
#ifndef VK_RADIX_SORT_BALANCED_H
#define VK_RADIX_SORT_BALANCED_H

#include "vk_radix_sort.h"

#ifdef __cplusplus
extern "C" {
#endif

/**
 * Balanced segmented sort (not part of the reference API): vrdxHipCmdSortSegmented[KeyValue], argument for argument and word
 * for word -- uint32 keys, ascending, stable, values of 4 bytes, offsets read on the device only, the storage
 * (vrdxGetSorter[KeyValue]StorageRequirements(maxElementCount)), the alignment rules, bad offsets
 * (VRDX_HIP_STATUS_SEGMENTS_INVALID, nothing written outside [0, maxElementCount) or outside the storage requirement), the clamp
 * at 2^30 - 4, word 1 reading VRDX_HIP_VERDICT_NONE afterwards, all 15 timestamp slots, capture with a NULL pool and replay on
 * any segmentation with the same segmentCount -- with ONE difference: a segment that is long AND longer than its share of the
 * chip is cut into pieces that many workgroups sort together (a SPREAD segment).  The result is bit for bit the twin's.
 * vrdxHipCmdSortSegmented gives every segment of more than 16384 elements to one workgroup, which is right when many such
 * segments fill the chip and slow when a few are huge: four segments of 2^22 keys keep four compute units busy.
 *
 * Which segments are spread is decided on the device, per call, from the segments of more than 16384 elements (the LISTED
 * ones): with totalLarge the sum of their lengths and share = ceil(totalLarge / compute units), a listed segment of len
 * elements is spread if and only if  len > max(VRDX_HIP_BALANCED_SPREAD_FROM, VRDX_HIP_BALANCED_SPREAD_SHARES x share).
 * 256 segments of 65537 keys stay with one workgroup each, which fills 256 compute units; 64 x 262144 and 4 x 2^22 are spread.
 * A spread segment is cut into pieces of L = max(16384, ceil(totalSpread / compute units) rounded up to a multiple of 256)
 * elements and sorted by count, scan and stable scatter over the pieces for each byte of the key that differs inside THAT
 * segment, then copied home after an odd number of such passes; a spread segment whose keys are all equal is neither read
 * again nor written.  No launch waits for another workgroup.
 *
 * What is recorded: with maxElementCount <= 65536 (no segment can be spread) exactly what the twin records, the same
 * launches and slots.  Beyond it 18 launches: fill, small, mid, split, the twin's large kernel on the segments that are not
 * spread, three launches per byte, the copy back.  Timestamps: slots 1-4 as in the twin (the split lies in [3,4]); byte p ends
 * slot 5 + 2 p with its count and scan and slot 6 + 2 p with its scatter; the copy back ends slot 13; slot 14 coincides.
 * The price: where nothing is spread, the split launch and 13 launches that return at once on top of the twin -- measured
 * on one MI355X at 21-36 us keys-only and 26-66 us key+value.  A caller whose large segments always
 * fill the chip keeps the twin.
 * vrdxHipDescribeBalancedSegmentedPlan reports what would be recorded; vrdxHipReadBalancedSplit what the device decided.
 */
void vrdxHipCmdBalancedSortSegmented(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                     uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                     VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer storageBuffer,
                                     VkDeviceSize storageOffset, VkQueryPool queryPool, uint32_t query);
void vrdxHipCmdBalancedSortSegmentedKeyValue(VkCommandBuffer commandBuffer, VrdxSorter sorter, uint32_t maxElementCount,
                                             uint32_t segmentCount, VkBuffer offsetsBuffer, VkDeviceSize offsetsOffset,
                                             VkBuffer keysBuffer, VkDeviceSize keysOffset, VkBuffer valuesBuffer,
                                             VkDeviceSize valuesOffset, VkBuffer storageBuffer, VkDeviceSize storageOffset,
                                             VkQueryPool queryPool, uint32_t query);

#define VRDX_HIP_BALANCED_NONE 0u     /* nothing is recorded: no elements, no segments */
#define VRDX_HIP_BALANCED_TWIN 1u     /* up to 65536 elements: what vrdxHipCmdSortSegmented[KeyValue] records */
#define VRDX_HIP_BALANCED_BALANCED 2u /* beyond: the split, the large kernel on the rest, the passes over the pieces */
#define VRDX_HIP_BALANCED_SPREAD_FROM 65536u /* a spread segment is longer than this (four tiles of the large kernel) ... */
#define VRDX_HIP_BALANCED_SPREAD_SHARES 3u   /* ... and longer than this many shares of the chip */
typedef struct VrdxHipBalancedSegmentedPlanInfo {
  uint32_t form;          /* VRDX_HIP_BALANCED_* */
  uint32_t launches;      /* kernels recorded (the fill is one): 18 for the balanced form */
  uint32_t spreadFrom;    /* VRDX_HIP_BALANCED_SPREAD_FROM */
  uint32_t spreadShares;  /* VRDX_HIP_BALANCED_SPREAD_SHARES */
  uint32_t spreadCap;     /* most segments that can be spread under this bound on this device (0: not the balanced form) */
  uint32_t pieceCap;      /* most pieces = workgroups of a count, scatter or copy-back launch */
  uint32_t minPieceKeys;  /* the smallest piece length L (the last piece of a segment holds what is left) */
} VrdxHipBalancedSegmentedPlanInfo;
/* What vrdxHipCmdBalancedSortSegmented[KeyValue] records on `sorter` for maxElementCount and segmentCount. */
void vrdxHipDescribeBalancedSegmentedPlan(VrdxSorter sorter, uint32_t maxElementCount, uint32_t segmentCount, int keyValue,
                                          VrdxHipBalancedSegmentedPlanInfo* info);
typedef struct VrdxHipBalancedSplitInfo {
  uint32_t listedSegments;  /* segments of more than 16384 elements */
  uint32_t spreadSegments;  /* of those, the ones cut into pieces */
  uint32_t pieces;          /* their pieces */
  uint32_t pieceKeys;       /* L */
} VrdxHipBalancedSplitInfo;
/* Diagnostic, like vrdxHipReadPlanVerdict: synchronises the stream and returns the four words the split launch of the last
 * balanced call on this storage wrote (storageBuffer + storageOffset, recorded with this maxElementCount).  All zero where the
 * call records the twin.  VK_ERROR_DEVICE_LOST when the words could not be read. */
VkResult vrdxHipReadBalancedSplit(VkCommandBuffer commandBuffer, VrdxSorter sorter, VkBuffer storageBuffer,
                                  VkDeviceSize storageOffset, uint32_t maxElementCount, VrdxHipBalancedSplitInfo* info);

#ifdef __cplusplus
}
#endif

#endif /* VK_RADIX_SORT_BALANCED_H */
