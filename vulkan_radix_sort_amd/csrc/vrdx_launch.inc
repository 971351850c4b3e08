// The launch layer of vrdx_kernels.h, written once for both backends:
//   * VRDX_KERNELS lists every kernel instantiation a launcher can start, each once: its id, its host stub (the library),
//     its block size, its dynamic LDS in bytes (0: none) and its mangled name (the single header;
//     tools/generate_single_header.py reads the names from here and checks them against the code object);
//   * every Launch* entry point picks an id, computes the grid, checks its arguments and starts the kernel.
// A backend supplies the two primitives declared below and expands VRDX_KERNELS for what it needs to find a kernel:
//   the library        (the end of vrdx_kernels.hip)      the host stub: hipFuncSetAttribute, hipLaunchKernel;
//   the single header  (vrdx_module_launch.inc)           the name: hipModuleGetFunction, hipModuleLaunchKernel.
// Included inside namespace vrdx.
//
// Order: the library instantiates the kernel templates where it expands the stubs, so the device code emits them in list
// order; the list keeps the order they were emitted in before it existed.  A launcher picks a form by its offset from its
// family's first id, in the order the family's comment gives, and refuses arguments it has no kernel for with
// hipErrorInvalidValue.
#define VRDX_KERNELS(X) \
  /* histogram_kernel: kHistCopies | kHistCopiesLarge replicas */ \
  X(kHistogram, (&histogram_kernel<kHistCopies>), kHistThreads, HistLdsBytes(kHistCopies), \
    "_ZN4vrdx16histogram_kernelILj8EEEvPKjjS2_PjS3_PDv4_jj") \
  X(kHistogramLarge, (&histogram_kernel<kHistCopiesLarge>), kHistThreads, HistLdsBytes(kHistCopiesLarge), \
    "_ZN4vrdx16histogram_kernelILj32EEEvPKjjS2_PjS3_PDv4_jj") \
  /* onesweep_kernel of tile configs 0-2, each [key-value][atomic rank] (V: key+value, A: one-atomic ranking); config 2 \
     also with run-time slot counts (S) */ \
  X(kOnesweep8, (&onesweep_kernel<1024, 8, false, false, false>), 1024, OnesweepLdsWords(1024, 8) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi8ELb0ELb0ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep8A, (&onesweep_kernel<1024, 8, false, true, false>), 1024, OnesweepLdsWords(1024, 8) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi8ELb0ELb1ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep8V, (&onesweep_kernel<1024, 8, true, false, false>), 1024, OnesweepLdsWords(1024, 8) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi8ELb1ELb0ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep8VA, (&onesweep_kernel<1024, 8, true, true, false>), 1024, OnesweepLdsWords(1024, 8) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi8ELb1ELb1ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep16, (&onesweep_kernel<1024, 16, false, false, false>), 1024, OnesweepLdsWords(1024, 16) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi16ELb0ELb0ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep16A, (&onesweep_kernel<1024, 16, false, true, false>), 1024, OnesweepLdsWords(1024, 16) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi16ELb0ELb1ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep16V, (&onesweep_kernel<1024, 16, true, false, false>), 1024, OnesweepLdsWords(1024, 16) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi16ELb1ELb0ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep16VA, (&onesweep_kernel<1024, 16, true, true, false>), 1024, OnesweepLdsWords(1024, 16) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi16ELb1ELb1ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep32, (&onesweep_kernel<1024, 32, false, false, false>), 1024, OnesweepLdsWords(1024, 32) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi32ELb0ELb0ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep32A, (&onesweep_kernel<1024, 32, false, true, false>), 1024, OnesweepLdsWords(1024, 32) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi32ELb0ELb1ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep32V, (&onesweep_kernel<1024, 32, true, false, false>), 1024, OnesweepLdsWords(1024, 32) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi32ELb1ELb0ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep32VA, (&onesweep_kernel<1024, 32, true, true, false>), 1024, OnesweepLdsWords(1024, 32) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi32ELb1ELb1ELb0EEEvNS_12OnesweepArgsE") \
  X(kOnesweep32S, (&onesweep_kernel<1024, 32, false, false, true>), 1024, OnesweepLdsWords(1024, 32) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi32ELb0ELb0ELb1EEEvNS_12OnesweepArgsE") \
  X(kOnesweep32SA, (&onesweep_kernel<1024, 32, false, true, true>), 1024, OnesweepLdsWords(1024, 32) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi32ELb0ELb1ELb1EEEvNS_12OnesweepArgsE") \
  X(kOnesweep32SV, (&onesweep_kernel<1024, 32, true, false, true>), 1024, OnesweepLdsWords(1024, 32) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi32ELb1ELb0ELb1EEEvNS_12OnesweepArgsE") \
  X(kOnesweep32SVA, (&onesweep_kernel<1024, 32, true, true, true>), 1024, OnesweepLdsWords(1024, 32) * 4, \
    "_ZN4vrdx15onesweep_kernelILi1024ELi32ELb1ELb1ELb1EEEvNS_12OnesweepArgsE") \
  /* onesweep_pair_kernel (config 3; keys-only, one-atomic ranking): run-time slot counts | fixed */ \
  X(kPair32S, (&onesweep_pair_kernel<1024, 32, true>), 1024, PairLdsWords(1024, 32) * 4, \
    "_ZN4vrdx20onesweep_pair_kernelILi1024ELi32ELb1EEEvNS_12OnesweepArgsE") \
  X(kPair32, (&onesweep_pair_kernel<1024, 32, false>), 1024, PairLdsWords(1024, 32) * 4, \
    "_ZN4vrdx20onesweep_pair_kernelILi1024ELi32ELb0EEEvNS_12OnesweepArgsE") \
  /* small_sort_kernel [256 | 1024 threads][key-value][atomic rank] */ \
  X(kSmall256, (&small_sort_kernel<256, 16, false, false>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx17small_sort_kernelILi256ELi16ELb0ELb0EEEvPjS1_jPKjS1_") \
  X(kSmall256A, (&small_sort_kernel<256, 16, false, true>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx17small_sort_kernelILi256ELi16ELb0ELb1EEEvPjS1_jPKjS1_") \
  X(kSmall256V, (&small_sort_kernel<256, 16, true, false>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx17small_sort_kernelILi256ELi16ELb1ELb0EEEvPjS1_jPKjS1_") \
  X(kSmall256VA, (&small_sort_kernel<256, 16, true, true>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx17small_sort_kernelILi256ELi16ELb1ELb1EEEvPjS1_jPKjS1_") \
  X(kSmall1024, (&small_sort_kernel<1024, 16, false, false>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx17small_sort_kernelILi1024ELi16ELb0ELb0EEEvPjS1_jPKjS1_") \
  X(kSmall1024A, (&small_sort_kernel<1024, 16, false, true>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx17small_sort_kernelILi1024ELi16ELb0ELb1EEEvPjS1_jPKjS1_") \
  X(kSmall1024V, (&small_sort_kernel<1024, 16, true, false>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx17small_sort_kernelILi1024ELi16ELb1ELb0EEEvPjS1_jPKjS1_") \
  X(kSmall1024VA, (&small_sort_kernel<1024, 16, true, true>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx17small_sort_kernelILi1024ELi16ELb1ELb1EEEvPjS1_jPKjS1_") \
  /* the segmented sort [key-value: yes | no][atomic rank: yes | no][small | mid | large] */ \
  X(kSegmentedSmallVA, (&segmented_small_kernel<true, true>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx22segmented_small_kernelILb1ELb1EEEvNS_13SegmentedArgsE") \
  X(kSegmentedMidVA, (&segmented_mid_kernel<true, true>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx20segmented_mid_kernelILb1ELb1EEEvNS_13SegmentedArgsE") \
  X(kSegmentedLargeVA, (&segmented_large_kernel<true, true>), 1024, SegmentLargeLdsWords(true) * 4, \
    "_ZN4vrdx22segmented_large_kernelILb1ELb1EEEvNS_13SegmentedArgsE") \
  X(kSegmentedSmallV, (&segmented_small_kernel<true, false>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx22segmented_small_kernelILb1ELb0EEEvNS_13SegmentedArgsE") \
  X(kSegmentedMidV, (&segmented_mid_kernel<true, false>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx20segmented_mid_kernelILb1ELb0EEEvNS_13SegmentedArgsE") \
  X(kSegmentedLargeV, (&segmented_large_kernel<true, false>), 1024, SegmentLargeLdsWords(true) * 4, \
    "_ZN4vrdx22segmented_large_kernelILb1ELb0EEEvNS_13SegmentedArgsE") \
  X(kSegmentedSmallA, (&segmented_small_kernel<false, true>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx22segmented_small_kernelILb0ELb1EEEvNS_13SegmentedArgsE") \
  X(kSegmentedMidA, (&segmented_mid_kernel<false, true>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx20segmented_mid_kernelILb0ELb1EEEvNS_13SegmentedArgsE") \
  X(kSegmentedLargeA, (&segmented_large_kernel<false, true>), 1024, SegmentLargeLdsWords(false) * 4, \
    "_ZN4vrdx22segmented_large_kernelILb0ELb1EEEvNS_13SegmentedArgsE") \
  X(kSegmentedSmall, (&segmented_small_kernel<false, false>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx22segmented_small_kernelILb0ELb0EEEvNS_13SegmentedArgsE") \
  X(kSegmentedMid, (&segmented_mid_kernel<false, false>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx20segmented_mid_kernelILb0ELb0EEEvNS_13SegmentedArgsE") \
  X(kSegmentedLarge, (&segmented_large_kernel<false, false>), 1024, SegmentLargeLdsWords(false) * 4, \
    "_ZN4vrdx22segmented_large_kernelILb0ELb0EEEvNS_13SegmentedArgsE") \
  /* bucket_sort_kernel [4 | 8 | 16 keys per thread][key-value][atomic rank]; 32 keys per thread: one-atomic ranking only */ \
  X(kBucket4, (&bucket_sort_kernel<1024, 4, false, false>), 1024, SmallSortLdsWords(1024, 4, false) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi4ELb0ELb0EEEvNS_14BucketSortArgsE") \
  X(kBucket4A, (&bucket_sort_kernel<1024, 4, false, true>), 1024, SmallSortLdsWords(1024, 4, false) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi4ELb0ELb1EEEvNS_14BucketSortArgsE") \
  X(kBucket4V, (&bucket_sort_kernel<1024, 4, true, false>), 1024, SmallSortLdsWords(1024, 4, true) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi4ELb1ELb0EEEvNS_14BucketSortArgsE") \
  X(kBucket4VA, (&bucket_sort_kernel<1024, 4, true, true>), 1024, SmallSortLdsWords(1024, 4, true) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi4ELb1ELb1EEEvNS_14BucketSortArgsE") \
  X(kBucket8, (&bucket_sort_kernel<1024, 8, false, false>), 1024, SmallSortLdsWords(1024, 8, false) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi8ELb0ELb0EEEvNS_14BucketSortArgsE") \
  X(kBucket8A, (&bucket_sort_kernel<1024, 8, false, true>), 1024, SmallSortLdsWords(1024, 8, false) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi8ELb0ELb1EEEvNS_14BucketSortArgsE") \
  X(kBucket8V, (&bucket_sort_kernel<1024, 8, true, false>), 1024, SmallSortLdsWords(1024, 8, true) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi8ELb1ELb0EEEvNS_14BucketSortArgsE") \
  X(kBucket8VA, (&bucket_sort_kernel<1024, 8, true, true>), 1024, SmallSortLdsWords(1024, 8, true) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi8ELb1ELb1EEEvNS_14BucketSortArgsE") \
  X(kBucket16, (&bucket_sort_kernel<1024, 16, false, false>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi16ELb0ELb0EEEvNS_14BucketSortArgsE") \
  X(kBucket16A, (&bucket_sort_kernel<1024, 16, false, true>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi16ELb0ELb1EEEvNS_14BucketSortArgsE") \
  X(kBucket16V, (&bucket_sort_kernel<1024, 16, true, false>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi16ELb1ELb0EEEvNS_14BucketSortArgsE") \
  X(kBucket16VA, (&bucket_sort_kernel<1024, 16, true, true>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi16ELb1ELb1EEEvNS_14BucketSortArgsE") \
  X(kBucket32A, (&bucket_sort_kernel<1024, 32, false, true>), 1024, SmallSortLdsWords(1024, 32, false) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi32ELb0ELb1EEEvNS_14BucketSortArgsE") \
  X(kBucket32VA, (&bucket_sort_kernel<1024, 32, true, true>), 1024, SmallSortLdsWords(1024, 32, true) * 4, \
    "_ZN4vrdx18bucket_sort_kernelILi1024ELi32ELb1ELb1EEEvNS_14BucketSortArgsE") \
  /* the MSD plan's scatter and bucket launches with a pass of its fallback as a second role \
     [10 | 11 bits][key-value][scatter | buckets][fixed | run-time slot counts] */ \
  X(kMsdScatterOrPass0_10, (&msd_scatter_or_pass0_kernel<10, false, false>), 1024, MsdFusedLdsWords(false, 10, false) * 4, \
    "_ZN4vrdx27msd_scatter_or_pass0_kernelILj10ELb0ELb0EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdScatterOrPass0_10S, (&msd_scatter_or_pass0_kernel<10, false, true>), 1024, MsdFusedLdsWords(false, 10, false) * 4, \
    "_ZN4vrdx27msd_scatter_or_pass0_kernelILj10ELb0ELb1EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdBucketsOrPass1_10, (&msd_buckets_or_pass1_kernel<10, false, false>), 1024, MsdFusedLdsWords(false, 10, true) * 4, \
    "_ZN4vrdx27msd_buckets_or_pass1_kernelILj10ELb0ELb0EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdBucketsOrPass1_10S, (&msd_buckets_or_pass1_kernel<10, false, true>), 1024, MsdFusedLdsWords(false, 10, true) * 4, \
    "_ZN4vrdx27msd_buckets_or_pass1_kernelILj10ELb0ELb1EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdScatterOrPass0_10V, (&msd_scatter_or_pass0_kernel<10, true, false>), 1024, MsdFusedLdsWords(true, 10, false) * 4, \
    "_ZN4vrdx27msd_scatter_or_pass0_kernelILj10ELb1ELb0EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdScatterOrPass0_10VS, (&msd_scatter_or_pass0_kernel<10, true, true>), 1024, MsdFusedLdsWords(true, 10, false) * 4, \
    "_ZN4vrdx27msd_scatter_or_pass0_kernelILj10ELb1ELb1EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdBucketsOrPass1_10V, (&msd_buckets_or_pass1_kernel<10, true, false>), 1024, MsdFusedLdsWords(true, 10, true) * 4, \
    "_ZN4vrdx27msd_buckets_or_pass1_kernelILj10ELb1ELb0EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdBucketsOrPass1_10VS, (&msd_buckets_or_pass1_kernel<10, true, true>), 1024, MsdFusedLdsWords(true, 10, true) * 4, \
    "_ZN4vrdx27msd_buckets_or_pass1_kernelILj10ELb1ELb1EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdScatterOrPass0_11, (&msd_scatter_or_pass0_kernel<11, false, false>), 1024, MsdFusedLdsWords(false, 11, false) * 4, \
    "_ZN4vrdx27msd_scatter_or_pass0_kernelILj11ELb0ELb0EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdScatterOrPass0_11S, (&msd_scatter_or_pass0_kernel<11, false, true>), 1024, MsdFusedLdsWords(false, 11, false) * 4, \
    "_ZN4vrdx27msd_scatter_or_pass0_kernelILj11ELb0ELb1EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdBucketsOrPass1_11, (&msd_buckets_or_pass1_kernel<11, false, false>), 1024, MsdFusedLdsWords(false, 11, true) * 4, \
    "_ZN4vrdx27msd_buckets_or_pass1_kernelILj11ELb0ELb0EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdBucketsOrPass1_11S, (&msd_buckets_or_pass1_kernel<11, false, true>), 1024, MsdFusedLdsWords(false, 11, true) * 4, \
    "_ZN4vrdx27msd_buckets_or_pass1_kernelILj11ELb0ELb1EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdScatterOrPass0_11V, (&msd_scatter_or_pass0_kernel<11, true, false>), 1024, MsdFusedLdsWords(true, 11, false) * 4, \
    "_ZN4vrdx27msd_scatter_or_pass0_kernelILj11ELb1ELb0EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdScatterOrPass0_11VS, (&msd_scatter_or_pass0_kernel<11, true, true>), 1024, MsdFusedLdsWords(true, 11, false) * 4, \
    "_ZN4vrdx27msd_scatter_or_pass0_kernelILj11ELb1ELb1EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdBucketsOrPass1_11V, (&msd_buckets_or_pass1_kernel<11, true, false>), 1024, MsdFusedLdsWords(true, 11, true) * 4, \
    "_ZN4vrdx27msd_buckets_or_pass1_kernelILj11ELb1ELb0EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  X(kMsdBucketsOrPass1_11VS, (&msd_buckets_or_pass1_kernel<11, true, true>), 1024, MsdFusedLdsWords(true, 11, true) * 4, \
    "_ZN4vrdx27msd_buckets_or_pass1_kernelILj11ELb1ELb1EEEvNS_7MsdArgsENS_12OnesweepArgsE") \
  /* the MSD plan: bucket_sort2_half_kernel (ten bits, buckets of at most kMsdHalfCap) [key-value: yes | no] */ \
  X(kBucketMsdHalfV, (&bucket_sort2_half_kernel<10, true>), 512, BucketSort2LdsWords(kMsdHalfCap / 512, 512) * 4, \
    "_ZN4vrdx24bucket_sort2_half_kernelILj10ELb1EEEvNS_7MsdArgsE") \
  X(kBucketMsdHalf, (&bucket_sort2_half_kernel<10, false>), 512, BucketSort2LdsWords(kMsdHalfCap / 512, 512) * 4, \
    "_ZN4vrdx24bucket_sort2_half_kernelILj10ELb0EEEvNS_7MsdArgsE") \
  /* histogram_msd_kernel [10 | 11 bits][kHistCopiesLarge | kHistCopies replicas] */ \
  X(kHistogramMsdLarge10, (&histogram_msd_kernel<kHistCopiesLarge, 10>), kHistThreads, HistMsdLdsBytes(kHistCopiesLarge, 10), \
    "_ZN4vrdx20histogram_msd_kernelILj32ELj10EEEvNS_7MsdArgsE") \
  X(kHistogramMsd10, (&histogram_msd_kernel<kHistCopies, 10>), kHistThreads, HistMsdLdsBytes(kHistCopies, 10), \
    "_ZN4vrdx20histogram_msd_kernelILj8ELj10EEEvNS_7MsdArgsE") \
  X(kHistogramMsdLarge11, (&histogram_msd_kernel<kHistCopiesLarge, 11>), kHistThreads, HistMsdLdsBytes(kHistCopiesLarge, 11), \
    "_ZN4vrdx20histogram_msd_kernelILj32ELj11EEEvNS_7MsdArgsE") \
  X(kHistogramMsd11, (&histogram_msd_kernel<kHistCopies, 11>), kHistThreads, HistMsdLdsBytes(kHistCopies, 11), \
    "_ZN4vrdx20histogram_msd_kernelILj8ELj11EEEvNS_7MsdArgsE") \
  /* spine_msd_kernel [10 | 11 bits] */ \
  X(kSpineMsd10, (&spine_msd_kernel<10>), 1024, 0, \
    "_ZN4vrdx16spine_msd_kernelILj10EEEvNS_7MsdArgsE") \
  X(kSpineMsd11, (&spine_msd_kernel<11>), 1024, 0, \
    "_ZN4vrdx16spine_msd_kernelILj11EEEvNS_7MsdArgsE") \
  /* no template: the segmented sort's fill, the two LDS order checks, the calibration spin */ \
  X(kSegmentedClear, (&segmented_clear_kernel), 64, 0, \
    "_ZN4vrdx22segmented_clear_kernelENS_13SegmentedArgsE") \
  X(kOrderCheck, (&lds_order_check_kernel), 1024, 0, \
    "_ZN4vrdx22lds_order_check_kernelEPjS0_") \
  X(kOrderCheckPacked, (&lds_order_check_packed_kernel), 1024, kOrderCheckPackedLdsBytes, \
    "_ZN4vrdx29lds_order_check_packed_kernelEPjS0_") \
  X(kSpin, (&spin_kernel), 64, 0, \
    "_ZN4vrdx11spin_kernelEPyj") \
  /* 64-bit keys: split64_kernel [high words | iota], merge, gather of the high words, permute, copy back */ \
  X(kSplit64, (&split64_kernel<false>), kSort64Threads, 0, \
    "_ZN4vrdx14split64_kernelILb0EEEvPKmPjS3_jPKj") \
  X(kSplit64Iota, (&split64_kernel<true>), kSort64Threads, 0, \
    "_ZN4vrdx14split64_kernelILb1EEEvPKmPjS3_jPKj") \
  X(kMerge64, (&merge64_kernel), kSort64Threads, 0, \
    "_ZN4vrdx14merge64_kernelEPmPKjS2_jS2_") \
  X(kGatherHi64, (&gather_hi64_kernel), kSort64Threads, 0, \
    "_ZN4vrdx18gather_hi64_kernelEPKmPKjPjjS3_") \
  X(kPermute64, (&permute64_kernel), kSort64Threads, 0, \
    "_ZN4vrdx16permute64_kernelEPKmPKjS3_PjPmjS3_") \
  X(kCopyBack64, (&copy_back64_kernel), kSort64Threads, 0, \
    "_ZN4vrdx18copy_back64_kernelEPmPjPKmPKjjS5_") \
  /* the segmented sort of 64-bit keys [small | mid | large][key-value][atomic rank] */ \
  X(kSegmented64Small, (&segmented_small64_kernel<false, false>), 256, SortInWorkgroup64LdsWords(256, 16, false) * 4, \
    "_ZN4vrdx24segmented_small64_kernelILb0ELb0EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64SmallA, (&segmented_small64_kernel<false, true>), 256, SortInWorkgroup64LdsWords(256, 16, false) * 4, \
    "_ZN4vrdx24segmented_small64_kernelILb0ELb1EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64SmallV, (&segmented_small64_kernel<true, false>), 256, SortInWorkgroup64LdsWords(256, 16, true) * 4, \
    "_ZN4vrdx24segmented_small64_kernelILb1ELb0EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64SmallVA, (&segmented_small64_kernel<true, true>), 256, SortInWorkgroup64LdsWords(256, 16, true) * 4, \
    "_ZN4vrdx24segmented_small64_kernelILb1ELb1EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64Mid, (&segmented_mid64_kernel<false, false>), 1024, SortInWorkgroup64LdsWords(1024, Seg64MidKpt(false), false) * 4, \
    "_ZN4vrdx22segmented_mid64_kernelILb0ELb0EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64MidA, (&segmented_mid64_kernel<false, true>), 1024, SortInWorkgroup64LdsWords(1024, Seg64MidKpt(false), false) * 4, \
    "_ZN4vrdx22segmented_mid64_kernelILb0ELb1EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64MidV, (&segmented_mid64_kernel<true, false>), 1024, SortInWorkgroup64LdsWords(1024, Seg64MidKpt(true), true) * 4, \
    "_ZN4vrdx22segmented_mid64_kernelILb1ELb0EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64MidVA, (&segmented_mid64_kernel<true, true>), 1024, SortInWorkgroup64LdsWords(1024, Seg64MidKpt(true), true) * 4, \
    "_ZN4vrdx22segmented_mid64_kernelILb1ELb1EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64Large, (&segmented_large64_kernel<false, false>), 1024, Segment64LargeLdsWords(false) * 4, \
    "_ZN4vrdx24segmented_large64_kernelILb0ELb0EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64LargeA, (&segmented_large64_kernel<false, true>), 1024, Segment64LargeLdsWords(false) * 4, \
    "_ZN4vrdx24segmented_large64_kernelILb0ELb1EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64LargeV, (&segmented_large64_kernel<true, false>), 1024, Segment64LargeLdsWords(true) * 4, \
    "_ZN4vrdx24segmented_large64_kernelILb1ELb0EEEvNS_15Segmented64ArgsE") \
  X(kSegmented64LargeVA, (&segmented_large64_kernel<true, true>), 1024, Segment64LargeLdsWords(true) * 4, \
    "_ZN4vrdx24segmented_large64_kernelILb1ELb1EEEvNS_15Segmented64ArgsE") \
  /* ---- the bit-range sorts (vrdxHipCmdSortBits): the range form of small_sort_kernel, in the same order ---- */ \
  /* small_sort_bits_kernel [256 | 1024 threads][key-value][atomic rank] */ \
  X(kSmallBits256, (&small_sort_bits_kernel<256, 16, false, false>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx22small_sort_bits_kernelILi256ELi16ELb0ELb0EEEvPjS1_jPKjS1_jj") \
  X(kSmallBits256A, (&small_sort_bits_kernel<256, 16, false, true>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx22small_sort_bits_kernelILi256ELi16ELb0ELb1EEEvPjS1_jPKjS1_jj") \
  X(kSmallBits256V, (&small_sort_bits_kernel<256, 16, true, false>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx22small_sort_bits_kernelILi256ELi16ELb1ELb0EEEvPjS1_jPKjS1_jj") \
  X(kSmallBits256VA, (&small_sort_bits_kernel<256, 16, true, true>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx22small_sort_bits_kernelILi256ELi16ELb1ELb1EEEvPjS1_jPKjS1_jj") \
  X(kSmallBits1024, (&small_sort_bits_kernel<1024, 16, false, false>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx22small_sort_bits_kernelILi1024ELi16ELb0ELb0EEEvPjS1_jPKjS1_jj") \
  X(kSmallBits1024A, (&small_sort_bits_kernel<1024, 16, false, true>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx22small_sort_bits_kernelILi1024ELi16ELb0ELb1EEEvPjS1_jPKjS1_jj") \
  X(kSmallBits1024V, (&small_sort_bits_kernel<1024, 16, true, false>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx22small_sort_bits_kernelILi1024ELi16ELb1ELb0EEEvPjS1_jPKjS1_jj") \
  X(kSmallBits1024VA, (&small_sort_bits_kernel<1024, 16, true, true>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx22small_sort_bits_kernelILi1024ELi16ELb1ELb1EEEvPjS1_jPKjS1_jj") \
  /* ---- the segmented sort by a bit range (vrdxHipCmdSortSegmentedBits): the range forms of the three segmented kernels \
     [small | mid | large][key-value][atomic rank] ---- */ \
  X(kSegmentedBitsSmall, (&segmented_small_bits_kernel<false, false>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx27segmented_small_bits_kernelILb0ELb0EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsSmallA, (&segmented_small_bits_kernel<false, true>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx27segmented_small_bits_kernelILb0ELb1EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsSmallV, (&segmented_small_bits_kernel<true, false>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx27segmented_small_bits_kernelILb1ELb0EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsSmallVA, (&segmented_small_bits_kernel<true, true>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx27segmented_small_bits_kernelILb1ELb1EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsMid, (&segmented_mid_bits_kernel<false, false>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx25segmented_mid_bits_kernelILb0ELb0EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsMidA, (&segmented_mid_bits_kernel<false, true>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx25segmented_mid_bits_kernelILb0ELb1EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsMidV, (&segmented_mid_bits_kernel<true, false>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx25segmented_mid_bits_kernelILb1ELb0EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsMidVA, (&segmented_mid_bits_kernel<true, true>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx25segmented_mid_bits_kernelILb1ELb1EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsLarge, (&segmented_large_bits_kernel<false, false>), 1024, SegmentLargeLdsWords(false) * 4, \
    "_ZN4vrdx27segmented_large_bits_kernelILb0ELb0EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsLargeA, (&segmented_large_bits_kernel<false, true>), 1024, SegmentLargeLdsWords(false) * 4, \
    "_ZN4vrdx27segmented_large_bits_kernelILb0ELb1EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsLargeV, (&segmented_large_bits_kernel<true, false>), 1024, SegmentLargeLdsWords(true) * 4, \
    "_ZN4vrdx27segmented_large_bits_kernelILb1ELb0EEEvNS_13SegmentedArgsEjj") \
  X(kSegmentedBitsLargeVA, (&segmented_large_bits_kernel<true, true>), 1024, SegmentLargeLdsWords(true) * 4, \
    "_ZN4vrdx27segmented_large_bits_kernelILb1ELb1EEEvNS_13SegmentedArgsEjj") \
  /* ---- key orders of the 64-bit sorts (vrdxHipCmdSort64Ordered*): the ordered forms of the split [high words | iota], \
     the merge, the gather and the permutation ---- */ \
  X(kSplit64Ordered, (&split64_ordered_kernel<false>), kSort64Threads, 0, \
    "_ZN4vrdx22split64_ordered_kernelILb0EEEvPKmPjS3_jPKjj") \
  X(kSplit64OrderedIota, (&split64_ordered_kernel<true>), kSort64Threads, 0, \
    "_ZN4vrdx22split64_ordered_kernelILb1EEEvPKmPjS3_jPKjj") \
  X(kMerge64Ordered, (&merge64_ordered_kernel), kSort64Threads, 0, \
    "_ZN4vrdx22merge64_ordered_kernelEPmPKjS2_jS2_j") \
  X(kGatherHi64Ordered, (&gather_hi64_ordered_kernel), kSort64Threads, 0, \
    "_ZN4vrdx26gather_hi64_ordered_kernelEPKmPKjPjjS3_j") \
  X(kPermute64Ordered, (&permute64_ordered_kernel), kSort64Threads, 0, \
    "_ZN4vrdx24permute64_ordered_kernelEPKmPKjS3_PjPmjS3_j") \
  /* ---- vrdxHipCmdSortSegmented64Ordered*: the ordered forms of the three segmented 64-bit kernels \
     [small | mid | large][key-value][atomic rank] ---- */ \
  X(kSegmented64OrderedSmall, (&segmented_small64_ordered_kernel<false, false>), 256, SortInWorkgroup64LdsWords(256, 16, false) * 4, \
    "_ZN4vrdx32segmented_small64_ordered_kernelILb0ELb0EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedSmallA, (&segmented_small64_ordered_kernel<false, true>), 256, SortInWorkgroup64LdsWords(256, 16, false) * 4, \
    "_ZN4vrdx32segmented_small64_ordered_kernelILb0ELb1EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedSmallV, (&segmented_small64_ordered_kernel<true, false>), 256, SortInWorkgroup64LdsWords(256, 16, true) * 4, \
    "_ZN4vrdx32segmented_small64_ordered_kernelILb1ELb0EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedSmallVA, (&segmented_small64_ordered_kernel<true, true>), 256, SortInWorkgroup64LdsWords(256, 16, true) * 4, \
    "_ZN4vrdx32segmented_small64_ordered_kernelILb1ELb1EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedMid, (&segmented_mid64_ordered_kernel<false, false>), 1024, SortInWorkgroup64LdsWords(1024, Seg64MidKpt(false), false) * 4, \
    "_ZN4vrdx30segmented_mid64_ordered_kernelILb0ELb0EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedMidA, (&segmented_mid64_ordered_kernel<false, true>), 1024, SortInWorkgroup64LdsWords(1024, Seg64MidKpt(false), false) * 4, \
    "_ZN4vrdx30segmented_mid64_ordered_kernelILb0ELb1EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedMidV, (&segmented_mid64_ordered_kernel<true, false>), 1024, SortInWorkgroup64LdsWords(1024, Seg64MidKpt(true), true) * 4, \
    "_ZN4vrdx30segmented_mid64_ordered_kernelILb1ELb0EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedMidVA, (&segmented_mid64_ordered_kernel<true, true>), 1024, SortInWorkgroup64LdsWords(1024, Seg64MidKpt(true), true) * 4, \
    "_ZN4vrdx30segmented_mid64_ordered_kernelILb1ELb1EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedLarge, (&segmented_large64_ordered_kernel<false, false>), 1024, Segment64LargeLdsWords(false) * 4, \
    "_ZN4vrdx32segmented_large64_ordered_kernelILb0ELb0EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedLargeA, (&segmented_large64_ordered_kernel<false, true>), 1024, Segment64LargeLdsWords(false) * 4, \
    "_ZN4vrdx32segmented_large64_ordered_kernelILb0ELb1EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedLargeV, (&segmented_large64_ordered_kernel<true, false>), 1024, Segment64LargeLdsWords(true) * 4, \
    "_ZN4vrdx32segmented_large64_ordered_kernelILb1ELb0EEEvNS_15Segmented64ArgsEj") \
  X(kSegmented64OrderedLargeVA, (&segmented_large64_ordered_kernel<true, true>), 1024, Segment64LargeLdsWords(true) * 4, \
    "_ZN4vrdx32segmented_large64_ordered_kernelILb1ELb1EEEvNS_15Segmented64ArgsEj")

// The kernels of the ordered 32-bit sorts (vrdxHipCmdOrderedSort*) stand in a list of their own BEHIND VRDX_KERNELS: that list,
// its ids and kNumKernels are what tests/native/record_trace prints, and no entry point it records starts one of these.  The
// backends expand VRDX_ALL_KERNELS (kNumAllKernels ids), so the library's stubs and the single header find both lists.
#define VRDX_ORDERED32_KERNELS(X) \
  /* small_sort_ordered_kernel [256 | 1024 threads][key-value][atomic rank] */ \
  X(kSmallOrdered256, (&small_sort_ordered_kernel<256, 16, false, false>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx25small_sort_ordered_kernelILi256ELi16ELb0ELb0EEEvPjS1_jPKjS1_j") \
  X(kSmallOrdered256A, (&small_sort_ordered_kernel<256, 16, false, true>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx25small_sort_ordered_kernelILi256ELi16ELb0ELb1EEEvPjS1_jPKjS1_j") \
  X(kSmallOrdered256V, (&small_sort_ordered_kernel<256, 16, true, false>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx25small_sort_ordered_kernelILi256ELi16ELb1ELb0EEEvPjS1_jPKjS1_j") \
  X(kSmallOrdered256VA, (&small_sort_ordered_kernel<256, 16, true, true>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx25small_sort_ordered_kernelILi256ELi16ELb1ELb1EEEvPjS1_jPKjS1_j") \
  X(kSmallOrdered1024, (&small_sort_ordered_kernel<1024, 16, false, false>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx25small_sort_ordered_kernelILi1024ELi16ELb0ELb0EEEvPjS1_jPKjS1_j") \
  X(kSmallOrdered1024A, (&small_sort_ordered_kernel<1024, 16, false, true>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx25small_sort_ordered_kernelILi1024ELi16ELb0ELb1EEEvPjS1_jPKjS1_j") \
  X(kSmallOrdered1024V, (&small_sort_ordered_kernel<1024, 16, true, false>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx25small_sort_ordered_kernelILi1024ELi16ELb1ELb0EEEvPjS1_jPKjS1_j") \
  X(kSmallOrdered1024VA, (&small_sort_ordered_kernel<1024, 16, true, true>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx25small_sort_ordered_kernelILi1024ELi16ELb1ELb1EEEvPjS1_jPKjS1_j") \
  /* order32_kernel [forward | inverse] */ \
  X(kOrder32Forward, (&order32_kernel<false>), kOrder32Threads, 0, \
    "_ZN4vrdx14order32_kernelILb0EEEvPjjPKjj") \
  X(kOrder32Inverse, (&order32_kernel<true>), kOrder32Threads, 0, \
    "_ZN4vrdx14order32_kernelILb1EEEvPjjPKjj") \
  /* the ordered forms of the three segmented kernels [small | mid | large][key-value][atomic rank] */ \
  X(kSegmentedOrderedSmall, (&segmented_small_ordered_kernel<false, false>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx30segmented_small_ordered_kernelILb0ELb0EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedSmallA, (&segmented_small_ordered_kernel<false, true>), 256, SmallSortLdsWords(256, 16, false) * 4, \
    "_ZN4vrdx30segmented_small_ordered_kernelILb0ELb1EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedSmallV, (&segmented_small_ordered_kernel<true, false>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx30segmented_small_ordered_kernelILb1ELb0EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedSmallVA, (&segmented_small_ordered_kernel<true, true>), 256, SmallSortLdsWords(256, 16, true) * 4, \
    "_ZN4vrdx30segmented_small_ordered_kernelILb1ELb1EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedMid, (&segmented_mid_ordered_kernel<false, false>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx28segmented_mid_ordered_kernelILb0ELb0EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedMidA, (&segmented_mid_ordered_kernel<false, true>), 1024, SmallSortLdsWords(1024, 16, false) * 4, \
    "_ZN4vrdx28segmented_mid_ordered_kernelILb0ELb1EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedMidV, (&segmented_mid_ordered_kernel<true, false>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx28segmented_mid_ordered_kernelILb1ELb0EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedMidVA, (&segmented_mid_ordered_kernel<true, true>), 1024, SmallSortLdsWords(1024, 16, true) * 4, \
    "_ZN4vrdx28segmented_mid_ordered_kernelILb1ELb1EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedLarge, (&segmented_large_ordered_kernel<false, false>), 1024, SegmentLargeLdsWords(false) * 4, \
    "_ZN4vrdx30segmented_large_ordered_kernelILb0ELb0EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedLargeA, (&segmented_large_ordered_kernel<false, true>), 1024, SegmentLargeLdsWords(false) * 4, \
    "_ZN4vrdx30segmented_large_ordered_kernelILb0ELb1EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedLargeV, (&segmented_large_ordered_kernel<true, false>), 1024, SegmentLargeLdsWords(true) * 4, \
    "_ZN4vrdx30segmented_large_ordered_kernelILb1ELb0EEEvNS_13SegmentedArgsEj") \
  X(kSegmentedOrderedLargeVA, (&segmented_large_ordered_kernel<true, true>), 1024, SegmentLargeLdsWords(true) * 4, \
    "_ZN4vrdx30segmented_large_ordered_kernelILb1ELb1EEEvNS_13SegmentedArgsEj")

// The kernels of the range sorts beyond one workgroup (vrdxHipCmdRangeSort*): a fourth list for the same reason.  Its ids
// follow the wide-value list's (VRDX_ALL_KERNELS below); the text stands in front of that list, whose names stay the last of
// this file.
#define VRDX_RANGE_SORT_KERNELS(X) \
  /* range_count_kernel [later passes | the first launch] */ \
  X(kRangeCount, (&range_count_kernel<false>), 1024, 0, \
    "_ZN4vrdx18range_count_kernelILb0EEEvNS_13RangeSortArgsE") \
  X(kRangeCountFirst, (&range_count_kernel<true>), 1024, 0, \
    "_ZN4vrdx18range_count_kernelILb1EEEvNS_13RangeSortArgsE") \
  X(kRangeScan, (&range_scan_kernel), 1024, 0, \
    "_ZN4vrdx17range_scan_kernelENS_13RangeSortArgsE") \
  /* range_scatter_kernel [key-value][atomic rank] */ \
  X(kRangeScatter, (&range_scatter_kernel<false, false>), 1024, RangeScatterLdsWords(false) * 4, \
    "_ZN4vrdx20range_scatter_kernelILb0ELb0EEEvNS_13RangeSortArgsE") \
  X(kRangeScatterA, (&range_scatter_kernel<false, true>), 1024, RangeScatterLdsWords(false) * 4, \
    "_ZN4vrdx20range_scatter_kernelILb0ELb1EEEvNS_13RangeSortArgsE") \
  X(kRangeScatterV, (&range_scatter_kernel<true, false>), 1024, RangeScatterLdsWords(true) * 4, \
    "_ZN4vrdx20range_scatter_kernelILb1ELb0EEEvNS_13RangeSortArgsE") \
  X(kRangeScatterVA, (&range_scatter_kernel<true, true>), 1024, RangeScatterLdsWords(true) * 4, \
    "_ZN4vrdx20range_scatter_kernelILb1ELb1EEEvNS_13RangeSortArgsE") \
  /* range_copy_back_kernel [key-value] */ \
  X(kRangeCopyBack, (&range_copy_back_kernel<false>), kRangeCopyThreads, 0, \
    "_ZN4vrdx22range_copy_back_kernelILb0EEEvNS_13RangeSortArgsE") \
  X(kRangeCopyBackV, (&range_copy_back_kernel<true>), kRangeCopyThreads, 0, \
    "_ZN4vrdx22range_copy_back_kernelILb1EEEvNS_13RangeSortArgsE")

// The kernels of the balanced segmented sort (vrdxHipCmdBalancedSortSegmented*): a fifth list for the same reason.  Its ids
// follow the range-sort list's; the text stands here, in front of the wide-value list.
#define VRDX_BALANCED_SEGMENTED_KERNELS(X) \
  X(kSegmentedSplit, (&segmented_split_kernel), 1024, 0, \
    "_ZN4vrdx22segmented_split_kernelENS_21BalancedSegmentedArgsE") \
  X(kSegmentedPieceCount, (&segmented_piece_count_kernel), 1024, 0, \
    "_ZN4vrdx28segmented_piece_count_kernelENS_21BalancedSegmentedArgsE") \
  X(kSegmentedPieceScan, (&segmented_piece_scan_kernel), 1024, 0, \
    "_ZN4vrdx27segmented_piece_scan_kernelENS_21BalancedSegmentedArgsE") \
  /* segmented_piece_scatter_kernel [key-value][atomic rank] */ \
  X(kSegmentedPieceScatter, (&segmented_piece_scatter_kernel<false, false>), 1024, RangeScatterLdsWords(false) * 4, \
    "_ZN4vrdx30segmented_piece_scatter_kernelILb0ELb0EEEvNS_21BalancedSegmentedArgsE") \
  X(kSegmentedPieceScatterA, (&segmented_piece_scatter_kernel<false, true>), 1024, RangeScatterLdsWords(false) * 4, \
    "_ZN4vrdx30segmented_piece_scatter_kernelILb0ELb1EEEvNS_21BalancedSegmentedArgsE") \
  X(kSegmentedPieceScatterV, (&segmented_piece_scatter_kernel<true, false>), 1024, RangeScatterLdsWords(true) * 4, \
    "_ZN4vrdx30segmented_piece_scatter_kernelILb1ELb0EEEvNS_21BalancedSegmentedArgsE") \
  X(kSegmentedPieceScatterVA, (&segmented_piece_scatter_kernel<true, true>), 1024, RangeScatterLdsWords(true) * 4, \
    "_ZN4vrdx30segmented_piece_scatter_kernelILb1ELb1EEEvNS_21BalancedSegmentedArgsE") \
  /* segmented_piece_copy_back_kernel [key-value] */ \
  X(kSegmentedPieceCopyBack, (&segmented_piece_copy_back_kernel<false>), 1024, 0, \
    "_ZN4vrdx32segmented_piece_copy_back_kernelILb0EEEvNS_21BalancedSegmentedArgsE") \
  X(kSegmentedPieceCopyBackV, (&segmented_piece_copy_back_kernel<true>), 1024, 0, \
    "_ZN4vrdx32segmented_piece_copy_back_kernelILb1EEEvNS_21BalancedSegmentedArgsE")

// The kernels of the sorts of 32-bit keys with 64-bit values (vrdxHipCmdWideValueSort*), in a third list behind the other two
// for the same reason.
#define VRDX_WIDE_VALUE_KERNELS(X) \
  /* small_sort_wide_kernel [256 x 16 | 1024 x 8][atomic rank] */ \
  X(kSmallWide256, (&small_sort_wide_kernel<256, 16, false>), 256, SortInWorkgroup64LdsWords(256, 16, true) * 4, \
    "_ZN4vrdx22small_sort_wide_kernelILi256ELi16ELb0EEEvPjPmjPKjS1_") \
  X(kSmallWide256A, (&small_sort_wide_kernel<256, 16, true>), 256, SortInWorkgroup64LdsWords(256, 16, true) * 4, \
    "_ZN4vrdx22small_sort_wide_kernelILi256ELi16ELb1EEEvPjPmjPKjS1_") \
  X(kSmallWide1024, (&small_sort_wide_kernel<1024, 8, false>), 1024, SortInWorkgroup64LdsWords(1024, 8, true) * 4, \
    "_ZN4vrdx22small_sort_wide_kernelILi1024ELi8ELb0EEEvPjPmjPKjS1_") \
  X(kSmallWide1024A, (&small_sort_wide_kernel<1024, 8, true>), 1024, SortInWorkgroup64LdsWords(1024, 8, true) * 4, \
    "_ZN4vrdx22small_sort_wide_kernelILi1024ELi8ELb1EEEvPjPmjPKjS1_") \
  /* the streaming steps: index, gather, copy back (the gather form); split, merge (the two-sorts form) */ \
  X(kIotaWide, (&iota_wide_kernel), kSort64Threads, 0, \
    "_ZN4vrdx16iota_wide_kernelEPjjPKj") \
  X(kGatherWide, (&gather_wide_kernel), kSort64Threads, 0, \
    "_ZN4vrdx18gather_wide_kernelEPKmPKjPmjS3_") \
  X(kCopyBackWide, (&copy_back_wide_kernel), kSort64Threads, 0, \
    "_ZN4vrdx21copy_back_wide_kernelEPmPKmjPKj") \
  X(kSplitWide, (&split_wide_kernel), kSort64Threads, 0, \
    "_ZN4vrdx17split_wide_kernelEPKjPKmPjS4_S4_jS1_") \
  X(kMergeWide, (&merge_wide_kernel), kSort64Threads, 0, \
    "_ZN4vrdx17merge_wide_kernelEPmPKjS2_jS2_") \
  /* ---- vrdxHipCmdWideValueSortSegmented: segmented_small_wide / mid_wide / large_wide_kernel [atomic rank] ---- */ \
  X(kSegmentedWideSmall, (&segmented_small_wide_kernel<false>), 256, SortInWorkgroup64LdsWords(256, 16, true) * 4, \
    "_ZN4vrdx27segmented_small_wide_kernelILb0EEEvNS_17SegmentedWideArgsE") \
  X(kSegmentedWideSmallA, (&segmented_small_wide_kernel<true>), 256, SortInWorkgroup64LdsWords(256, 16, true) * 4, \
    "_ZN4vrdx27segmented_small_wide_kernelILb1EEEvNS_17SegmentedWideArgsE") \
  X(kSegmentedWideMid, (&segmented_mid_wide_kernel<false>), 1024, SortInWorkgroup64LdsWords(1024, 8, true) * 4, \
    "_ZN4vrdx25segmented_mid_wide_kernelILb0EEEvNS_17SegmentedWideArgsE") \
  X(kSegmentedWideMidA, (&segmented_mid_wide_kernel<true>), 1024, SortInWorkgroup64LdsWords(1024, 8, true) * 4, \
    "_ZN4vrdx25segmented_mid_wide_kernelILb1EEEvNS_17SegmentedWideArgsE") \
  X(kSegmentedWideLarge, (&segmented_large_wide_kernel<false>), 1024, SegmentWideLargeLdsWords() * 4, \
    "_ZN4vrdx27segmented_large_wide_kernelILb0EEEvNS_17SegmentedWideArgsE") \
  X(kSegmentedWideLargeA, (&segmented_large_wide_kernel<true>), 1024, SegmentWideLargeLdsWords() * 4, \
    "_ZN4vrdx27segmented_large_wide_kernelILb1EEEvNS_17SegmentedWideArgsE")

#define VRDX_ALL_KERNELS(X) VRDX_KERNELS(X) VRDX_ORDERED32_KERNELS(X) VRDX_WIDE_VALUE_KERNELS(X) VRDX_RANGE_SORT_KERNELS(X) \
  VRDX_BALANCED_SEGMENTED_KERNELS(X)

enum KernelId : int {
#define VRDX_KERNEL_ID(id, stub, threads, ldsBytes, name) id,
  VRDX_KERNELS(VRDX_KERNEL_ID)
  kNumKernels,
  kLastListedKernel = kNumKernels - 1,  // (the ordered list's first id is kNumKernels)
  VRDX_ORDERED32_KERNELS(VRDX_KERNEL_ID)
  VRDX_WIDE_VALUE_KERNELS(VRDX_KERNEL_ID)
  VRDX_RANGE_SORT_KERNELS(VRDX_KERNEL_ID)
  VRDX_BALANCED_SEGMENTED_KERNELS(VRDX_KERNEL_ID)
#undef VRDX_KERNEL_ID
  kNumAllKernels
};

struct KernelShape {
  uint32_t threads;
  uint32_t ldsBytes;
};
static constexpr KernelShape kKernelShapes[kNumAllKernels] = {
#define VRDX_KERNEL_SHAPE(id, stub, threads, ldsBytes, name) {threads, (uint32_t)(ldsBytes)},
    VRDX_ALL_KERNELS(VRDX_KERNEL_SHAPE)
#undef VRDX_KERNEL_SHAPE
};
static_assert(kSmallOrdered256 == kNumKernels, "the ordered list follows the first one");

// The backend's primitives (defined behind this file).  PrepareKernel readies kernel `id` on the current device: it raises
// the kernel's dynamic-LDS limit if it takes dynamic LDS.  LaunchKernel starts it with the list's block size and LDS and
// returns the hipError_t of ITS launch, so that the recorder never has to consult the calling thread's sticky last-error
// state, which an unrelated earlier failure may have set.
static hipError_t PrepareKernel(KernelId id);
static hipError_t LaunchKernel(KernelId id, uint32_t grid, hipStream_t stream, void** params);

template <typename... Args>
static hipError_t Launch(KernelId id, uint32_t grid, hipStream_t stream, Args... args) {
  void* params[] = {static_cast<void*>(&args)...};
  return LaunchKernel(id, grid, stream, params);
}

// a form of a family of four, listed as [key-value][atomic rank]
static KernelId Form(KernelId first, bool keyValue, bool atomicRank) { return KernelId(first + 2 * keyValue + atomicRank); }
// kKeyOrderUint64 starts the plain kernel, which takes no order word; any other word (checked by the caller) its ordered form
template <typename... Args>
static hipError_t LaunchInOrder(uint32_t order, KernelId plain, KernelId ordered, uint32_t grid, hipStream_t stream, Args... args) {
  return order == kKeyOrderUint64 ? Launch(plain, grid, stream, args...) : Launch(ordered, grid, stream, args..., order);
}

hipError_t PrepareKernels() {
  for (int id = 0; id < kNumAllKernels; ++id) {
    const hipError_t e = PrepareKernel(KernelId(id));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// run-time slot counts (even-split and tail-split tiles, PlanTiles in vrdx_plan.h): multiples of 4, at most the geometry's
static bool SlotsFit(const OnesweepArgs& a, uint32_t keysPerThread) {
  return a.slots % 4 == 0 && a.slots <= keysPerThread && a.tailSlots % 4 == 0 && a.tailSlots != 0 &&
         a.tailSlots <= keysPerThread;
}

// tiles of rows x 4096 keys (the scatter's even-split tiles); a tile of full capacity is eight rows
static bool MsdShapeFits(const MsdArgs& a) {
  return (a.bits == 10 || a.bits == 11) && a.tileKeys != 0 && a.tileKeys % 4096u == 0 && a.tileKeys <= kMsdTileKeys;
}

hipError_t LaunchHistogram(hipStream_t stream, uint32_t grid, const uint32_t* keys, uint32_t maxCount,
                           const uint32_t* countPtr, uint32_t* globalHistogram, uint32_t* tickets, void* statusClear,
                           uint32_t statusClearBytes) {
  const uint32_t vecs = statusClearBytes / 16u;  // whole status rows: a multiple of 1 KiB, 128-byte aligned
  return Launch(maxCount >= kHistManyCopiesFrom ? kHistogramLarge : kHistogram, grid, stream, keys, maxCount, countPtr,
                globalHistogram, tickets, statusClear, vecs);
}

// The two-sub-tile kernel exists for keys-only sorts with the one-atomic ranking (the ballot form of it spills
// 152 bytes per lane and ConfigIndex never selected it): its key+value form would hold sub-tile B's keys and
// ranks, A's staging slots and A's values at once and spills (measured 40 GItems/s in round 1; a 768-thread
// form with 168 registers and no spill measured 54.5 GItems/s against 67.2 for onesweep_kernel<1024, 32>,
// profiles/r03_geometry.txt), so it is not built.
hipError_t LaunchOnesweep(hipStream_t stream, int configIndex, uint32_t grid, bool keyValue, bool atomicRank,
                          const OnesweepArgs& args) {
  // kTileConfigs: configs 0-2 are onesweep_kernel of 8, 16 and 32 keys per thread, config 3 the two-sub-tile kernel; only
  // the geometries of 32 keys per thread (2, 3) have forms with run-time slot counts
  if (configIndex < 0 || configIndex >= kNumTileConfigs) return hipErrorInvalidValue;
  const bool split = args.slots != 0;
  if (split && (configIndex < 2 || !SlotsFit(args, 32))) return hipErrorInvalidValue;
  if (configIndex == 3) {
    if (keyValue || !atomicRank) return hipErrorInvalidValue;  // never selected (ConfigIndex)
    return Launch(split ? kPair32S : kPair32, grid, stream, args);
  }
  const KernelId first = split ? kOnesweep32S : configIndex == 0 ? kOnesweep8 : configIndex == 1 ? kOnesweep16 : kOnesweep32;
  return Launch(Form(first, keyValue, atomicRank), grid, stream, args);
}

hipError_t LaunchSmallSort(hipStream_t stream, bool atomicRank, uint32_t* keys, uint32_t* values, uint32_t maxCount,
                           const uint32_t* countPtr, uint32_t* failure) {
  const KernelId first = maxCount <= 256u * 16u ? kSmall256 : kSmall1024;
  return Launch(Form(first, values != nullptr, atomicRank), 1, stream, keys, values, maxCount, countPtr, failure);
}

// The bit-range sorts: the range travels behind the arguments of the whole-key kernel.  Widths 1 ... 31 only (v_bfe_u32 takes a
// width modulo 32; the recorder forwards the one range of 32 bits to the whole-key sort).
hipError_t LaunchSmallSortBits(hipStream_t stream, bool atomicRank, uint32_t* keys, uint32_t* values, uint32_t maxCount,
                               const uint32_t* countPtr, uint32_t* failure, uint32_t beginBit, uint32_t width) {
  if (width < 1u || width > 31u || beginBit + width > 32u || maxCount > kSmallSortMaxElements) return hipErrorInvalidValue;
  const KernelId first = maxCount <= 256u * 16u ? kSmallBits256 : kSmallBits1024;
  return Launch(Form(first, values != nullptr, atomicRank), 1, stream, keys, values, maxCount, countPtr, failure, beginBit, width);
}

hipError_t LaunchBucketSort(hipStream_t stream, bool keyValue, bool atomicRank, const BucketSortArgs& args) {
  KernelId id;
  switch (args.hybridCap) {
    case 1024u * 4u: id = Form(kBucket4, keyValue, atomicRank); break;
    case 1024u * 8u: id = Form(kBucket8, keyValue, atomicRank); break;
    case 1024u * 16u: id = Form(kBucket16, keyValue, atomicRank); break;
    case 1024u * 32u:
      // the one-atomic ranking only (the ballot forms would spill; never recorded: HybridCapacity); key+value stages keys
      // and values through ONE buffer (SharedStage)
      if (!atomicRank) return hipErrorInvalidValue;
      id = keyValue ? kBucket32VA : kBucket32A;
      break;
    default: return hipErrorInvalidValue;
  }
  return Launch(id, VRDX_RADIX, stream, args);
}

// ---- MSD plan -----------------------------------------------------------------------------------------
hipError_t LaunchHistogramMsd(hipStream_t stream, uint32_t grid, const MsdArgs& args) {
  if (!MsdShapeFits(args)) return hipErrorInvalidValue;
  const bool many = args.maxCount >= kHistManyCopiesFrom;
  return Launch(KernelId(kHistogramMsd10 + 2 * ((int)args.bits - 10) - many), grid, stream, args);
}

hipError_t LaunchSpineMsd(hipStream_t stream, const MsdArgs& args) {
  if ((args.bits != 10 && args.bits != 11) || args.tiles > kMsdMaxTiles) return hipErrorInvalidValue;
  return Launch(KernelId(kSpineMsd10 + ((int)args.bits - 10)), (1u << args.bits) / 32u, stream, args);
}

hipError_t LaunchBucketSortHalf(hipStream_t stream, bool keyValue, const MsdArgs& args) {
  if (args.cap != kMsdHalfCap || args.bits != 10) return hipErrorInvalidValue;
  return Launch(keyValue ? kBucketMsdHalfV : kBucketMsdHalf, MsdBucketGrid(args.bits, true), stream, args);
}

// The plan's scatter / bucket launch with the fallback's pass 0 / pass 1 as its second role (bucketLaunch selects which).
// passGrid: the grid LaunchOnesweep would have used for that pass.
hipError_t LaunchMsdFused(hipStream_t stream, bool bucketLaunch, bool keyValue, const MsdArgs& m, const OnesweepArgs& p,
                          uint32_t passGrid) {
  if (!MsdShapeFits(m) || (bucketLaunch && m.cap != (keyValue ? kMsdCapKeyValue : kMsdCapKeys))) return hipErrorInvalidValue;
  const bool split = p.slots != 0;  // the pass's run-time slot counts, checked like LaunchOnesweep does
  if (split && !SlotsFit(p, 32)) return hipErrorInvalidValue;
  // the larger of the two roles' grids, a multiple of 8 (the scatter derives its tile from the grid: eight chunks of tiles,
  // one per XCD; a workgroup beyond its role's range returns).  The bucket launch asks for 2^bits / 2 workgroups
  // (MsdBucketGrid): a pass of up to that many tiles has no idle workgroups, and in the bucket role every workgroup of the
  // grid, whichever role's it is, may draw a bucket.
  const uint32_t planGrid = bucketLaunch ? MsdBucketGrid(m.bits, false) : MsdScatterGrid(m.tiles, keyValue, m.bits);
  const uint32_t grid = 8u * (((planGrid > passGrid ? planGrid : passGrid) + 7u) / 8u);
  const int form = 8 * ((int)m.bits - 10) + 4 * keyValue + 2 * bucketLaunch + split;
  return Launch(KernelId(kMsdScatterOrPass0_10 + form), grid, stream, m, p);
}

// ---- segmented sort ---------------------------------------------------------------------------------
hipError_t LaunchSegmentedClear(hipStream_t stream, const SegmentedArgs& args) {
  return Launch(kSegmentedClear, 1, stream, args);
}

// width == 0: the whole key.  The range forms: the range travels behind SegmentedArgs, widths 1 ... 31 only (v_bfe_u32 takes a
// width modulo 32; the planner forwards the one range of 32 bits to the whole-key kernels).
hipError_t LaunchSegmented(hipStream_t stream, SegmentClass sizeClass, uint32_t grid, bool keyValue, bool atomicRank,
                           const SegmentedArgs& args, uint32_t beginBit, uint32_t width) {
  if (grid == 0 || width > 31u || beginBit + width > 32u) return hipErrorInvalidValue;
  if (width == 0) return Launch(KernelId(kSegmentedSmall - 3 * (2 * keyValue + atomicRank) + sizeClass), grid, stream, args);
  return Launch(Form(KernelId(kSegmentedBitsSmall + 4 * sizeClass), keyValue, atomicRank), grid, stream, args, beginBit, width);
}

// ---- segmented sort of 64-bit keys ------------------------------------------------------------------
hipError_t LaunchSegmentedClear(hipStream_t stream, const Segmented64Args& args) {
  // segmented_clear_kernel reads the failure word and the two counters only
  SegmentedArgs clear = {};
  clear.midCount = args.midCount;
  clear.largeCount = args.largeCount;
  clear.failure = args.failure;
  return Launch(kSegmentedClear, 1, stream, clear);
}

hipError_t LaunchSegmented64(hipStream_t stream, SegmentClass sizeClass, uint32_t grid, bool keyValue, bool atomicRank,
                             const Segmented64Args& args, uint32_t order) {
  if (grid == 0 || !KeyOrderValid(order)) return hipErrorInvalidValue;
  return LaunchInOrder(order, Form(KernelId(kSegmented64Small + 4 * sizeClass), keyValue, atomicRank),
                       Form(KernelId(kSegmented64OrderedSmall + 4 * sizeClass), keyValue, atomicRank), grid, stream, args);
}

// ---- 64-bit keys ------------------------------------------------------------------------------------
// one thread per four elements of the bound (the kernels take the count from countPtr where there is one); an empty launch
// is the planner's business (it lists none).
static uint32_t Sort64Grid(uint32_t maxCount) { return (maxCount + 4u * kSort64Threads - 1u) / (4u * kSort64Threads); }
static bool Sort64Fits(uint32_t maxCount, uint32_t order = kKeyOrderUint64) {
  return maxCount != 0 && maxCount <= VRDX_MAX_ELEMENTS && KeyOrderValid(order);
}

hipError_t LaunchSplit64(hipStream_t stream, bool iota, const uint64_t* keys, uint32_t* lo, uint32_t* other, uint32_t maxCount,
                         const uint32_t* countPtr, uint32_t order) {
  if (!Sort64Fits(maxCount, order)) return hipErrorInvalidValue;
  return LaunchInOrder(order, iota ? kSplit64Iota : kSplit64, iota ? kSplit64OrderedIota : kSplit64Ordered, Sort64Grid(maxCount),
                       stream, keys, lo, other, maxCount, countPtr);
}

hipError_t LaunchMerge64(hipStream_t stream, uint64_t* keys, const uint32_t* lo, const uint32_t* hi, uint32_t maxCount,
                         const uint32_t* countPtr, uint32_t order) {
  if (!Sort64Fits(maxCount, order)) return hipErrorInvalidValue;
  return LaunchInOrder(order, kMerge64, kMerge64Ordered, Sort64Grid(maxCount), stream, keys, lo, hi, maxCount, countPtr);
}

hipError_t LaunchGatherHi64(hipStream_t stream, const uint64_t* keys, const uint32_t* index, uint32_t* hi, uint32_t maxCount,
                            const uint32_t* countPtr, uint32_t order) {
  if (!Sort64Fits(maxCount, order)) return hipErrorInvalidValue;
  return LaunchInOrder(order, kGatherHi64, kGatherHi64Ordered, Sort64Grid(maxCount), stream, keys, index, hi, maxCount, countPtr);
}

hipError_t LaunchPermute64(hipStream_t stream, const uint64_t* keys, const uint32_t* values, const uint32_t* index,
                           uint32_t* hiThenValues, uint64_t* keysOut, uint32_t maxCount, const uint32_t* countPtr, uint32_t order) {
  if (!Sort64Fits(maxCount, order)) return hipErrorInvalidValue;
  return LaunchInOrder(order, kPermute64, kPermute64Ordered, Sort64Grid(maxCount), stream, keys, values, index, hiThenValues,
                       keysOut, maxCount, countPtr);
}

hipError_t LaunchCopyBack64(hipStream_t stream, uint64_t* keys, uint32_t* values, const uint64_t* keysIn,
                            const uint32_t* valuesIn, uint32_t maxCount, const uint32_t* countPtr) {
  if (!Sort64Fits(maxCount)) return hipErrorInvalidValue;
  return Launch(kCopyBack64, Sort64Grid(maxCount), stream, keys, values, keysIn, valuesIn, maxCount, countPtr);
}

// ---- the LDS order check and the calibration spin -----------------------------------------------------
hipError_t LdsOrderCheck(bool* laneOrdered) {
  uint32_t* d = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(uint32_t));
  if (e != hipSuccess) return e;
  uint32_t h = 0xFFFFFFFFu;
  e = hipMemset(d, 0, sizeof(uint32_t));
  uint32_t* const noSticky = nullptr;
  if (e == hipSuccess) e = Launch(kOrderCheck, 512, nullptr, d, noSticky);
  // the packed-counter shape of the MSD plan: two digits to a word
  if (e == hipSuccess) e = Launch(kOrderCheckPacked, 256, nullptr, d, noSticky);
  if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(uint32_t), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e == hipSuccess) *laneOrdered = h == 0;
  return e;
}

hipError_t LaunchLdsOrderRecheck(hipStream_t stream, uint32_t* sticky) {
  uint32_t* const noCount = nullptr;
  const hipError_t e = Launch(kOrderCheck, 8, stream, noCount, sticky);
  if (e != hipSuccess) return e;
  return Launch(kOrderCheckPacked, 8, stream, noCount, sticky);
}

hipError_t LaunchSpin(hipStream_t stream, unsigned long long* out, uint32_t ticks) {
  return Launch(kSpin, 1, stream, out, ticks);
}

// ---- key orders of the 32-bit sorts (VRDX_ORDERED32_KERNELS) ----------------------------------------
hipError_t LaunchSmallSortOrdered(hipStream_t stream, bool atomicRank, uint32_t* keys, uint32_t* values, uint32_t maxCount,
                                  const uint32_t* countPtr, uint32_t* failure, uint32_t order) {
  if (!KeyOrder32Launchable(order) || maxCount > kSmallSortMaxElements) return hipErrorInvalidValue;
  const KernelId first = maxCount <= 256u * 16u ? kSmallOrdered256 : kSmallOrdered1024;
  return Launch(Form(first, values != nullptr, atomicRank), 1, stream, keys, values, maxCount, countPtr, failure, order);
}

// one thread per four keys of the bound
hipError_t LaunchOrder32(hipStream_t stream, bool inverse, uint32_t* keys, uint32_t maxCount, const uint32_t* countPtr,
                         uint32_t order) {
  if (!KeyOrder32Launchable(order) || maxCount == 0 || maxCount > VRDX_MAX_ELEMENTS) return hipErrorInvalidValue;
  const uint32_t grid = (maxCount + 4u * kOrder32Threads - 1u) / (4u * kOrder32Threads);
  return Launch(inverse ? kOrder32Inverse : kOrder32Forward, grid, stream, keys, maxCount, countPtr, order);
}

hipError_t LaunchSegmentedOrdered(hipStream_t stream, SegmentClass sizeClass, uint32_t grid, bool keyValue, bool atomicRank,
                                  const SegmentedArgs& args, uint32_t order) {
  if (grid == 0 || !KeyOrder32Launchable(order)) return hipErrorInvalidValue;
  return Launch(Form(KernelId(kSegmentedOrderedSmall + 4 * sizeClass), keyValue, atomicRank), grid, stream, args, order);
}

// ---- 32-bit keys with 64-bit values (VRDX_WIDE_VALUE_KERNELS) ---------------------------------------
// (three staging planes of the 1024 x 8 form and its wave counters must fit one CU's LDS)
static_assert(kWideSmallMaxElements == 1024u * 8u && SortInWorkgroup64LdsWords(1024, 8, true) * 4 <= 160u * 1024u,
              "small_sort_wide_kernel's largest form");
hipError_t LaunchSmallSortWide(hipStream_t stream, bool atomicRank, uint32_t* keys, uint64_t* values, uint32_t maxCount,
                               const uint32_t* countPtr, uint32_t* failure) {
  if (maxCount == 0 || maxCount > kWideSmallMaxElements) return hipErrorInvalidValue;
  const KernelId first = maxCount <= kWideSmall256Max ? kSmallWide256 : kSmallWide1024;
  return Launch(KernelId(first + atomicRank), 1, stream, keys, values, maxCount, countPtr, failure);
}

hipError_t LaunchIotaWide(hipStream_t stream, uint32_t* index, uint32_t maxCount, const uint32_t* countPtr) {
  if (!Sort64Fits(maxCount)) return hipErrorInvalidValue;
  return Launch(kIotaWide, Sort64Grid(maxCount), stream, index, maxCount, countPtr);
}

hipError_t LaunchGatherWide(hipStream_t stream, const uint64_t* values, const uint32_t* index, uint64_t* out, uint32_t maxCount,
                            const uint32_t* countPtr) {
  if (!Sort64Fits(maxCount)) return hipErrorInvalidValue;
  return Launch(kGatherWide, Sort64Grid(maxCount), stream, values, index, out, maxCount, countPtr);
}

hipError_t LaunchCopyBackWide(hipStream_t stream, uint64_t* values, const uint64_t* in, uint32_t maxCount,
                              const uint32_t* countPtr) {
  if (!Sort64Fits(maxCount)) return hipErrorInvalidValue;
  return Launch(kCopyBackWide, Sort64Grid(maxCount), stream, values, in, maxCount, countPtr);
}

hipError_t LaunchSplitWide(hipStream_t stream, const uint32_t* keys, const uint64_t* values, uint32_t* keysCopy, uint32_t* lo,
                           uint32_t* hi, uint32_t maxCount, const uint32_t* countPtr) {
  if (!Sort64Fits(maxCount)) return hipErrorInvalidValue;
  return Launch(kSplitWide, Sort64Grid(maxCount), stream, keys, values, keysCopy, lo, hi, maxCount, countPtr);
}

hipError_t LaunchMergeWide(hipStream_t stream, uint64_t* values, const uint32_t* lo, const uint32_t* hi, uint32_t maxCount,
                           const uint32_t* countPtr) {
  if (!Sort64Fits(maxCount)) return hipErrorInvalidValue;
  return Launch(kMergeWide, Sort64Grid(maxCount), stream, values, lo, hi, maxCount, countPtr);
}

// ---- segmented sort of 32-bit keys with 64-bit values ---------------------------------------------------
static_assert(kSegWideSmallMax == 256u * 16u && kSegWideMidMax == 1024u * 8u && kSegWideLargeTile == 1024u * 8u &&
                  SegmentWideLargeLdsWords() * 4 <= 160u * 1024u,
              "the segmented wide-value kernels' forms and the large kernel's LDS");
hipError_t LaunchSegmentedClear(hipStream_t stream, const SegmentedWideArgs& args) {
  // segmented_clear_kernel reads the failure word and the two counters only
  SegmentedArgs clear = {};
  clear.midCount = args.midCount;
  clear.largeCount = args.largeCount;
  clear.failure = args.failure;
  return Launch(kSegmentedClear, 1, stream, clear);
}

hipError_t LaunchSegmentedWide(hipStream_t stream, SegmentClass sizeClass, uint32_t grid, bool atomicRank,
                               const SegmentedWideArgs& args) {
  if (grid == 0) return hipErrorInvalidValue;
  return Launch(KernelId(kSegmentedWideSmall + 2 * sizeClass + atomicRank), grid, stream, args);
}

// ---- range sorts beyond one workgroup (VRDX_RANGE_SORT_KERNELS) ---------------------------------------
// widths 1 ... 31 only (v_bfe_u32 takes a width modulo 32; the planner forwards the one range of 32 bits to the whole-key
// sort); at most one chunk per 8192 keys of the bound, so that the rows of counts fit where MakeRangeSortLayout puts them
static_assert(RangeScatterLdsWords(true) * 4 <= 160u * 1024u, "range_scatter_kernel's key+value form");
static bool RangeSortFits(const RangeSortArgs& a, bool passLaunch) {
  return a.width >= 1u && a.width <= 31u && a.beginBit + a.width <= 32u && a.maxCount != 0 && a.maxCount <= VRDX_MAX_ELEMENTS &&
         a.grid != 0 && a.grid == RangeSortGrid(a.maxCount, a.grid) && (!passLaunch || 8u * a.pass < a.width);
}

hipError_t LaunchRangeCount(hipStream_t stream, const RangeSortArgs& args) {
  if (!RangeSortFits(args, true)) return hipErrorInvalidValue;
  return Launch(args.pass == 0 ? kRangeCountFirst : kRangeCount, args.grid, stream, args);
}

hipError_t LaunchRangeScan(hipStream_t stream, const RangeSortArgs& args) {
  if (!RangeSortFits(args, true)) return hipErrorInvalidValue;
  return Launch(kRangeScan, 1, stream, args);
}

hipError_t LaunchRangeScatter(hipStream_t stream, bool keyValue, bool atomicRank, const RangeSortArgs& args) {
  if (!RangeSortFits(args, true) || keyValue != (args.values != nullptr)) return hipErrorInvalidValue;
  return Launch(Form(kRangeScatter, keyValue, atomicRank), args.grid, stream, args);
}

hipError_t LaunchRangeCopyBack(hipStream_t stream, bool keyValue, const RangeSortArgs& args) {
  if (!RangeSortFits(args, false) || keyValue != (args.values != nullptr)) return hipErrorInvalidValue;
  const uint32_t grid = (args.maxCount + 4u * kRangeCopyThreads - 1u) / (4u * kRangeCopyThreads);
  return Launch(keyValue ? kRangeCopyBackV : kRangeCopyBack, grid, stream, args);
}

// ---- the balanced segmented sort (VRDX_BALANCED_SEGMENTED_KERNELS) ------------------------------------
// the caps are those of vrdx_layout.h for this bound and CU count: the tables and rows lie where MakeBalancedSegmentedLayout
// puts them, sized by the same two functions
static bool BalancedSegmentedFits(const BalancedSegmentedArgs& a, bool passLaunch) {
  const SegmentedArgs& s = a.segmented;
  return s.maxCount > kSegSpreadFrom && s.maxCount <= VRDX_MAX_ELEMENTS && s.segmentCount != 0 && a.computeUnits != 0 &&
         a.spreadCap != 0 && a.spreadCap == SegSpreadCap(s.maxCount, a.computeUnits) &&
         a.pieceCap == SegPieceCap(s.maxCount, a.computeUnits) && (!passLaunch || a.pass < VRDX_PASSES);
}

hipError_t LaunchSegmentedSplit(hipStream_t stream, const BalancedSegmentedArgs& args) {
  if (!BalancedSegmentedFits(args, false)) return hipErrorInvalidValue;
  return Launch(kSegmentedSplit, 1, stream, args);
}

hipError_t LaunchSegmentedPieceCount(hipStream_t stream, const BalancedSegmentedArgs& args) {
  if (!BalancedSegmentedFits(args, true)) return hipErrorInvalidValue;
  return Launch(kSegmentedPieceCount, args.pieceCap, stream, args);
}

hipError_t LaunchSegmentedPieceScan(hipStream_t stream, const BalancedSegmentedArgs& args) {
  if (!BalancedSegmentedFits(args, true)) return hipErrorInvalidValue;
  return Launch(kSegmentedPieceScan, args.spreadCap, stream, args);
}

hipError_t LaunchSegmentedPieceScatter(hipStream_t stream, bool keyValue, bool atomicRank, const BalancedSegmentedArgs& args) {
  if (!BalancedSegmentedFits(args, true) || keyValue != (args.segmented.values != nullptr)) return hipErrorInvalidValue;
  return Launch(Form(kSegmentedPieceScatter, keyValue, atomicRank), args.pieceCap, stream, args);
}

hipError_t LaunchSegmentedPieceCopyBack(hipStream_t stream, bool keyValue, const BalancedSegmentedArgs& args) {
  if (!BalancedSegmentedFits(args, false) || keyValue != (args.segmented.values != nullptr)) return hipErrorInvalidValue;
  return Launch(keyValue ? kSegmentedPieceCopyBackV : kSegmentedPieceCopyBack, args.pieceCap, stream, args);
}
