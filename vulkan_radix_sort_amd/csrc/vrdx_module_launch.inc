// Launch interface of vrdx_kernels.h on top of an EMBEDDED code object: the single-header distribution
// (tools/generate_single_header.py), the analogue of the reference's header with its SPIR-V arrays
// spliced in (/root/reference/tools/generate_header.py:5-35, tools/slangc_to_header.py:43-57,
// src/vk_radix_sort.h.in:85-98,205-232: vkCreateShaderModule from the embedded words).  The kernels
// are the ones of vrdx_kernels.hip, compiled ahead of time with `hipcc --genco --offload-arch=gfx950`;
// here they are loaded with hipModuleLoadData and launched with hipModuleLaunchKernel, so that a
// translation unit that defines VRDX_IMPLEMENTATION needs a host compiler and libamdhip64 only.
//
// Included (by the generator) after vrdx_kernels.h and after the array
//   static const unsigned char kVrdxCodeObject[]  /  kVrdxCodeObjectSize.
#include <cstdio>
#include <cstring>
#include <mutex>

namespace vrdx {
namespace {

constexpr int kMaxDevices = 64;

// One loaded module per device and, resolved ONCE per device by the Prepare* calls of vrdxCreateSorter, the
// function handle of every kernel the recorder can launch: a launch is then hipGetDevice + one table read +
// hipModuleLaunchKernel, with no lock, no name formatting and no symbol lookup.  Functions are looked up by their
// (Itanium-mangled) kernel names, which follow from the template arguments -- the generator checks every name it
// will ask for against the code object's symbol table.
struct DeviceKernels {
  hipModule_t module = nullptr;
  hipFunction_t histogram[2] = {nullptr, nullptr};       // [few copies, many copies]
  hipFunction_t onesweep[kNumTileConfigs][2][2] = {};    // [config][key-value][atomic rank]
  hipFunction_t onesweepSplit[kNumTileConfigs][2][2] = {};  // forms with run-time slot counts (configs 2 and 3): [config][key-value][atomic rank]
  hipFunction_t small[2][2][2] = {};                     // [256 | 1024 threads][key-value][atomic rank]
  hipFunction_t bucket[4][2][2] = {};                    // [4 | 8 | 16 | 32 keys per thread][key-value][atomic rank]
  hipFunction_t histogramMsd[2][2] = {};                 // the MSD plan: [10 | 11 bits][few copies, many copies]
  hipFunction_t spineMsd[2] = {nullptr, nullptr};        // [10 | 11 bits]
  hipFunction_t scatterMsd[2][2] = {};                   // [10 | 11 bits][key-value]
  hipFunction_t bucket2[2][2] = {};                      // [10 | 11 bits][key-value]
  hipFunction_t bucket2Half[2] = {};                     // ten bits, buckets of <= 16384: [key-value]
  hipFunction_t fused[2][2][2][2] = {};                  // [10 | 11 bits][scatter-or-pass-0 | buckets-or-pass-1][key-value][full | split tiles]
  hipFunction_t segmented[3][2][2] = {};                 // [small | mid | large][key-value][atomic rank]
  hipFunction_t segmentedClear = nullptr;
  hipFunction_t orderCheck = nullptr;
  hipFunction_t orderCheckPacked = nullptr;
  hipFunction_t spin = nullptr;
};
DeviceKernels g_devices[kMaxDevices];
std::mutex g_moduleMutex;  // module load and handle resolution only (sorter creation), never a launch

hipError_t CurrentDevice(DeviceKernels** out) {
  int device = -1;
  const hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  if (device < 0 || device >= kMaxDevices) return hipErrorInvalidDevice;
  *out = &g_devices[device];
  return hipSuccess;
}

// The table is written under g_moduleMutex by the Prepare* calls of a sorter's creation and read WITHOUT a lock by every
// launch, possibly while another thread creates a sorter on the same device: every slot is published once, with release
// semantics, and read with acquire semantics (a handle is a pointer: the accesses are single atomic words).  A slot that
// was never resolved reads as nullptr and the launch reports hipErrorInvalidDeviceFunction.
hipFunction_t Handle(const hipFunction_t& slot) { return __atomic_load_n(&slot, __ATOMIC_ACQUIRE); }

// Under g_moduleMutex.  A failed load is retried by the next sorter creation.
hipError_t Resolve(DeviceKernels* dev, const char* name, hipFunction_t* fn) {
  if (__atomic_load_n(fn, __ATOMIC_RELAXED) != nullptr) return hipSuccess;
  if (dev->module == nullptr) {
    const hipError_t e = hipModuleLoadData(&dev->module, kVrdxCodeObject);
    if (e != hipSuccess) {
      dev->module = nullptr;
      return e;
    }
  }
  hipFunction_t resolved = nullptr;
  const hipError_t e = hipModuleGetFunction(&resolved, dev->module, name);
  if (e == hipSuccess) __atomic_store_n(fn, resolved, __ATOMIC_RELEASE);
  return e;
}

void OnesweepName(char (&name)[128], const TileConfig& c, bool keyValue, bool atomicRank, bool even) {
  if (c.subTiles == 2)  // keys-only, one-atomic ranking
    std::snprintf(name, sizeof(name), "_ZN4vrdx20onesweep_pair_kernelILi%dELi%dELb%dEEEvNS_12OnesweepArgsE", c.threads,
                  c.keysPerThread, even ? 1 : 0);
  else
    std::snprintf(name, sizeof(name), "_ZN4vrdx15onesweep_kernelILi%dELi%dELb%dELb%dELb%dEEEvNS_12OnesweepArgsE", c.threads,
                  c.keysPerThread, keyValue ? 1 : 0, atomicRank ? 1 : 0, even ? 1 : 0);
}

bool HasSplitForms(const TileConfig& c) { return c.keysPerThread == 32; }  // PrepareKernels of vrdx_kernels.hip

size_t OnesweepLdsBytes(const TileConfig& c) {
  // OnesweepLdsWords / PairLdsWords of vrdx_kernels.hip
  const size_t waves = (size_t)c.threads / 64;
  size_t words = (size_t)c.threads * c.keysPerThread + waves * 256;
  if (c.subTiles == 2) words += (size_t)256 * (2 + 2 * ((size_t)c.threads / 256)) + 512;
  return words * sizeof(uint32_t);
}



size_t BucketLdsBytes(int keysPerThread, bool keyValue) {  // SmallSortLdsWords<1024, keysPerThread, keyValue> of vrdx_kernels.hip
  const bool shared = keyValue && keysPerThread == 32;  // SharedStage: keys and values take turns in one buffer
  return ((size_t)1024 * keysPerThread * (keyValue && !shared ? 2 : 1) + (size_t)16 * 256 + 16) * 4;
}

size_t SmallLdsBytes(int threads, bool keyValue) {  // SmallSortLdsWords of vrdx_kernels.hip
  return ((size_t)threads * 16 * (keyValue ? 2 : 1) + (size_t)(threads / 64) * 256 + 16) * 4;
}

// Dynamic LDS beyond 64 KiB.  The runtime takes a module function where it takes a host stub; should a runtime
// refuse, the launch itself decides.  A refusal here must not linger in the calling thread's last-error state,
// but an error the caller already had is the caller's: it is cleared only if the state was clean before.
void RaiseLdsLimit(hipFunction_t fn, size_t bytes) {
  const bool clean = hipPeekAtLastError() == hipSuccess;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
          hipSuccess &&
      clean)
    (void)hipGetLastError();
}

hipError_t Launch(hipFunction_t fn, uint32_t grid, uint32_t block, size_t lds, hipStream_t stream, void** params) {
  if (fn == nullptr) return hipErrorInvalidDeviceFunction;  // Prepare* has not run for this device
  return hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, (unsigned int)lds, stream, params, nullptr);
}

}  // namespace

const TileConfig kTileConfigs[kNumTileConfigs] = {
    {1024, 8, 1}, {1024, 16, 1}, {1024, 32, 1}, {1024, 32, 2},
};

hipError_t PrepareKernels(int configIndex) {
  if (configIndex < 0 || configIndex >= kNumTileConfigs) return hipErrorInvalidValue;
  DeviceKernels* dev = nullptr;
  hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_moduleMutex);
  char name[128];
  if (configIndex == 0) {
    for (int many = 0; many < 2; ++many) {
      const uint32_t copies = many ? kHistCopiesLarge : kHistCopies;
      std::snprintf(name, sizeof(name), "_ZN4vrdx16histogram_kernelILj%uEEEvPKjjS2_PjS3_PDv4_jj", copies);
      if ((e = Resolve(dev, name, &dev->histogram[many])) != hipSuccess) return e;
      RaiseLdsLimit(dev->histogram[many], HistLdsBytes(copies));
    }
  }
  const TileConfig& c = kTileConfigs[configIndex];
  for (int kv = 0; kv < 2; ++kv)
    for (int atomic = 0; atomic < 2; ++atomic) {
      if (c.subTiles == 2 && (kv != 0 || atomic == 0)) continue;  // the two-sub-tile kernel: keys-only, one-atomic ranking
      OnesweepName(name, c, kv != 0, atomic != 0, false);
      if ((e = Resolve(dev, name, &dev->onesweep[configIndex][kv][atomic])) != hipSuccess) return e;
      RaiseLdsLimit(dev->onesweep[configIndex][kv][atomic], OnesweepLdsBytes(c));
      if (HasSplitForms(c)) {
        OnesweepName(name, c, kv != 0, atomic != 0, true);
        if ((e = Resolve(dev, name, &dev->onesweepSplit[configIndex][kv][atomic])) != hipSuccess) return e;
        RaiseLdsLimit(dev->onesweepSplit[configIndex][kv][atomic], OnesweepLdsBytes(c));
      }
    }
  return hipSuccess;
}

hipError_t LaunchHistogram(hipStream_t stream, uint32_t grid, const uint32_t* keys, uint32_t maxCount, const uint32_t* countPtr,
                           uint32_t* globalHistogram, uint32_t* tickets, void* statusClear, uint32_t statusClearBytes) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  const int many = maxCount >= kHistManyCopiesFrom ? 1 : 0;
  const uint32_t copies = many ? kHistCopiesLarge : kHistCopies;
  uint32_t statusVecs = statusClearBytes / 16u;
  void* params[] = {&keys, &maxCount, &countPtr, &globalHistogram, &tickets, &statusClear, &statusVecs};
  return Launch(Handle(dev->histogram[many]), grid, kHistThreads, HistLdsBytes(copies), stream, params);
}

hipError_t LaunchOnesweep(hipStream_t stream, int configIndex, uint32_t grid, bool keyValue, bool atomicRank,
                          const OnesweepArgs& args) {
  if (configIndex < 0 || configIndex >= kNumTileConfigs) return hipErrorInvalidValue;
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  const TileConfig& c = kTileConfigs[configIndex];
  OnesweepArgs copy = args;
  void* params[] = {&copy};
  hipFunction_t fn = Handle(dev->onesweep[configIndex][keyValue ? 1 : 0][atomicRank ? 1 : 0]);
  if (args.slots != 0) {  // run-time slot counts (even-split and tail-split tiles)
    if (!HasSplitForms(c) || args.slots % 4 != 0 || args.slots > (uint32_t)c.keysPerThread || args.tailSlots % 4 != 0 ||
        args.tailSlots == 0 || args.tailSlots > (uint32_t)c.keysPerThread)
      return hipErrorInvalidValue;
    fn = Handle(dev->onesweepSplit[configIndex][keyValue ? 1 : 0][atomicRank ? 1 : 0]);
  }
  return Launch(fn, grid, (uint32_t)c.threads, OnesweepLdsBytes(c), stream, params);
}

hipError_t PrepareSmallSort() {
  DeviceKernels* dev = nullptr;
  hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_moduleMutex);
  for (int big = 0; big < 2; ++big)
    for (int kv = 0; kv < 2; ++kv)
      for (int atomic = 0; atomic < 2; ++atomic) {
        const int threads = big ? 1024 : 256;
        char name[128];
        std::snprintf(name, sizeof(name), "_ZN4vrdx17small_sort_kernelILi%dELi16ELb%dELb%dEEEvPjS1_jPKjS1_", threads, kv, atomic);
        if ((e = Resolve(dev, name, &dev->small[big][kv][atomic])) != hipSuccess) return e;
        RaiseLdsLimit(dev->small[big][kv][atomic], SmallLdsBytes(threads, kv != 0));
      }
  return hipSuccess;
}

hipError_t LaunchSmallSort(hipStream_t stream, bool atomicRank, uint32_t* keys, uint32_t* values, uint32_t maxCount,
                           const uint32_t* countPtr, uint32_t* failure) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  const int big = maxCount <= 256u * 16u ? 0 : 1;
  const int kv = values != nullptr ? 1 : 0;
  void* params[] = {&keys, &values, &maxCount, &countPtr, &failure};
  return Launch(Handle(dev->small[big][kv][atomicRank ? 1 : 0]), 1, big ? 1024u : 256u, SmallLdsBytes(big ? 1024 : 256, kv != 0), stream,
                params);
}

hipError_t PrepareBucketSort() {
  DeviceKernels* dev = nullptr;
  hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_moduleMutex);
  for (int size = 0; size < 4; ++size)
    for (int kv = 0; kv < 2; ++kv)
      for (int atomic = 0; atomic < 2; ++atomic) {
        if (size == 3 && atomic == 0) continue;  // 32768-element buckets: one-atomic ranking only
        char name[128];
        std::snprintf(name, sizeof(name), "_ZN4vrdx18bucket_sort_kernelILi1024ELi%dELb%dELb%dEEEvNS_14BucketSortArgsE",
                      4 << size, kv, atomic);
        if ((e = Resolve(dev, name, &dev->bucket[size][kv][atomic])) != hipSuccess) return e;
        RaiseLdsLimit(dev->bucket[size][kv][atomic], BucketLdsBytes(4 << size, kv != 0));
      }
  return hipSuccess;
}

hipError_t LaunchBucketSort(hipStream_t stream, bool keyValue, bool atomicRank, const BucketSortArgs& args) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  const int size = args.hybridCap == 4096u ? 0 : args.hybridCap == 8192u ? 1 : args.hybridCap == 16384u ? 2 : args.hybridCap == 32768u ? 3 : -1;
  if (size < 0) return hipErrorInvalidValue;
  BucketSortArgs copy = args;
  void* params[] = {&copy};
  return Launch(Handle(dev->bucket[size][keyValue ? 1 : 0][atomicRank ? 1 : 0]), VRDX_RADIX, 1024, BucketLdsBytes(4 << size, keyValue), stream,
                params);
}

// ---- the MSD plan (vrdx_kernels.hip: PrepareMsd, LaunchHistogramMsd, LaunchSpineMsd, LaunchScatterMsd, LaunchBucketSort2) ----
constexpr size_t kOrderCheckPackedLdsBytes = 2 * 16 * 1024 * sizeof(uint32_t);
size_t HistMsdLdsBytesOf(uint32_t copies, uint32_t bits) {  // HistMsdLdsBytes
  return (3u * 256u * copies + 8192u + (1u << bits) + 256u * (copies < 16u ? copies : 16u) + 4u) * 4u;
}
size_t ScatterMsdLdsBytes(uint32_t bits) { return ((size_t)kMsdTileKeys + ((size_t)1 << bits) + 32) * 4; }  // ScatterMsdLdsWords
size_t FusedLdsBytes(uint32_t bits, bool bucketLaunch, bool keyValue) {  // MsdFusedLdsWords<KV>: the larger of the two roles'
  const size_t pass = keyValue ? ((size_t)1024 * 32 + 16 * 256) * 4                                     // OnesweepLdsWords<1024, 32, true>
                               : ((size_t)1024 * 32 + 16 * 256 + (size_t)256 * (2 + 2 * 4) + 512) * 4;  // PairLdsWords<1024, 32>
  const size_t plan = bucketLaunch ? ((size_t)(keyValue ? kMsdCapKeyValue : kMsdCapKeys) + 32) * 4
                                   : ((size_t)kMsdTileKeys + ((size_t)1 << bits) + 32) * 4;
  return pass > plan ? pass : plan;
}
uint32_t MsdScatterGridOf(uint32_t tiles, bool keyValue, uint32_t bits) {  // MsdScatterGrid: keys-only sorts by ten bits take two tiles per workgroup
  const uint32_t units = !keyValue && bits == 10 ? (tiles + 1u) / 2u : tiles;
  return 8u * ((units + 7u) / 8u);
}
size_t Bucket2LdsBytes(bool keyValue) { return ((size_t)(keyValue ? kMsdCapKeyValue : kMsdCapKeys) + 32) * 4; }  // BucketSort2LdsWords

hipError_t PrepareMsd() {
  DeviceKernels* dev = nullptr;
  hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_moduleMutex);
  char name[128];
  if ((e = Resolve(dev, "_ZN4vrdx29lds_order_check_packed_kernelEPjS0_", &dev->orderCheckPacked)) != hipSuccess) return e;
  RaiseLdsLimit(dev->orderCheckPacked, kOrderCheckPackedLdsBytes);
  for (int kv = 0; kv < 2; ++kv) {
    std::snprintf(name, sizeof(name), "_ZN4vrdx24bucket_sort2_half_kernelILj10ELb%dEEEvNS_7MsdArgsE", kv);
    if ((e = Resolve(dev, name, &dev->bucket2Half[kv])) != hipSuccess) return e;
    RaiseLdsLimit(dev->bucket2Half[kv], ((size_t)kMsdHalfCap + 32) * 4);
  }
  for (int b = 0; b < 2; ++b) {
    const uint32_t bits = 10u + (uint32_t)b;
    std::snprintf(name, sizeof(name), "_ZN4vrdx16spine_msd_kernelILj%uEEEvNS_7MsdArgsE", bits);
    if ((e = Resolve(dev, name, &dev->spineMsd[b])) != hipSuccess) return e;
    for (int many = 0; many < 2; ++many) {
      const uint32_t copies = many ? kHistCopiesLarge : kHistCopies;
      std::snprintf(name, sizeof(name), "_ZN4vrdx20histogram_msd_kernelILj%uELj%uEEEvNS_7MsdArgsE", copies, bits);
      if ((e = Resolve(dev, name, &dev->histogramMsd[b][many])) != hipSuccess) return e;
      RaiseLdsLimit(dev->histogramMsd[b][many], HistMsdLdsBytesOf(copies, bits));
    }
    for (int kv = 0; kv < 2; ++kv) {
      std::snprintf(name, sizeof(name), "_ZN4vrdx18scatter_msd_kernelILj%uELb%dEEEvNS_7MsdArgsE", bits, kv);
      if ((e = Resolve(dev, name, &dev->scatterMsd[b][kv])) != hipSuccess) return e;
      RaiseLdsLimit(dev->scatterMsd[b][kv], ScatterMsdLdsBytes(bits));
      std::snprintf(name, sizeof(name), "_ZN4vrdx19bucket_sort2_kernelILj%uELi%dELb%dEEEvNS_7MsdArgsE", bits,
                    (int)((kv ? kMsdCapKeyValue : kMsdCapKeys) / 1024u), kv);
      if ((e = Resolve(dev, name, &dev->bucket2[b][kv])) != hipSuccess) return e;
      RaiseLdsLimit(dev->bucket2[b][kv], Bucket2LdsBytes(kv != 0));
    }
    for (int bucket = 0; bucket < 2; ++bucket)
      for (int kv = 0; kv < 2; ++kv)
        for (int dyn = 0; dyn < 2; ++dyn) {
          std::snprintf(name, sizeof(name), "_ZN4vrdx%sILj%uELb%dELb%dEEEvNS_7MsdArgsENS_12OnesweepArgsE",
                        bucket ? "27msd_buckets_or_pass1_kernel" : "27msd_scatter_or_pass0_kernel", bits, kv, dyn);
          if ((e = Resolve(dev, name, &dev->fused[b][bucket][kv][dyn])) != hipSuccess) return e;
          RaiseLdsLimit(dev->fused[b][bucket][kv][dyn], FusedLdsBytes(bits, bucket != 0, kv != 0));
        }
  }
  return hipSuccess;
}

hipError_t LaunchMsdFused(hipStream_t stream, bool bucketLaunch, bool keyValue, const MsdArgs& m, const OnesweepArgs& p,
                          uint32_t passGrid) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  if ((m.bits != 10 && m.bits != 11) || m.tileKeys == 0 || m.tileKeys % 4096u != 0 || m.tileKeys > kMsdTileKeys ||
      (bucketLaunch && m.cap != (keyValue ? kMsdCapKeyValue : kMsdCapKeys)))
    return hipErrorInvalidValue;
  MsdArgs plan = m;
  OnesweepArgs pass = p;
  void* params[] = {&plan, &pass};
  // (vrdx_kernels.hip, LaunchMsdFusedBits: a multiple of 8 workgroups, the pass's slot counts checked)
  const uint32_t planGrid = bucketLaunch ? (1u << m.bits) / 2u : MsdScatterGridOf(m.tiles, keyValue, m.bits);  // (MsdBucketGrid: two buckets per workgroup)
  const uint32_t grid = 8u * (((planGrid > passGrid ? planGrid : passGrid) + 7u) / 8u);
  if (p.slots != 0 && (p.slots % 4 != 0 || p.slots > 32u || p.tailSlots % 4 != 0 || p.tailSlots == 0 || p.tailSlots > 32u))
    return hipErrorInvalidValue;
  return Launch(Handle(dev->fused[m.bits - 10][bucketLaunch ? 1 : 0][keyValue ? 1 : 0][p.slots != 0 ? 1 : 0]), grid, 1024,
                FusedLdsBytes(m.bits, bucketLaunch, keyValue), stream, params);
}

hipError_t LaunchHistogramMsd(hipStream_t stream, uint32_t grid, const MsdArgs& args) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  if ((args.bits != 10 && args.bits != 11) || args.tileKeys == 0 || args.tileKeys % 4096u != 0 || args.tileKeys > kMsdTileKeys)
    return hipErrorInvalidValue;
  const int many = args.maxCount >= kHistManyCopiesFrom ? 1 : 0;
  MsdArgs copy = args;
  void* params[] = {&copy};
  return Launch(Handle(dev->histogramMsd[args.bits - 10][many]), grid, kHistThreads,
                HistMsdLdsBytesOf(many ? kHistCopiesLarge : kHistCopies, args.bits), stream, params);
}

hipError_t LaunchSpineMsd(hipStream_t stream, const MsdArgs& args) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  if ((args.bits != 10 && args.bits != 11) || args.tiles > kMsdMaxTiles) return hipErrorInvalidValue;
  MsdArgs copy = args;
  void* params[] = {&copy};
  return Launch(Handle(dev->spineMsd[args.bits - 10]), (1u << args.bits) / 32u, 1024, 0, stream, params);
}

hipError_t LaunchScatterMsd(hipStream_t stream, bool keyValue, const MsdArgs& args) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  if ((args.bits != 10 && args.bits != 11) || args.tileKeys == 0 || args.tileKeys % 4096u != 0 || args.tileKeys > kMsdTileKeys)
    return hipErrorInvalidValue;
  MsdArgs copy = args;
  void* params[] = {&copy};
  return Launch(Handle(dev->scatterMsd[args.bits - 10][keyValue ? 1 : 0]), MsdScatterGridOf(args.tiles, keyValue, args.bits), 1024,
                ScatterMsdLdsBytes(args.bits), stream, params);
}

hipError_t LaunchBucketSort2(hipStream_t stream, bool keyValue, const MsdArgs& args) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  MsdArgs copy = args;
  void* params[] = {&copy};
  if (args.cap == kMsdHalfCap && args.bits == 10)
    return Launch(Handle(dev->bucket2Half[keyValue ? 1 : 0]), 1u << args.bits, 512, ((size_t)kMsdHalfCap + 32) * 4, stream, params);
  if ((args.bits != 10 && args.bits != 11) || args.cap != (keyValue ? kMsdCapKeyValue : kMsdCapKeys)) return hipErrorInvalidValue;
  // (MsdBucketGrid of vrdx_kernels.hip: the full-size kernel takes two buckets per workgroup)
  return Launch(Handle(dev->bucket2[args.bits - 10][keyValue ? 1 : 0]), (1u << args.bits) / 2u, 1024, Bucket2LdsBytes(keyValue), stream,
                params);
}

// ---- the segmented sort (vrdx_kernels.hip: PrepareSegmented, LaunchSegmented*) ----
size_t SegmentedLdsBytesOf(int which, bool keyValue) {
  if (which == 0) return SmallLdsBytes(256, keyValue);
  if (which == 1) return SmallLdsBytes(1024, keyValue);
  // SegmentLargeLdsWords: staging | wave counters | scan scratch | bases | tile starts | tile counts | 16
  return ((size_t)kSegLargeTile * (keyValue ? 2 : 1) + 16 * 256 + 16 + 4 * 256 + 256 + 256 + 16) * 4;
}

hipError_t PrepareSegmented() {
  DeviceKernels* dev = nullptr;
  hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_moduleMutex);
  if ((e = Resolve(dev, "_ZN4vrdx22segmented_clear_kernelENS_13SegmentedArgsE", &dev->segmentedClear)) != hipSuccess) return e;
  static const char* const kNames[3] = {"22segmented_small_kernel", "20segmented_mid_kernel", "22segmented_large_kernel"};
  for (int which = 0; which < 3; ++which)
    for (int kv = 0; kv < 2; ++kv)
      for (int atomic = 0; atomic < 2; ++atomic) {
        char name[128];
        std::snprintf(name, sizeof(name), "_ZN4vrdx%sILb%dELb%dEEEvNS_13SegmentedArgsE", kNames[which], kv, atomic);
        if ((e = Resolve(dev, name, &dev->segmented[which][kv][atomic])) != hipSuccess) return e;
        RaiseLdsLimit(dev->segmented[which][kv][atomic], SegmentedLdsBytesOf(which, kv != 0));
      }
  return hipSuccess;
}

hipError_t LaunchSegmentedKernel(int which, hipStream_t stream, uint32_t grid, bool keyValue, bool atomicRank,
                                 const SegmentedArgs& args) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  if (grid == 0) return hipErrorInvalidValue;
  SegmentedArgs copy = args;
  void* params[] = {&copy};
  return Launch(Handle(dev->segmented[which][keyValue ? 1 : 0][atomicRank ? 1 : 0]), grid, which == 0 ? 256u : 1024u,
                SegmentedLdsBytesOf(which, keyValue), stream, params);
}
hipError_t LaunchSegmentedClear(hipStream_t stream, const SegmentedArgs& args) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  SegmentedArgs copy = args;
  void* params[] = {&copy};
  return Launch(Handle(dev->segmentedClear), 1, 64, 0, stream, params);
}
hipError_t LaunchSegmentedSmall(hipStream_t stream, uint32_t grid, bool keyValue, bool atomicRank, const SegmentedArgs& args) {
  return LaunchSegmentedKernel(0, stream, grid, keyValue, atomicRank, args);
}
hipError_t LaunchSegmentedMid(hipStream_t stream, uint32_t grid, bool keyValue, bool atomicRank, const SegmentedArgs& args) {
  return LaunchSegmentedKernel(1, stream, grid, keyValue, atomicRank, args);
}
hipError_t LaunchSegmentedLarge(hipStream_t stream, uint32_t grid, bool keyValue, bool atomicRank, const SegmentedArgs& args) {
  return LaunchSegmentedKernel(2, stream, grid, keyValue, atomicRank, args);
}

hipError_t LaunchLdsOrderRecheck(hipStream_t stream, uint32_t* sticky) {
  DeviceKernels* dev = nullptr;
  hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  uint32_t* noCount = nullptr;
  void* params[] = {&noCount, &sticky};
  e = Launch(Handle(dev->orderCheck), 8, 1024, 0, stream, params);
  if (e != hipSuccess) return e;
  return Launch(Handle(dev->orderCheckPacked), 8, 1024, kOrderCheckPackedLdsBytes, stream, params);
}

hipError_t LaunchSpin(hipStream_t stream, unsigned long long* out, uint32_t ticks) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  void* params[] = {&out, &ticks};
  return Launch(Handle(dev->spin), 1, 64, 0, stream, params);
}

hipError_t LdsOrderCheck(bool* laneOrdered) {
  DeviceKernels* dev = nullptr;
  hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  {
    std::lock_guard<std::mutex> lock(g_moduleMutex);
    e = Resolve(dev, "_ZN4vrdx22lds_order_check_kernelEPjS0_", &dev->orderCheck);
    if (e == hipSuccess) e = Resolve(dev, "_ZN4vrdx11spin_kernelEPyj", &dev->spin);
  }
  if (e != hipSuccess) return e;
  uint32_t* d = nullptr;
  e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(uint32_t));
  if (e != hipSuccess) return e;
  uint32_t h = 0xFFFFFFFFu;
  e = hipMemset(d, 0, sizeof(uint32_t));
  if (e == hipSuccess) {
    uint32_t* noSticky = nullptr;
    void* params[] = {&d, &noSticky};
    e = Launch(Handle(dev->orderCheck), 512, 1024, 0, nullptr, params);
    // the packed-counter shape of the MSD plan (PrepareMsd has resolved it and raised its LDS limit)
    if (e == hipSuccess) e = Launch(Handle(dev->orderCheckPacked), 256, 1024, kOrderCheckPackedLdsBytes, nullptr, params);
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(uint32_t), hipMemcpyDeviceToHost);
  }
  (void)hipFree(d);
  if (e == hipSuccess) *laneOrdered = h == 0;
  return e;
}

}  // namespace vrdx
