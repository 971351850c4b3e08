// CPU-only trace of what the host recorder (vrdx_api.cpp) enqueues: the recorder itself, compiled here with a third backend
// of the launch layer (vrdx_launch.inc) that logs every launch instead of starting it, and a fake HIP runtime that logs
// every fill, copy and event record.  Nothing of ROCm is linked (hip_runtime_api.h gives the types).
//   record_trace <cus>...     for every CU count: every vrdxCmd* / vrdxHipCmd* entry point over a fixed matrix of counts,
//                             segment counts, bit ranges and order words, keys-only and key+value, with a 15-slot pool
// Output: the kernel list once (id, mangled name, threads, LDS bytes), then one row per CU count and entry point (segmented
// sorts: and count) with the number of the BODY of each of its calls (per count or segment count, one per bit range / order word).  A body is one line,
// printed where it first occurs (most calls repeat one): the launches (id:grid), fills, copies (addresses relative to the
// caller's buffers) and event records (E<slot>) in the order they were enqueued, the host bits of vrdxHipReadSorterStatus,
// how far the sorter's two counters moved and each slot's source (!: not recorded).  tests/test_record_trace.py compares the output with
// tests/golden/record_trace.txt byte for byte.  Kernel ARGUMENTS are not in the log (the backend sees void** only): the GPU
// suites hold those.
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../vulkan_radix_sort_amd/csrc/vrdx_kernels.h"
#include "../../vulkan_radix_sort_amd/csrc/vrdx_layout.h"

namespace trace {

std::string g_log;     // the body of the call being recorded
bool g_logging = false;
int g_computeUnits = 0;

void Log(const char* format, ...) {
  if (!g_logging) return;
  char line[256];
  va_list args;
  va_start(args, format);
  std::vsnprintf(line, sizeof(line), format, args);
  va_end(args);
  g_log += line;
}

// The caller's buffers are address ranges nobody dereferences (a sort of 2^30 elements is recorded, not run).
constexpr uintptr_t kRange = (uintptr_t)1 << 40;
constexpr uintptr_t kStorage = (uintptr_t)1 << 44, kKeys = (uintptr_t)2 << 44, kValues = (uintptr_t)3 << 44,
                    kIndirect = (uintptr_t)4 << 44, kOffsets = (uintptr_t)5 << 44;
std::vector<std::pair<uintptr_t, size_t>> g_allocations;  // what hipMalloc handed out: host memory

bool Allocated(const void* p) {
  for (const auto& a : g_allocations)
    if ((uintptr_t)p >= a.first && (uintptr_t)p < a.first + a.second) return true;
  return false;
}

std::string Name(const void* p) {
  const uintptr_t a = (uintptr_t)p;
  if (Allocated(p)) return "sorter";
  const std::pair<uintptr_t, const char*> buffers[] = {
      {kStorage, "storage"}, {kKeys, "keys"}, {kValues, "values"}, {kIndirect, "indirect"}, {kOffsets, "offsets"}};
  for (const auto& b : buffers)
    if (a >= b.first && a < b.first + kRange) return std::string(b.second) + "+" + std::to_string(a - b.first);
  return "host";
}

}  // namespace trace

// ---- the launch backend ----
namespace vrdx {

#include "../../vulkan_radix_sort_amd/csrc/vrdx_launch.inc"

static const char* const kKernelIds[kNumKernels] = {
#define VRDX_KERNEL_ID_TEXT(id, stub, threads, ldsBytes, name) #id,
    VRDX_KERNELS(VRDX_KERNEL_ID_TEXT)
#undef VRDX_KERNEL_ID_TEXT
};
static const char* const kKernelNames[kNumKernels] = {
#define VRDX_KERNEL_NAME(id, stub, threads, ldsBytes, name) name,
    VRDX_KERNELS(VRDX_KERNEL_NAME)
#undef VRDX_KERNEL_NAME
};

static hipError_t PrepareKernel(KernelId) { return hipSuccess; }

static hipError_t LaunchKernel(KernelId id, uint32_t grid, hipStream_t, void**) {
  trace::Log(" %s:%u", kKernelIds[id], grid);
  return hipSuccess;
}

}  // namespace vrdx

// ---- the fake HIP runtime: what vrdx_api.cpp and vrdx_launch.inc call ----
extern "C" {

hipError_t hipGetDevice(int* device) { *device = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceCount(int* count) { *count = 1; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int) {
  std::memset(prop, 0, sizeof(*prop));
  std::strcpy(prop->gcnArchName, "gfx950:sramecc+:xnack-");
  prop->multiProcessorCount = trace::g_computeUnits;
  return hipSuccess;
}
hipError_t hipStreamGetDevice(hipStream_t, int* device) { *device = 0; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t, int) { *value = 100000; return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "error"; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* status) {
  *status = hipStreamCaptureStatusNone;
  return hipSuccess;
}

hipError_t hipMalloc(void** p, size_t bytes) {
  *p = std::calloc(1, bytes);
  trace::g_allocations.emplace_back((uintptr_t)*p, bytes);
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  for (size_t i = 0; i < trace::g_allocations.size(); ++i)
    if (trace::g_allocations[i].first == (uintptr_t)p) {
      trace::g_allocations.erase(trace::g_allocations.begin() + i);
      break;
    }
  std::free(p);
  return hipSuccess;
}
// a fill or copy is carried out where it touches what hipMalloc handed out (the sorter's words: the order check and the
// status read back 0) and logged either way
hipError_t hipMemset(void* p, int value, size_t bytes) {
  if (trace::Allocated(p)) std::memset(p, value, bytes);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* p, int value, size_t bytes, hipStream_t) {
  trace::Log(" fill(%s,%d,%zu)", trace::Name(p).c_str(), value, bytes);
  return hipMemset(p, value, bytes);
}
hipError_t hipMemcpy(void* to, const void* from, size_t bytes, hipMemcpyKind) {
  const bool real = (trace::Allocated(to) || trace::Name(to) == "host") && (trace::Allocated(from) || trace::Name(from) == "host");
  if (real) std::memcpy(to, from, bytes);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* to, const void* from, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  trace::Log(" copy(%s<-%s,%zu)", trace::Name(to).c_str(), trace::Name(from).c_str(), bytes);
  return hipMemcpy(to, from, bytes, kind);
}

// an event is its index + 1; the pool creates its events in slot order
static uintptr_t g_eventsCreated = 0;
hipError_t hipEventCreate(hipEvent_t* event) { *event = reinterpret_cast<hipEvent_t>(++g_eventsCreated); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t event, hipStream_t) {
  trace::Log(" E%u", (unsigned)(reinterpret_cast<uintptr_t>(event) - 1));
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }

}  // extern "C"

// ---- the recorder itself ----
#include "../../vulkan_radix_sort_amd/csrc/vrdx_api.cpp"

namespace trace {

constexpr uint32_t kSlots = 15;
std::map<std::string, int> g_bodies;

struct Recorder {
  VrdxSorter sorter = nullptr;
  VkQueryPool pool = nullptr;
  VkCommandBuffer stream = reinterpret_cast<VkCommandBuffer>((uintptr_t)0x77);
  std::string row;  // the body numbers of the calls of the row being written

  // records one call and adds its body's number to the row; a body is printed where it first occurs
  template <typename Call>
  void Record(Call&& call) {
    VrdxHipQueryPool* p = reinterpret_cast<VrdxHipQueryPool*>(pool);
    for (uint32_t i = 0; i < p->count; ++i) {
      p->slots[i].recorded = false;
      p->slots[i].source = i;
    }
    const uint32_t sorts = sorter->sortsRecorded.load(), plans = sorter->plansRecorded.load();
    g_log.clear();
    g_logging = true;
    call();
    g_logging = false;
    const uint32_t status = vrdxHipReadSorterStatus(sorter, stream);
    char line[256];
    int at = std::snprintf(line, sizeof(line), " | status %08x sorts +%u plans +%u source", status,
                           sorter->sortsRecorded.load() - sorts, sorter->plansRecorded.load() - plans);
    for (uint32_t i = 0; i < p->count; ++i)
      at += std::snprintf(line + at, sizeof(line) - at, " %s%u", p->slots[i].recorded ? "" : "!", p->slots[i].source);
    g_log += line;
    const auto found = g_bodies.emplace(g_log, (int)g_bodies.size());
    if (found.second) std::printf("body %d:%s\n", found.first->second, g_log.c_str());
    row += " " + std::to_string(found.first->second);
  }
  void EndRow(int cus, const char* entry) {
    std::printf("cus %d %s:%s\n", cus, entry, row.c_str());
    row.clear();
  }
  void EndRow(int cus, const char* entry, uint32_t n) { EndRow(cus, (std::string(entry) + " n " + std::to_string(n)).c_str()); }
};

void Matrix(int cus) {
  g_computeUnits = cus;
  g_eventsCreated = 0;
  Recorder r;
  VrdxSorterCreateInfo info = {};
  if (vrdxCreateSorter(&info, &r.sorter) != VK_SUCCESS || vrdxHipCreateQueryPool(kSlots, &r.pool) != VK_SUCCESS) {
    std::printf("no sorter\n");
    std::exit(1);
  }
  const uint32_t counts[] = {0u, 1u, 4096u, 4097u, 8192u, 8193u, 16384u, 16385u, (1u << 20) + 3u, 0x3FFFFFFCu, 0x3FFFFFFDu};
  const uint32_t segments[] = {0u, 1u, 2u * (uint32_t)cus - 1u, 2u * (uint32_t)cus + 1u, (1u << 20) + 1u};
  const uint32_t ranges[][2] = {{0, 32}, {5, 5}, {3, 20}, {9, 4}, {0, 33}};
  const uint32_t orders[] = {0u, 1u, 2u, 0x100u, 0x102u, 3u, 0x200u};
  // every buffer at an offset: the storage 48 bytes behind a 128-byte line, so that the layouts' pads are not zero
  const VkCommandBuffer cb = r.stream;
  const VrdxSorter s = r.sorter;
  const VkQueryPool q = r.pool;
  const VkBuffer st = reinterpret_cast<VkBuffer>(kStorage), k = reinterpret_cast<VkBuffer>(kKeys), v = reinterpret_cast<VkBuffer>(kValues),
                 in = reinterpret_cast<VkBuffer>(kIndirect), of = reinterpret_cast<VkBuffer>(kOffsets);
  const VkDeviceSize so = 48, ko = 8, vo = 4, io = 12, oo = 4;
  // the sorts: a row per entry point, the counts one after the other, each closed by | (one call, or one per bit range / order word)
  const auto row = [&](const char* entry, auto&& call) {
    for (const uint32_t n : counts) r.Record([&] { call(n); }), r.row += " |";
    r.EndRow(cus, entry);
  };
  const auto rowOfRanges = [&](const char* entry, auto&& call) {
    for (const uint32_t n : counts) {
      for (const auto& range : ranges) r.Record([&] { call(n, range[0], range[1]); });
      r.row += " |";
    }
    r.EndRow(cus, entry);
  };
  const auto rowOfOrders = [&](const char* entry, auto&& call) {
    for (const uint32_t n : counts) {
      for (const uint32_t order : orders) r.Record([&] { call(n, order); });
      r.row += " |";
    }
    r.EndRow(cus, entry);
  };
  using u32 = uint32_t;
  row("vrdxCmdSort", [&](u32 n) { vrdxCmdSort(cb, s, n, k, ko, st, so, q, 0); });
  row("vrdxCmdSortIndirect", [&](u32 n) { vrdxCmdSortIndirect(cb, s, n, in, io, k, ko, st, so, q, 0); });
  row("vrdxCmdSortKeyValue", [&](u32 n) { vrdxCmdSortKeyValue(cb, s, n, k, ko, v, vo, st, so, q, 0); });
  row("vrdxCmdSortKeyValueIndirect", [&](u32 n) { vrdxCmdSortKeyValueIndirect(cb, s, n, in, io, k, ko, v, vo, st, so, q, 0); });
  rowOfRanges("vrdxHipCmdSortBits", [&](u32 n, u32 b, u32 e) { vrdxHipCmdSortBits(cb, s, n, k, ko, b, e, st, so, q, 0); });
  rowOfRanges("vrdxHipCmdSortBitsKeyValue",
              [&](u32 n, u32 b, u32 e) { vrdxHipCmdSortBitsKeyValue(cb, s, n, k, ko, v, vo, b, e, st, so, q, 0); });
  rowOfRanges("vrdxHipCmdSortBitsIndirect",
              [&](u32 n, u32 b, u32 e) { vrdxHipCmdSortBitsIndirect(cb, s, n, in, io, k, ko, b, e, st, so, q, 0); });
  rowOfRanges("vrdxHipCmdSortBitsKeyValueIndirect", [&](u32 n, u32 b, u32 e) {
    vrdxHipCmdSortBitsKeyValueIndirect(cb, s, n, in, io, k, ko, v, vo, b, e, st, so, q, 0);
  });
  row("vrdxHipCmdSort64", [&](u32 n) { vrdxHipCmdSort64(cb, s, n, k, ko, st, so, q, 0); });
  row("vrdxHipCmdSort64KeyValue", [&](u32 n) { vrdxHipCmdSort64KeyValue(cb, s, n, k, ko, v, vo, st, so, q, 0); });
  row("vrdxHipCmdSort64Indirect", [&](u32 n) { vrdxHipCmdSort64Indirect(cb, s, n, in, io, k, ko, st, so, q, 0); });
  row("vrdxHipCmdSort64KeyValueIndirect", [&](u32 n) { vrdxHipCmdSort64KeyValueIndirect(cb, s, n, in, io, k, ko, v, vo, st, so, q, 0); });
  rowOfOrders("vrdxHipCmdSort64Ordered", [&](u32 n, u32 o) { vrdxHipCmdSort64Ordered(cb, s, n, k, ko, o, st, so, q, 0); });
  rowOfOrders("vrdxHipCmdSort64OrderedKeyValue",
              [&](u32 n, u32 o) { vrdxHipCmdSort64OrderedKeyValue(cb, s, n, k, ko, v, vo, o, st, so, q, 0); });
  rowOfOrders("vrdxHipCmdSort64OrderedIndirect",
              [&](u32 n, u32 o) { vrdxHipCmdSort64OrderedIndirect(cb, s, n, in, io, k, ko, o, st, so, q, 0); });
  rowOfOrders("vrdxHipCmdSort64OrderedKeyValueIndirect", [&](u32 n, u32 o) {
    vrdxHipCmdSort64OrderedKeyValueIndirect(cb, s, n, in, io, k, ko, v, vo, o, st, so, q, 0);
  });
  for (const uint32_t n : counts) {
    // the segmented sorts: a row per entry point, the segment counts one after the other (and within each, the ranges / orders)
    const auto segmentedRow = [&](const char* entry, auto&& call) {
      for (const uint32_t m : segments) r.Record([&] { call(m); }), r.row += " |";
      r.EndRow(cus, entry, n);
    };
    const auto segmentedRowOfRanges = [&](const char* entry, auto&& call) {
      for (const uint32_t m : segments) {
        for (const auto& range : ranges) r.Record([&] { call(m, range[0], range[1]); });
        r.row += " |";
      }
      r.EndRow(cus, entry, n);
    };
    const auto segmentedRowOfOrders = [&](const char* entry, auto&& call) {
      for (const uint32_t m : segments) {
        for (const uint32_t order : orders) r.Record([&] { call(m, order); });
        r.row += " |";
      }
      r.EndRow(cus, entry, n);
    };
    segmentedRow("vrdxHipCmdSortSegmented", [&](uint32_t m) { vrdxHipCmdSortSegmented(cb, s, n, m, of, oo, k, ko, st, so, q, 0); });
    segmentedRow("vrdxHipCmdSortSegmentedKeyValue",
                 [&](uint32_t m) { vrdxHipCmdSortSegmentedKeyValue(cb, s, n, m, of, oo, k, ko, v, vo, st, so, q, 0); });
    segmentedRowOfRanges("vrdxHipCmdSortSegmentedBits", [&](uint32_t m, uint32_t b, uint32_t e) {
      vrdxHipCmdSortSegmentedBits(cb, s, n, m, of, oo, k, ko, b, e, st, so, q, 0);
    });
    segmentedRowOfRanges("vrdxHipCmdSortSegmentedBitsKeyValue", [&](uint32_t m, uint32_t b, uint32_t e) {
      vrdxHipCmdSortSegmentedBitsKeyValue(cb, s, n, m, of, oo, k, ko, v, vo, b, e, st, so, q, 0);
    });
    segmentedRow("vrdxHipCmdSortSegmented64", [&](uint32_t m) { vrdxHipCmdSortSegmented64(cb, s, n, m, of, oo, k, ko, st, so, q, 0); });
    segmentedRow("vrdxHipCmdSortSegmented64KeyValue",
                 [&](uint32_t m) { vrdxHipCmdSortSegmented64KeyValue(cb, s, n, m, of, oo, k, ko, v, vo, st, so, q, 0); });
    segmentedRowOfOrders("vrdxHipCmdSortSegmented64Ordered", [&](uint32_t m, uint32_t o) {
      vrdxHipCmdSortSegmented64Ordered(cb, s, n, m, of, oo, k, ko, o, st, so, q, 0);
    });
    segmentedRowOfOrders("vrdxHipCmdSortSegmented64OrderedKeyValue", [&](uint32_t m, uint32_t o) {
      vrdxHipCmdSortSegmented64OrderedKeyValue(cb, s, n, m, of, oo, k, ko, v, vo, o, st, so, q, 0);
    });
  }

  // ---- the repeat of the lane-order check behind every 65536th sort: each kind of call with the count one short of it ----
  const auto atTheRecheck = [&](const char* what, uint32_t n, auto&& call) {
    r.sorter->sortsRecorded.store(0xFFFFu);
    r.Record(call);
    r.EndRow(cus, what, n);
  };
  atTheRecheck("sort 65536: vrdxCmdSort (one workgroup: not counted)", 4096, [&] { vrdxCmdSort(cb, s, 4096, k, ko, st, so, q, 0); });
  atTheRecheck("sort 65536: vrdxCmdSort", 16385, [&] { vrdxCmdSort(cb, s, 16385, k, ko, st, so, q, 0); });
  atTheRecheck("sort 65536: vrdxHipCmdSort64", 16385, [&] { vrdxHipCmdSort64(cb, s, 16385, k, ko, st, so, q, 0); });
  atTheRecheck("sort 65536: vrdxHipCmdSort64", 4096, [&] { vrdxHipCmdSort64(cb, s, 4096, k, ko, st, so, q, 0); });
  atTheRecheck("sort 65536: vrdxHipCmdSortSegmented segments 2", 4096,
               [&] { vrdxHipCmdSortSegmented(cb, s, 4096, 2, of, oo, k, ko, st, so, q, 0); });
  atTheRecheck("sort 65536: vrdxHipCmdSortSegmented segments 0", 4096,
               [&] { vrdxHipCmdSortSegmented(cb, s, 4096, 0, of, oo, k, ko, st, so, q, 0); });
  atTheRecheck("sort 65536: vrdxHipCmdSortSegmented64Ordered segments 2 order 0x1", 4096,
               [&] { vrdxHipCmdSortSegmented64Ordered(cb, s, 4096, 2, of, oo, k, ko, 1, st, so, q, 0); });

  // ---- no pool, and a pool that ends inside the sort's slots ----
  r.Record([&] { vrdxHipCmdSortSegmented(cb, s, 4097, 2, of, oo, k, ko, st, so, nullptr, 0); });
  r.EndRow(cus, "no pool: vrdxHipCmdSortSegmented segments 2", 4097);
  r.Record([&] { vrdxHipCmdSort64KeyValue(cb, s, 16385, k, ko, v, vo, st, so, q, 12); });
  r.EndRow(cus, "query 12: vrdxHipCmdSort64KeyValue", 16385);

  vrdxHipDestroyQueryPool(r.pool);
  vrdxDestroySorter(r.sorter);
}

}  // namespace trace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: record_trace <compute units>...\n");
    return 2;
  }
  for (int id = 0; id < vrdx::kNumKernels; ++id)
    std::printf("kernel %s %s %u %u\n", vrdx::kKernelIds[id], vrdx::kKernelNames[id], vrdx::kKernelShapes[id].threads,
                vrdx::kKernelShapes[id].ldsBytes);
  std::printf("columns: bit ranges [0,32) [5,5) [3,20) [9,4) [0,33); order words 0 1 2 0x100 0x102 3 0x200; each closed by |: the "
              "counts 0 1 4096 4097 8192 8193 16384 16385 2^20+3 2^30-4 2^30-3 (sorts), the segment counts 0 1 2cus-1 2cus+1 2^20+1 "
              "(segmented sorts)\n");
  for (int i = 1; i < argc; ++i) trace::Matrix(std::atoi(argv[i]));
  return 0;
}
