// The single header's backend of the launch layer (vrdx_launch.inc): the kernels of vrdx_kernels.hip as an EMBEDDED code
// object -- the analogue of the reference's header with its SPIR-V arrays spliced in
// (the reference's tools/generate_header.py:5-35, tools/slangc_to_header.py:43-57, src/vk_radix_sort.h.in:85-98,205-232:
// vkCreateShaderModule from the embedded words).  The kernels are compiled ahead of time with
// `hipcc --genco --offload-arch=gfx950`; here they are loaded with hipModuleLoadData and launched with
// hipModuleLaunchKernel, so that a translation unit that defines VRDX_IMPLEMENTATION needs a host compiler and
// libamdhip64 only.
//
// Included (by the generator, which splices vrdx_launch.inc in for the #include below) after vrdx_kernels.h and after
// the array
//   static const unsigned char kVrdxCodeObject[]  /  kVrdxCodeObjectSize.
#include <mutex>

namespace vrdx {

#include "vrdx_launch.inc"

namespace {

constexpr int kMaxDevices = 64;

const char* const kKernelNames[kNumAllKernels] = {
#define VRDX_KERNEL_NAME(id, stub, threads, ldsBytes, name) name,
    VRDX_ALL_KERNELS(VRDX_KERNEL_NAME)
#undef VRDX_KERNEL_NAME
};

// One loaded module per device and, resolved ONCE per device by PrepareKernels (vrdxCreateSorter), the function handle of
// every kernel in the list: a launch is then hipGetDevice + one table read + hipModuleLaunchKernel, with no lock and no
// symbol lookup.
//
// A handle exists only once a sorter has been created on its device.  vrdxHipEventOverheadNs may run before any sorter
// exists: the library launches its spin kernel then, this backend finds an empty slot and the call returns all ones.
struct DeviceKernels {
  hipModule_t module = nullptr;
  hipFunction_t fn[kNumAllKernels] = {};
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

// The table is written under g_moduleMutex by PrepareKernels and read WITHOUT a lock by every launch, possibly while
// another thread creates a sorter on the same device: every slot is published once, with release semantics, and read with
// acquire semantics (a handle is a pointer: the accesses are single atomic words).  A slot that was never resolved reads as
// nullptr and the launch reports hipErrorInvalidDeviceFunction.
hipFunction_t Handle(const hipFunction_t& slot) { return __atomic_load_n(&slot, __ATOMIC_ACQUIRE); }

// Under g_moduleMutex.  A failed load is retried by the next sorter creation.
hipError_t Resolve(DeviceKernels* dev, KernelId id) {
  if (__atomic_load_n(&dev->fn[id], __ATOMIC_RELAXED) != nullptr) return hipSuccess;
  if (dev->module == nullptr) {
    const hipError_t e = hipModuleLoadData(&dev->module, kVrdxCodeObject);
    if (e != hipSuccess) {
      dev->module = nullptr;
      return e;
    }
  }
  hipFunction_t resolved = nullptr;
  const hipError_t e = hipModuleGetFunction(&resolved, dev->module, kKernelNames[id]);
  if (e == hipSuccess) __atomic_store_n(&dev->fn[id], resolved, __ATOMIC_RELEASE);
  return e;
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

}  // namespace

static hipError_t PrepareKernel(KernelId id) {
  DeviceKernels* dev = nullptr;
  hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_moduleMutex);
  if ((e = Resolve(dev, id)) != hipSuccess) return e;
  if (kKernelShapes[id].ldsBytes != 0) RaiseLdsLimit(dev->fn[id], kKernelShapes[id].ldsBytes);
  return hipSuccess;
}

static hipError_t LaunchKernel(KernelId id, uint32_t grid, hipStream_t stream, void** params) {
  DeviceKernels* dev = nullptr;
  const hipError_t e = CurrentDevice(&dev);
  if (e != hipSuccess) return e;
  const hipFunction_t fn = Handle(dev->fn[id]);
  if (fn == nullptr) return hipErrorInvalidDeviceFunction;  // PrepareKernels has not run on this device
  const KernelShape& k = kKernelShapes[id];
  return hipModuleLaunchKernel(fn, grid, 1, 1, k.threads, 1, 1, k.ldsBytes, stream, params, nullptr);
}

}  // namespace vrdx
