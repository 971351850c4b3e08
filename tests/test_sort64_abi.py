"""CPU-only checks of the 64-bit sorts (vrdxHipCmdSort64[KeyValue]): the C-ABI surface, the header in C and C++, the single
header's implementation object, the kernels in the gfx950 code object, the storage carving (MakeSort64Layout) and the
host-side argument checks of vulkan_radix_sort_amd.sort64."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
SINGLE_HEADER = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
NAMES = ("vrdxHipGetSorter64StorageRequirements", "vrdxHipGetSorter64KeyValueStorageRequirements", "vrdxHipCmdSort64",
         "vrdxHipCmdSort64KeyValue")
KERNELS = ("split64_kernel", "merge64_kernel", "gather_hi64_kernel", "permute64_kernel", "copy_back64_kernel")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(vrdx[A-Z]\w+)\s*\(", text))


def _single_header():
    """The generated header, regenerated when it is older than what it is made from."""
    sources = [HEADER, os.path.join(ROOT, "tools", "generate_single_header.py")]
    csrc = os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc")
    sources += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.startswith("vrdx_")]
    if not os.path.exists(SINGLE_HEADER) or os.path.getmtime(SINGLE_HEADER) < max(os.path.getmtime(s) for s in sources):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", SINGLE_HEADER],
                       check=True)
    return SINGLE_HEADER


def test_header_library_and_python_agree_on_the_sort64_entry_points():
    import vulkan_radix_sort_amd as vrdx
    declared = _declared()
    lib = vrdx.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in vrdx.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None, name
    assert callable(vrdx.sort64)
    for method in ("storage_requirements64", "cmd_sort64", "cmd_sort64_key_value"):
        assert callable(getattr(vrdx.Sorter, method)), method


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_sort64_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*size)(VrdxSorter, uint32_t, VrdxSorterStorageRequirements*) = vrdxHipGetSorter64StorageRequirements;\n"
        "  void (*sizePairs)(VrdxSorter, uint32_t, VrdxSorterStorageRequirements*) = vrdxHipGetSorter64KeyValueStorageRequirements;\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkQueryPool,\n"
        "               uint32_t) = vrdxHipCmdSort64;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "                VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSort64KeyValue;\n"
        "  return (size != 0 && sizePairs != 0 && keys != 0 && pairs != 0) ? 0 : 1;\n}\n")
    obj = tmp_path / "s.o"
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                   check=True)


def test_single_header_implementation_exports_the_sort64_entry_points(tmp_path):
    header = _single_header()
    (tmp_path / "impl.cc").write_text('#define VRDX_IMPLEMENTATION\n#include "%s"\n' % header)
    gxx = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    subprocess.run(gxx + ["-c", str(tmp_path / "impl.cc"), "-o", str(tmp_path / "impl.o")], check=True)
    nm = subprocess.run(["nm", "-g", "--defined-only", str(tmp_path / "impl.o")], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in nm, name


def test_code_object_holds_the_sort64_kernels():
    """expected_kernels() lists every 64-bit kernel (the split in both forms), and the gfx950 code object embedded in the
    single header holds each of them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import generate_single_header as gen
    finally:
        sys.path.pop(0)
    names = gen.expected_kernels()
    for kernel in KERNELS:
        assert sum(kernel in n for n in names) == (2 if kernel == "split64_kernel" else 1), kernel
    text = open(_single_header()).read()
    array = text.split("static const unsigned char kVrdxCodeObject[] = {", 1)[1].split("};", 1)[0]
    blob = bytes(int(x) for x in array.replace("\n", "").split(","))
    kernels = {k.decode() for k in re.findall(rb"(_ZN4vrdx\w+)\.kd\x00", blob)}
    assert kernels == set(names), sorted(kernels ^ set(names))
    for kernel in KERNELS:
        assert any(kernel in k for k in kernels), kernel


def test_sort64_storage_carving_fits_every_count(tmp_path):
    """vrdx_layout.h MakeSort64Layout, for every count from 1 to 2^21, sampled counts up to 2^30 - 4 and every 16-byte
    alignment of the storage within a 128-byte line: the 32-bit key+value storage sits at offset 0 with exactly the size
    of the reference's formula (what vrdxGetSorterKeyValueStorageRequirements returns), the word arrays follow it without
    overlap on 128-byte lines of the absolute address, and all of it lies inside the reported sizes, which do not depend
    on the address."""
    src = tmp_path / "fit64.cc"
    src.write_text(
        '#include <cstdio>\n#include "vrdx_layout.h"\n'
        "int main() {\n"
        "  unsigned long bad = 0, seen = 0;\n"
        "  auto check = [&](uint32_t n) {\n"
        "    const uint64_t inout = vrdx::InoutSize(n, 16);\n"
        "    const uint64_t inner = 16 + vrdx::HistogramSize(n, 16) + vrdx::Align((uint32_t)inout, 16) + inout;\n"
        "    const vrdx::Sort64Layout at0 = vrdx::MakeSort64Layout(n, 16, 0);\n"
        "    for (uint64_t a = 0; a < 128; a += 16) {\n"
        "      const vrdx::Sort64Layout s = vrdx::MakeSort64Layout(n, 16, a);\n"
        "      ++seen;\n"
        "      const uint64_t words = 4ull * n, longs = 8ull * n;\n"
        "      bool ok = s.innerSize == inner && s.innerSize == vrdx::MakeLayout(n, 16, 0).keyValueSize;\n"
        "      ok = ok && s.keysOnlySize == at0.keysOnlySize && s.keyValueSize == at0.keyValueSize;\n"
        "      ok = ok && s.loOffset >= s.innerSize && s.otherOffset >= s.loOffset + words && s.keysTempOffset >= s.otherOffset + words;\n"
        "      ok = ok && (a + s.loOffset) % 128 == 0 && (a + s.otherOffset) % 128 == 0 && (a + s.keysTempOffset) % 128 == 0;\n"
        "      ok = ok && s.otherOffset + words <= s.keysOnlySize && s.keysTempOffset + longs <= s.keyValueSize;\n"
        "      ok = ok && s.keysOnlySize <= s.keyValueSize && s.keysOnlySize <= inner + 112 + 2 * (words + 124) &&\n"
        "           s.keyValueSize <= inner + 112 + 2 * (words + 124) + longs + 120;\n"
        "      if (!ok) { if (bad++ < 5) std::printf(\"n=%u a=%u\\n\", n, (unsigned)a); }\n"
        "    }\n"
        "  };\n"
        "  for (uint32_t n = 1; n <= (1u << 21); ++n) check(n);\n"
        "  for (uint64_t n = (1u << 21); n < 0x3FFFFFFCu; n += 65521) check((uint32_t)n);\n"
        "  check(0x3FFFFFFCu);\n"
        '  std::printf("%lu layouts, %lu failures\\n", seen, bad);\n'
        "  return bad != 0;\n}\n")
    exe = tmp_path / "fit64"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc"), str(src), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, r.stdout


def test_sort64_rejects_bad_arguments_on_the_host():
    """Wrong dtypes, shapes, strides, CPU tensors and mismatched values are refused before anything is recorded (no sorter
    call is reached, so no GPU is needed to see it)."""
    import torch
    from vulkan_radix_sort_amd.sort64 import sort64
    keys = torch.zeros(16, dtype=torch.int64)
    with pytest.raises(TypeError):
        sort64(None, keys.to(torch.int32))
    with pytest.raises(TypeError):
        sort64(None, keys.to(torch.float64))
    with pytest.raises(TypeError):
        sort64(None, keys.numpy())
    with pytest.raises(ValueError):
        sort64(None, keys.view(4, 4))
    with pytest.raises(ValueError):
        sort64(None, torch.zeros(32, dtype=torch.int64)[::2])
    with pytest.raises(ValueError):  # not on a GPU
        sort64(None, keys)
    if torch.cuda.is_available():
        dk = keys.cuda()
        values = torch.zeros(16, dtype=torch.int32, device="cuda")
        with pytest.raises(TypeError):
            sort64(None, dk, values=values.to(torch.int64))
        with pytest.raises(TypeError):
            sort64(None, dk, values=values.to(torch.float32))
        with pytest.raises(ValueError):
            sort64(None, dk, values=values[:8])
        with pytest.raises(ValueError):
            sort64(None, dk, values=values.view(4, 4))
        with pytest.raises(ValueError):
            sort64(None, dk, values=torch.zeros(32, dtype=torch.int32, device="cuda")[::2])
        with pytest.raises(ValueError):  # values on the CPU
            sort64(None, dk, values=values.cpu())
        with pytest.raises(TypeError):
            sort64(None, dk, storage=torch.zeros(64, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError):  # storage on the CPU
            sort64(None, dk, storage=torch.zeros(64, dtype=torch.uint8))
