"""CPU-only checks of the 64-bit sorts by a device-side count (vrdxHipCmdSort64[KeyValue]Indirect): the C-ABI surface, the
declarations in C and C++ with the exact function-pointer types, the single header's implementation object, and the
host-side checks of the `count` argument of vulkan_radix_sort_amd.sort64."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
SINGLE_HEADER = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
NAMES = ("vrdxHipCmdSort64Indirect", "vrdxHipCmdSort64KeyValueIndirect")
METHODS = ("cmd_sort64_indirect", "cmd_sort64_key_value_indirect")


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


def test_header_library_and_python_agree_on_the_indirect_entry_points():
    import vulkan_radix_sort_amd as vrdx
    declared = _declared()
    lib = vrdx.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in vrdx.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None, name
    for method in METHODS:
        assert callable(getattr(vrdx.Sorter, method)), method
    # the binding passes what the C declaration takes: two handles, the bound, (buffer, offset) pairs, pool, query
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for name, pairs in ((NAMES[0], 3), (NAMES[1], 4)):
        assert list(getattr(lib, name).argtypes) == [vp, vp, u32] + [vp, u64] * pairs + [vp, u32], name
    # the header no longer files the indirect forms under what is left to the caller
    assert "no vrdxHipCmdSort64Indirect" not in open(HEADER).read()


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_indirect_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "               VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSort64Indirect;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "                VkDeviceSize, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSort64KeyValueIndirect;\n"
        "  return (keys != 0 && pairs != 0) ? 0 : 1;\n}\n")
    obj = tmp_path / "s.o"
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                   check=True)


def test_single_header_implementation_exports_the_indirect_entry_points(tmp_path):
    header = _single_header()
    (tmp_path / "impl.cc").write_text('#define VRDX_IMPLEMENTATION\n#include "%s"\n' % header)
    gxx = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    subprocess.run(gxx + ["-c", str(tmp_path / "impl.cc"), "-o", str(tmp_path / "impl.o")], check=True)
    nm = subprocess.run(["nm", "-g", "--defined-only", str(tmp_path / "impl.o")], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in nm, name


def test_sort64_rejects_a_bad_count_on_the_host():
    """What can be told without a GPU: a count that is no tensor or holds no 4-byte integer is a TypeError, one with more
    than one element or on the CPU a ValueError -- raised before the sorter is touched (it is None here).  The keys are
    checked first, so these need keys on a GPU; the cases with CPU keys only show that the new argument exists."""
    import torch
    from vulkan_radix_sort_amd.sort64 import sort64
    keys = torch.zeros(16, dtype=torch.int64)
    with pytest.raises(ValueError):  # keys not on a GPU: refused as before, whatever the count
        sort64(None, keys, count=torch.zeros(1, dtype=torch.int32))
    if torch.cuda.is_available():
        dk = keys.cuda()
        with pytest.raises(TypeError):
            sort64(None, dk, count=16)
        with pytest.raises(TypeError):
            sort64(None, dk, count=torch.zeros(1, dtype=torch.int64, device="cuda"))
        with pytest.raises(TypeError):
            sort64(None, dk, count=torch.zeros(1, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            sort64(None, dk, count=torch.zeros(2, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError):
            sort64(None, dk, count=torch.zeros(0, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError):
            sort64(None, dk, count=torch.zeros(1, dtype=torch.int32))
