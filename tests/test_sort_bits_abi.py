"""CPU-only checks of the bit-range sorts (vrdxHipCmdSortBits[KeyValue][Indirect], vrdxHipDescribeSortBitsPlan): the header
declares the five functions with the range right behind the keys (and values), the library exports them, the ctypes
signatures take the arguments in the documented order, and vulkan_radix_sort_amd.sort_bits refuses bad arguments on the
host before any library call (one test marked gpu: tensors on the wrong device, which needs one on the right one)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
NAMES = ("vrdxHipCmdSortBits", "vrdxHipCmdSortBitsKeyValue", "vrdxHipCmdSortBitsIndirect", "vrdxHipCmdSortBitsKeyValueIndirect",
         "vrdxHipDescribeSortBitsPlan")
METHODS = ("cmd_sort_bits", "cmd_sort_bits_key_value", "cmd_sort_bits_indirect", "cmd_sort_bits_key_value_indirect",
           "describe_sort_bits_plan")


def _declarations():
    """name -> parameter names, in order, of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(vrdx[A-Z]\w+)\s*\(([^)]*)\)\s*;", text):
        out[name] = [p.split()[-1].lstrip("*") for p in params.split(",") if p.strip() and p.strip() != "void"]
    return out


def test_header_library_and_python_agree_on_the_five_entry_points():
    import vulkan_radix_sort_amd as vrdx
    declared = _declarations()
    lib = vrdx.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in vrdx.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None, name
    for method in METHODS:
        assert callable(getattr(vrdx.Sorter, method)), method
    assert callable(vrdx.sort_bits) and "sort_bits" in vrdx.__all__


def test_the_range_sits_right_behind_the_keys_and_values():
    """every range call is the matching whole-key call with beginBit, endBit inserted behind the last array argument"""
    declared = _declarations()
    for whole, ranged in (("vrdxCmdSort", "vrdxHipCmdSortBits"), ("vrdxCmdSortKeyValue", "vrdxHipCmdSortBitsKeyValue"),
                          ("vrdxCmdSortIndirect", "vrdxHipCmdSortBitsIndirect"),
                          ("vrdxCmdSortKeyValueIndirect", "vrdxHipCmdSortBitsKeyValueIndirect")):
        want = list(declared[whole])
        at = want.index("storageBuffer")
        want[at:at] = ["beginBit", "endBit"]
        assert declared[ranged] == want, ranged
        assert want[at - 1] in ("keysOffset", "valuesOffset")
    assert declared["vrdxHipDescribeSortBitsPlan"] == ["sorter", "elementCount", "keyValue", "beginBit", "endBit", "info"]


def test_ctypes_signatures_take_the_documented_order():
    import vulkan_radix_sort_amd as vrdx
    lib = vrdx.load_library()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    tail = [u32, u32, vp, u64, vp, u32]   # beginBit, endBit, storage, storageOffset, queryPool, query
    assert list(lib.vrdxHipCmdSortBits.argtypes) == [vp, vp, u32, vp, u64] + tail
    assert list(lib.vrdxHipCmdSortBitsKeyValue.argtypes) == [vp, vp, u32, vp, u64, vp, u64] + tail
    assert list(lib.vrdxHipCmdSortBitsIndirect.argtypes) == [vp, vp, u32, vp, u64, vp, u64] + tail
    assert list(lib.vrdxHipCmdSortBitsKeyValueIndirect.argtypes) == [vp, vp, u32, vp, u64, vp, u64, vp, u64] + tail
    assert list(lib.vrdxHipDescribeSortBitsPlan.argtypes) == [vp, u32, ctypes.c_int, u32, u32,
                                                              ctypes.POINTER(vrdx.VrdxHipPlanInfo)]
    for name in NAMES:
        assert getattr(lib, name).restype is None, name


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, uint32_t, uint32_t, VkBuffer, VkDeviceSize,\n"
        "               VkQueryPool, uint32_t) = vrdxHipCmdSortBits;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, uint32_t, uint32_t,\n"
        "                VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSortBitsKeyValue;\n"
        "  void (*keysIndirect)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, uint32_t,\n"
        "                       uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSortBitsIndirect;\n"
        "  void (*pairsIndirect)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "                        VkDeviceSize, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) =\n"
        "      vrdxHipCmdSortBitsKeyValueIndirect;\n"
        "  void (*describe)(VrdxSorter, uint32_t, int, uint32_t, uint32_t, VrdxHipPlanInfo*) = vrdxHipDescribeSortBitsPlan;\n"
        "  return (keys != 0 && pairs != 0 && keysIndirect != 0 && pairsIndirect != 0 && describe != 0) ? 0 : 1;\n}\n")
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "s.o")],
                   check=True)


class _NoLibraryCall:
    """stands in for the sorter: any use of it is a library call the host checks should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"sort_bits reached the sorter ({name}) with arguments it should have refused")


def test_sort_bits_rejects_bad_arguments_before_any_library_call():
    """Types, dtypes, shapes, the range and the lengths are checked before where the tensors live, so CPU tensors show every
    one of them without a GPU; the last check standing is the device."""
    import torch
    from vulkan_radix_sort_amd import sort_bits
    sorter = _NoLibraryCall()
    keys = torch.zeros(16, dtype=torch.int32)
    for bad, error in ((torch.zeros(16, dtype=torch.int64), TypeError), (torch.zeros(16, dtype=torch.float32), TypeError),
                       ([1, 2, 3], TypeError), (torch.zeros((4, 4), dtype=torch.int32), ValueError)):   # dtype, type, shape
        with pytest.raises(error):
            sort_bits(sorter, bad, 0, 8)
    for begin, end in ((9, 8), (0, 33), (-1, 8), (33, 33)):   # begin > end, end > 32
        with pytest.raises(ValueError, match="bit range"):
            sort_bits(sorter, keys, begin, end)
    with pytest.raises(TypeError):
        sort_bits(sorter, keys, 0.0, 8)
    with pytest.raises(TypeError):
        sort_bits(sorter, keys, 0, True)
    with pytest.raises(TypeError):       # values: dtype, then length
        sort_bits(sorter, keys, 0, 8, values=torch.zeros(16, dtype=torch.int64))
    with pytest.raises(ValueError, match="values hold 15"):
        sort_bits(sorter, keys, 0, 8, values=torch.zeros(15, dtype=torch.int32))
    with pytest.raises(ValueError, match="at most 16384"):   # more than one workgroup takes, and not the whole key
        sort_bits(sorter, torch.zeros(16385, dtype=torch.int32), 3, 12)
    with pytest.raises(TypeError):       # count: type, dtype, one element
        sort_bits(sorter, keys, 0, 8, count=16)
    with pytest.raises(TypeError):
        sort_bits(sorter, keys, 0, 8, count=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="count must hold 1"):
        sort_bits(sorter, keys, 0, 8, count=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):       # storage
        sort_bits(sorter, keys, 0, 8, storage=torch.zeros(1 << 16, dtype=torch.int32))
    # everything else in order: CPU tensors are what is left to refuse
    with pytest.raises(ValueError, match="must live on a GPU"):
        sort_bits(sorter, keys, 0, 8, values=torch.zeros(16, dtype=torch.int32), count=torch.zeros(1, dtype=torch.int32))


@pytest.mark.gpu
def test_sort_bits_rejects_tensors_on_the_wrong_device():
    import torch
    from vulkan_radix_sort_amd import sort_bits
    sorter = _NoLibraryCall()
    dk = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="values must live on a GPU"):
        sort_bits(sorter, dk, 0, 8, values=torch.zeros(16, dtype=torch.int32))
    with pytest.raises(ValueError, match="count must live on a GPU"):
        sort_bits(sorter, dk, 0, 8, count=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="storage must live on a GPU"):
        sort_bits(sorter, dk, 0, 8, storage=torch.zeros(1 << 16, dtype=torch.uint8))
