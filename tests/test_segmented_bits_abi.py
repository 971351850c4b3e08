"""CPU-only checks of the segmented sort by a bit range (vrdxHipCmdSortSegmentedBits[KeyValue]): the header declares both
functions with the range in front of storageBuffer, the library exports them, the ctypes signatures take the arguments in the
documented order, and vulkan_radix_sort_amd.sort_segments_bits refuses bad arguments on the host before any library call."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
NAMES = ("vrdxHipCmdSortSegmentedBits", "vrdxHipCmdSortSegmentedBitsKeyValue")
METHODS = ("cmd_sort_segmented_bits", "cmd_sort_segmented_bits_key_value")


def _declarations():
    """name -> parameter names, in order, of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(vrdx[A-Z]\w+)\s*\(([^)]*)\)\s*;", text):
        out[name] = [p.split()[-1].lstrip("*") for p in params.split(",") if p.strip() and p.strip() != "void"]
    return out


def test_header_library_and_python_agree_on_both_entry_points():
    import vulkan_radix_sort_amd as vrdx
    declared = _declarations()
    lib = vrdx.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in vrdx.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None, name
    nm = subprocess.run(["nm", "-D", "--defined-only", vrdx.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in nm, name
    for method in METHODS:
        assert callable(getattr(vrdx.Sorter, method)), method


def test_sort_segments_bits_is_importable_from_the_package():
    import vulkan_radix_sort_amd as vrdx
    from vulkan_radix_sort_amd import sort_segments_bits
    from vulkan_radix_sort_amd.segmented_bits import sort_segments_bits as from_module
    assert sort_segments_bits is from_module and callable(vrdx.sort_segments_bits) and "sort_segments_bits" in vrdx.__all__
    assert callable(vrdx.sort_segments) and callable(vrdx.sort_bits)   # (both keep their place)


def test_the_range_sits_in_front_of_the_storage():
    """each call is the matching whole-key segmented call with beginBit, endBit inserted in front of storageBuffer, the
    position they have in vrdxHipCmdSortBits*"""
    declared = _declarations()
    for whole, ranged in (("vrdxHipCmdSortSegmented", "vrdxHipCmdSortSegmentedBits"),
                          ("vrdxHipCmdSortSegmentedKeyValue", "vrdxHipCmdSortSegmentedBitsKeyValue")):
        want = list(declared[whole])
        at = want.index("storageBuffer")
        want[at:at] = ["beginBit", "endBit"]
        assert declared[ranged] == want, ranged
        assert want[at - 1] in ("keysOffset", "valuesOffset")


def test_ctypes_signatures_take_the_documented_order():
    import vulkan_radix_sort_amd as vrdx
    lib = vrdx.load_library()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    head = [vp, vp, u32, u32, vp, u64, vp, u64]   # commandBuffer, sorter, maxElementCount, segmentCount, offsets, keys
    tail = [u32, u32, vp, u64, vp, u32]           # beginBit, endBit, storage, storageOffset, queryPool, query
    assert list(lib.vrdxHipCmdSortSegmentedBits.argtypes) == head + tail
    assert list(lib.vrdxHipCmdSortSegmentedBitsKeyValue.argtypes) == head + [vp, u64] + tail
    for name in NAMES:
        assert getattr(lib, name).restype is None, name
    # the whole-key calls are what they were
    assert list(lib.vrdxHipCmdSortSegmented.argtypes) == head + tail[2:]
    assert list(lib.vrdxHipCmdSortSegmentedKeyValue.argtypes) == head + [vp, u64] + tail[2:]


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, uint32_t,\n"
        "               uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSortSegmentedBits;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "                VkDeviceSize, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) =\n"
        "      vrdxHipCmdSortSegmentedBitsKeyValue;\n"
        "  return (keys != 0 && pairs != 0) ? 0 : 1;\n}\n")
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "s.o")],
                   check=True)


class _NoLibraryCall:
    """stands in for the sorter: any use of it is a library call the host checks should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"sort_segments_bits reached the sorter ({name}) with arguments it should have refused")


def test_sort_segments_bits_rejects_bad_arguments_before_any_library_call():
    import torch
    from vulkan_radix_sort_amd import sort_segments_bits
    sorter = _NoLibraryCall()
    keys = torch.zeros(16, dtype=torch.int32)
    offsets = torch.tensor([0, 16], dtype=torch.int32)
    for begin, end in ((9, 3), (0, 33), (33, 40), (-1, 8)):   # the range first: invalid whatever the tensors are
        with pytest.raises(ValueError, match="bit range"):
            sort_segments_bits(sorter, keys, offsets, begin, end)
    with pytest.raises(TypeError):
        sort_segments_bits(sorter, keys, offsets, 0.0, 8)
    with pytest.raises(TypeError):
        sort_segments_bits(sorter, keys, offsets, 0, True)
    for bad, error in ((torch.zeros(16, dtype=torch.int64), TypeError), (torch.zeros(16, dtype=torch.float32), TypeError),
                       ([1, 2, 3], TypeError), (torch.zeros((4, 4), dtype=torch.int32), ValueError)):   # dtype, type, shape
        with pytest.raises(error):
            sort_segments_bits(sorter, bad, offsets, 0, 8)
    with pytest.raises(TypeError):       # offsets: dtype; at least one entry
        sort_segments_bits(sorter, keys, torch.tensor([0, 16], dtype=torch.int64), 3, 12)
    with pytest.raises(ValueError, match="offsets must hold"):
        sort_segments_bits(sorter, keys, torch.zeros(0, dtype=torch.int32), 3, 12)
    with pytest.raises(TypeError):       # values: dtype, then length
        sort_segments_bits(sorter, keys, offsets, 3, 12, values=torch.zeros(16, dtype=torch.int64))
    with pytest.raises(ValueError, match="values hold 15"):
        sort_segments_bits(sorter, keys, offsets, 3, 12, values=torch.zeros(15, dtype=torch.int32))
    # everything else in order: CPU tensors are what is left to refuse
    with pytest.raises(ValueError, match="keys must live on a GPU"):
        sort_segments_bits(sorter, keys, offsets, 3, 12, values=torch.zeros(16, dtype=torch.int32))


@pytest.mark.gpu
def test_sort_segments_bits_rejects_tensors_on_the_wrong_device():
    import torch
    from vulkan_radix_sort_amd import sort_segments_bits
    sorter = _NoLibraryCall()
    dk = torch.zeros(16, dtype=torch.int32, device="cuda")
    do = torch.tensor([0, 16], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="offsets must live on a GPU"):
        sort_segments_bits(sorter, dk, torch.tensor([0, 16], dtype=torch.int32), 3, 12)
    with pytest.raises(ValueError, match="values must live on a GPU"):
        sort_segments_bits(sorter, dk, do, 3, 12, values=torch.zeros(16, dtype=torch.int32))
    with pytest.raises(ValueError, match="storage must live on a GPU"):
        sort_segments_bits(sorter, dk, do, 3, 12, storage=torch.zeros(1 << 16, dtype=torch.uint8))
