"""CPU-only checks of the balanced segmented sort's interface (vrdxHipCmdBalancedSortSegmented[KeyValue],
vrdxHipDescribeBalancedSegmentedPlan, vrdxHipReadBalancedSplit): the header declares the two calls with the argument lists of
vrdxHipCmdSortSegmented[KeyValue], name for name and position for position; the library exports all four; the rows of
BALANCED_SEGMENTED_CALLS, the ctypes signatures and the Sorter methods follow the declarations; RECORDING_CALLS keeps its 24
rows; the two info structures are the header's; and vulkan_radix_sort_amd.sort_segments_balanced refuses what sort_segments
refuses, with the same words, before any library call."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")   # the twin's declarations
BALANCED_HEADER = os.path.join(ROOT, "include", "vk_radix_sort_balanced.h")
PAIRS = (("vrdxHipCmdSortSegmented", "vrdxHipCmdBalancedSortSegmented"),
         ("vrdxHipCmdSortSegmentedKeyValue", "vrdxHipCmdBalancedSortSegmentedKeyValue"))
NAMES = tuple(balanced for _, balanced in PAIRS) + ("vrdxHipDescribeBalancedSegmentedPlan", "vrdxHipReadBalancedSplit")
METHODS = ("cmd_balanced_sort_segmented", "cmd_balanced_sort_segmented_key_value", "describe_balanced_segmented_plan",
           "read_balanced_split")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read() + open(BALANCED_HEADER).read(), flags=re.S)


def _declarations():
    """name -> [(type, parameter name)], in order, of every function the header declares"""
    out = {}
    for name, params in re.findall(r"\b(vrdx[A-Z]\w+)\s*\(([^)]*)\)\s*;", _header()):
        out[name] = [(" ".join(p.split()[:-1]) + "*" * p.split()[-1].count("*"), p.split()[-1].lstrip("*"))
                     for p in params.split(",") if p.strip() and p.strip() != "void"]
    return out


def test_header_library_and_python_agree_on_the_four_entry_points():
    import vulkan_radix_sort_amd as vrdx
    declared = _declarations()
    lib = vrdx.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vrdx.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in declared and name in vrdx.BALANCED_EXPORTED_SYMBOLS and f" T {name}\n" in nm, name
        assert getattr(lib, name) is not None, name
    for method in METHODS:
        assert callable(getattr(vrdx.Sorter, method)), method
    for name in ("sort_segments_balanced", "BALANCED_SEGMENTED_CALLS", "BALANCED_FORM_NAMES", "VrdxHipBalancedSegmentedPlanInfo",
                 "VrdxHipBalancedSplitInfo"):
        assert name in vrdx.__all__ and hasattr(vrdx, name), name
    # a tuple of their own, for a header of their own: EXPORTED_SYMBOLS stays what include/vk_radix_sort.h declares
    assert vrdx.BALANCED_EXPORTED_SYMBOLS == NAMES and not set(NAMES) & set(vrdx.EXPORTED_SYMBOLS)
    assert set(re.findall(r"\b(vrdx[A-Z]\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(BALANCED_HEADER).read(), flags=re.S))) == set(NAMES)
    assert "BALANCED_EXPORTED_SYMBOLS" in vrdx.__all__
    assert len(vrdx.api.RECORDING_CALLS) == 24
    assert not set(NAMES) & {call.c_name for call in vrdx.api.RECORDING_CALLS}
    assert not any(re.fullmatch(r"vrdx(Hip)?CmdSort\w*", name) for name in NAMES)


def test_the_argument_lists_are_the_twin_s():
    declared = _declarations()
    for twin, balanced in PAIRS:
        assert declared[balanced] == declared[twin], balanced
    assert declared["vrdxHipDescribeBalancedSegmentedPlan"] == [
        ("VrdxSorter", "sorter"), ("uint32_t", "maxElementCount"), ("uint32_t", "segmentCount"), ("int", "keyValue"),
        ("VrdxHipBalancedSegmentedPlanInfo*", "info")]
    assert declared["vrdxHipReadBalancedSplit"] == [
        ("VkCommandBuffer", "commandBuffer"), ("VrdxSorter", "sorter"), ("VkBuffer", "storageBuffer"),
        ("VkDeviceSize", "storageOffset"), ("uint32_t", "maxElementCount"), ("VrdxHipBalancedSplitInfo*", "info")]


def test_the_table_of_calls_follows_the_declarations():
    import vulkan_radix_sort_amd as vrdx
    from vulkan_radix_sort_amd import api
    declared = _declarations()
    lib = vrdx.load_library()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    ctype_of = {"VkCommandBuffer": vp, "VrdxSorter": vp, "VkBuffer": vp, "VkQueryPool": vp, "uint32_t": u32, "VkDeviceSize": u64}
    assert [call.c_name for call in api.BALANCED_SEGMENTED_CALLS] == [balanced for _, balanced in PAIRS]
    assert [call.method for call in api.BALANCED_SEGMENTED_CALLS] == list(METHODS[:2])
    by_name = {call.c_name: call for call in api.RECORDING_CALLS}
    for (twin, balanced), call in zip(PAIRS, api.BALANCED_SEGMENTED_CALLS):
        assert call.facts == by_name[twin].facts and call.parameters == by_name[twin].parameters, balanced
        assert list(getattr(lib, balanced).argtypes) == [ctype_of[t] for t, _ in declared[balanced]] == call.argtypes, balanced
        assert getattr(lib, balanced).restype is None
        assert call.doc and "\n" not in call.doc
    assert list(lib.vrdxHipDescribeBalancedSegmentedPlan.argtypes) == [
        vp, u32, u32, ctypes.c_int, ctypes.POINTER(vrdx.VrdxHipBalancedSegmentedPlanInfo)]
    assert lib.vrdxHipDescribeBalancedSegmentedPlan.restype is None
    assert list(lib.vrdxHipReadBalancedSplit.argtypes) == [vp, vp, vp, u64, u32, ctypes.POINTER(vrdx.VrdxHipBalancedSplitInfo)]
    assert lib.vrdxHipReadBalancedSplit.restype is ctypes.c_int32


def test_the_methods_forward_in_the_header_s_order():
    from vulkan_radix_sort_amd import api

    class Library:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *args: self.calls.append((name,) + args)

    for call in api.BALANCED_SEGMENTED_CALLS:
        sorter = api.Sorter.__new__(api.Sorter)
        sorter._lib, sorter.handle = Library(), 99
        count = len(call.parameters)
        sentinels = [1000 + 7 * i for i in range(count)]
        getattr(sorter, call.method)(*sentinels)
        assert sorter._lib.calls == [(call.c_name, sentinels[0], 99) + tuple(sentinels[1:])]
        sorter.handle = None   # (so that __del__ has nothing to destroy)


def test_the_info_structures_and_their_constants_are_the_header_s():
    import vulkan_radix_sort_amd as vrdx
    text = _header()
    for name, fields in (("VrdxHipBalancedSegmentedPlanInfo", ["form", "launches", "spreadFrom", "spreadShares", "spreadCap",
                                                                "pieceCap", "minPieceKeys"]),
                         ("VrdxHipBalancedSplitInfo", ["listedSegments", "spreadSegments", "pieces", "pieceKeys"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        struct = getattr(vrdx, name)
        assert re.findall(r"uint32_t\s+(\w+);", body) == fields == [field for field, _ in struct._fields_]
        assert all(ctype is ctypes.c_uint32 for _, ctype in struct._fields_) and ctypes.sizeof(struct) == 4 * len(fields)
    defines = dict(re.findall(r"#define VRDX_HIP_BALANCED_(\w+) (\d+)u", text))
    assert {name.lower(): int(defines[name]) for name in ("NONE", "TWIN", "BALANCED")} == {
        name: value for value, name in vrdx.BALANCED_FORM_NAMES.items()}
    assert (int(defines["SPREAD_FROM"]), int(defines["SPREAD_SHARES"])) == (65536, 3)
    layout = open(os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc", "vrdx_layout.h")).read()
    assert "constexpr uint32_t kSegSpreadFrom = 65536u;" in layout and "constexpr uint32_t kSegSpreadShares = 3u;" in layout


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort_balanced.h"\n'
        "int main(void) {\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "               VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdBalancedSortSegmented;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "                VkDeviceSize, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdBalancedSortSegmentedKeyValue;\n"
        "  void (*describe)(VrdxSorter, uint32_t, uint32_t, int, VrdxHipBalancedSegmentedPlanInfo*) =\n"
        "      vrdxHipDescribeBalancedSegmentedPlan;\n"
        "  VkResult (*read)(VkCommandBuffer, VrdxSorter, VkBuffer, VkDeviceSize, uint32_t, VrdxHipBalancedSplitInfo*) =\n"
        "      vrdxHipReadBalancedSplit;\n"
        "  VrdxHipBalancedSegmentedPlanInfo info = {VRDX_HIP_BALANCED_NONE, 0, 0, 0, 0, 0, 0};\n"
        "  VrdxHipBalancedSplitInfo split = {0, 0, 0, 0};\n"
        "  (void)info;\n  (void)split;\n"
        "  return (keys != 0 && pairs != 0 && describe != 0 && read != 0 && VRDX_HIP_BALANCED_BALANCED == 2u &&\n"
        "          VRDX_HIP_BALANCED_SPREAD_FROM == 65536u && VRDX_HIP_BALANCED_SPREAD_SHARES == 3u) ? 0 : 1;\n}\n")
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "s.o")],
                   check=True)


class _NoLibraryCall:
    """stands in for the sorter: any use of it is a library call the host checks should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"sort_segments_balanced reached the sorter ({name}) with arguments it should have refused")


def test_the_front_end_refuses_what_sort_segments_refuses_with_the_same_words():
    """on CPU tensors every check of sort_segments speaks, in its order, and the last one standing is the device"""
    import torch
    from vulkan_radix_sort_amd import sort_segments, sort_segments_balanced
    sorter = _NoLibraryCall()
    keys = torch.zeros(16, dtype=torch.int32)
    offsets = torch.tensor([0, 16], dtype=torch.int32)
    tried = ((torch.zeros(16, dtype=torch.int64), offsets, None, None), ([1, 2, 3], offsets, None, None),
             (torch.zeros((4, 4), dtype=torch.int32), offsets, None, None), (keys, offsets, None, None),
             (keys, torch.zeros(2, dtype=torch.int64), None, None), (keys, [0, 16], None, None),
             (keys, offsets, torch.zeros(15, dtype=torch.int32), None), (keys, offsets, torch.zeros(16, dtype=torch.int64), None),
             (keys, offsets, None, torch.zeros(64, dtype=torch.int32)))
    for k, o, v, s in tried:
        outcome = []
        for front_end in (sort_segments, sort_segments_balanced):
            with pytest.raises((TypeError, ValueError)) as caught:
                front_end(sorter, k, o, values=v, storage=s)
            outcome.append((caught.type, str(caught.value)))
        assert outcome[0] == outcome[1]
    with pytest.raises(ValueError, match="must live on a GPU"):
        sort_segments_balanced(sorter, keys, offsets)
