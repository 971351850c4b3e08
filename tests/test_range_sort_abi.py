"""CPU-only checks of the range sorts at every size (vrdxHipCmdRangeSort[KeyValue][Indirect], vrdxHipDescribeRangeSortPlan):
the header declares the four calls with the argument lists of vrdxHipCmdSortBits*, name for name and position for position,
and the describe call; the library exports them; RANGE_SORT_CALLS, the ctypes signatures and the Sorter methods follow the
declarations; RECORDING_CALLS keeps its 24 rows; and vulkan_radix_sort_amd.sort_range refuses bad arguments on the host before
any library call, in the order of sort_bits, without its bound on the number of keys (one test marked gpu: tensors on the
wrong device, which needs one on the right one)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
PAIRS = (("vrdxHipCmdSortBits", "vrdxHipCmdRangeSort"), ("vrdxHipCmdSortBitsKeyValue", "vrdxHipCmdRangeSortKeyValue"),
         ("vrdxHipCmdSortBitsIndirect", "vrdxHipCmdRangeSortIndirect"),
         ("vrdxHipCmdSortBitsKeyValueIndirect", "vrdxHipCmdRangeSortKeyValueIndirect"))
NAMES = tuple(ranged for _, ranged in PAIRS) + ("vrdxHipDescribeRangeSortPlan",)
METHODS = ("cmd_range_sort", "cmd_range_sort_key_value", "cmd_range_sort_indirect", "cmd_range_sort_key_value_indirect",
           "describe_range_sort_plan")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declarations():
    """name -> [(type, parameter name)], in order, of every function the header declares"""
    out = {}
    for name, params in re.findall(r"\b(vrdx[A-Z]\w+)\s*\(([^)]*)\)\s*;", _header()):
        out[name] = [(" ".join(p.split()[:-1]) + "*" * p.split()[-1].count("*"), p.split()[-1].lstrip("*"))
                     for p in params.split(",") if p.strip() and p.strip() != "void"]
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
    assert callable(vrdx.sort_range) and "sort_range" in vrdx.__all__
    # added as one group, in this order, behind the rows of RECORDING_CALLS; the names every earlier pull request exported keep
    # their order around it and the later groups their distance from the end (which their own tests pin)
    symbols = vrdx.EXPORTED_SYMBOLS
    at = symbols.index(NAMES[0])
    assert symbols[at:at + 5] == NAMES and symbols[at - 1] == vrdx.api.RECORDING_CALLS[-1].c_name
    assert symbols[at + 5] == vrdx.api.WIDE_VALUE_SEGMENTED_CALLS[0].c_name
    assert len(set(symbols)) == len(symbols) == 59
    assert len(vrdx.api.RECORDING_CALLS) == 24
    assert not set(NAMES) & {call.c_name for call in vrdx.api.RECORDING_CALLS}


def test_the_argument_lists_are_those_of_the_sort_bits_calls():
    declared = _declarations()
    for bits, ranged in PAIRS:
        assert declared[ranged] == declared[bits], ranged
    assert declared["vrdxHipDescribeRangeSortPlan"] == [("VrdxSorter", "sorter"), ("uint32_t", "elementCount"), ("int", "keyValue"),
                                                        ("uint32_t", "beginBit"), ("uint32_t", "endBit"),
                                                        ("VrdxHipRangeSortPlanInfo*", "info")]


def test_the_table_of_calls_follows_the_declarations():
    import vulkan_radix_sort_amd as vrdx
    from vulkan_radix_sort_amd import api
    declared = _declarations()
    lib = vrdx.load_library()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    ctype_of = {"VkCommandBuffer": vp, "VrdxSorter": vp, "VkBuffer": vp, "VkQueryPool": vp, "uint32_t": u32, "VkDeviceSize": u64}
    assert [call.c_name for call in api.RANGE_SORT_CALLS] == [ranged for _, ranged in PAIRS]
    assert [call.method for call in api.RANGE_SORT_CALLS] == list(METHODS[:4])
    by_name = {call.c_name: call for call in api.RECORDING_CALLS}
    for (bits, ranged), call in zip(PAIRS, api.RANGE_SORT_CALLS):
        assert call.facts == by_name[bits].facts and call.parameters == by_name[bits].parameters, ranged
        assert list(getattr(lib, ranged).argtypes) == [ctype_of[t] for t, _ in declared[ranged]] == call.argtypes, ranged
        assert getattr(lib, ranged).restype is None
        snake = [re.sub(r"(?<!^)([A-Z])", r"_\1", name).lower().replace("_buffer", "") for _, name in declared[ranged]]
        snake = ["command_buffer" if s == "command" else s for s in snake]
        assert [name for name, _ in call.parameters] == [s for s in snake if s != "sorter"], ranged
    assert list(lib.vrdxHipDescribeRangeSortPlan.argtypes) == [vp, u32, ctypes.c_int, u32, u32,
                                                               ctypes.POINTER(vrdx.VrdxHipRangeSortPlanInfo)]
    assert lib.vrdxHipDescribeRangeSortPlan.restype is None


def test_the_info_structure_and_its_constants_are_the_header_s():
    import vulkan_radix_sort_amd as vrdx
    text = _header()
    body = re.search(r"typedef struct VrdxHipRangeSortPlanInfo \{(.*?)\} VrdxHipRangeSortPlanInfo;", text, flags=re.S).group(1)
    fields = re.findall(r"uint32_t\s+(\w+);", body)
    assert fields == [name for name, _ in vrdx.VrdxHipRangeSortPlanInfo._fields_]
    assert fields == ["form", "chunks", "keysPerChunk", "digits", "launches", "bytesPerElementPerPass", "bytesPerElementCopyBack"]
    assert all(ctype is ctypes.c_uint32 for _, ctype in vrdx.VrdxHipRangeSortPlanInfo._fields_)
    forms = {name.lower().replace("_", "-"): int(value)
             for name, value in re.findall(r"#define VRDX_HIP_RANGE_SORT_(\w+) (\d+)u", text)}
    assert forms == {name: value for value, name in vrdx.RANGE_SORT_FORM_NAMES.items()}


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, uint32_t, uint32_t, VkBuffer, VkDeviceSize,\n"
        "               VkQueryPool, uint32_t) = vrdxHipCmdRangeSort;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, uint32_t, uint32_t,\n"
        "                VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdRangeSortKeyValue;\n"
        "  void (*keysIndirect)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, uint32_t,\n"
        "                       uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdRangeSortIndirect;\n"
        "  void (*pairsIndirect)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "                        VkDeviceSize, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) =\n"
        "      vrdxHipCmdRangeSortKeyValueIndirect;\n"
        "  void (*describe)(VrdxSorter, uint32_t, int, uint32_t, uint32_t, VrdxHipRangeSortPlanInfo*) = vrdxHipDescribeRangeSortPlan;\n"
        "  VrdxHipRangeSortPlanInfo info = {VRDX_HIP_RANGE_SORT_NONE, 0, 0, 0, 0, 0, 0};\n"
        "  (void)info;\n"
        "  return (keys != 0 && pairs != 0 && keysIndirect != 0 && pairsIndirect != 0 && describe != 0 &&\n"
        "          VRDX_HIP_RANGE_SORT_CHUNKED == 3u) ? 0 : 1;\n}\n")
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "s.o")],
                   check=True)


class _NoLibraryCall:
    """stands in for the sorter: any use of it is a library call the host checks should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"sort_range reached the sorter ({name}) with arguments it should have refused")


def test_sort_range_rejects_bad_arguments_before_any_library_call():
    """Types, dtypes, shapes, the range and the lengths are checked before where the tensors live, so CPU tensors show every
    one of them without a GPU; the last check standing is the device."""
    import torch
    from vulkan_radix_sort_amd import sort_range
    sorter = _NoLibraryCall()
    keys = torch.zeros(16, dtype=torch.int32)
    for bad, error in ((torch.zeros(16, dtype=torch.int64), TypeError), (torch.zeros(16, dtype=torch.float32), TypeError),
                       ([1, 2, 3], TypeError), (torch.zeros((4, 4), dtype=torch.int32), ValueError)):   # dtype, type, shape
        with pytest.raises(error):
            sort_range(sorter, bad, 0, 8)
    for begin, end in ((9, 8), (0, 33), (-1, 8), (33, 33)):   # begin > end, end > 32
        with pytest.raises(ValueError, match="bit range"):
            sort_range(sorter, keys, begin, end)
    with pytest.raises(TypeError):
        sort_range(sorter, keys, 0.0, 8)
    with pytest.raises(TypeError):
        sort_range(sorter, keys, 0, True)
    with pytest.raises(TypeError):       # values: dtype, then length
        sort_range(sorter, keys, 0, 8, values=torch.zeros(16, dtype=torch.int64))
    with pytest.raises(ValueError, match="values hold 15"):
        sort_range(sorter, keys, 0, 8, values=torch.zeros(15, dtype=torch.int32))
    with pytest.raises(TypeError):       # count: type, dtype, one element
        sort_range(sorter, keys, 0, 8, count=16)
    with pytest.raises(TypeError):
        sort_range(sorter, keys, 0, 8, count=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="count must hold 1"):
        sort_range(sorter, keys, 0, 8, count=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):       # storage
        sort_range(sorter, keys, 0, 8, storage=torch.zeros(1 << 16, dtype=torch.int32))
    # everything else in order: CPU tensors are what is left to refuse
    with pytest.raises(ValueError, match="must live on a GPU"):
        sort_range(sorter, keys, 0, 8, values=torch.zeros(16, dtype=torch.int32), count=torch.zeros(1, dtype=torch.int32))
    # no bound on the number of keys of a partial range: 16385 keys get as far as the device check, where sort_bits refuses
    many = torch.zeros(16385, dtype=torch.int32)
    with pytest.raises(ValueError, match="keys must live on a GPU"):
        sort_range(sorter, many, 3, 12)
    from vulkan_radix_sort_amd import sort_bits
    with pytest.raises(ValueError, match="at most 16384"):
        sort_bits(sorter, many, 3, 12)


def test_the_order_of_the_checks_is_that_of_sort_bits():
    """one call with several things wrong: the refusal that wins is the same in both front ends, check by check"""
    import torch
    from vulkan_radix_sort_amd import sort_bits, sort_range
    sorter = _NoLibraryCall()
    keys = torch.zeros(16, dtype=torch.int32)
    wrong = {"keys": torch.zeros(16, dtype=torch.int64), "values": torch.zeros(15, dtype=torch.int32), "begin_bit": 9,
             "count": torch.zeros(2, dtype=torch.int32), "storage": torch.zeros(64, dtype=torch.int32)}
    right = {"keys": keys, "values": None, "begin_bit": 0, "count": None, "storage": None}
    order = ["keys", "values", "begin_bit", "count", "storage"]
    messages = []
    for first in range(len(order) + 1):   # everything from `first` on is wrong; then nothing is, and the device check is left
        given = {name: (wrong if i >= first else right)[name] for i, name in enumerate(order)}
        outcome = []
        for front_end in (sort_bits, sort_range):
            with pytest.raises((TypeError, ValueError)) as caught:
                front_end(sorter, given["keys"], given["begin_bit"], 8, values=given["values"], count=given["count"],
                          storage=given["storage"])
            outcome.append((caught.type, str(caught.value)))
        assert outcome[0] == outcome[1], order[first:]
        messages.append(outcome[1][1])
    assert len(set(messages)) == len(order) + 1   # each check spoke once, in turn
    assert "must live on a GPU" in messages[-1]


@pytest.mark.gpu
def test_sort_range_rejects_tensors_on_the_wrong_device():
    import torch
    from vulkan_radix_sort_amd import sort_range
    sorter = _NoLibraryCall()
    dk = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="values must live on a GPU"):
        sort_range(sorter, dk, 0, 8, values=torch.zeros(16, dtype=torch.int32))
    with pytest.raises(ValueError, match="count must live on a GPU"):
        sort_range(sorter, dk, 0, 8, count=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="storage must live on a GPU"):
        sort_range(sorter, dk, 0, 8, storage=torch.zeros(1 << 16, dtype=torch.uint8))
