"""CPU-only checks of the segmented sort of 32-bit keys with 64-bit values (vrdxHipCmdWideValueSortSegmented): the header
declares it behind the wide-value block with the arguments of vrdxHipCmdSortSegmentedKeyValue, name for name; the library
exports it; api.WIDE_VALUE_SEGMENTED_CALLS is a one-row table of its own, its name directly in front of the wide-value group of
EXPORTED_SYMBOLS; ctypes signature, the generated Sorter.cmd_wide_value_sort_segmented and its forwarding order follow the
header; RecordingCall.facts learnt the name and nothing else; and sort_segments_key_value64 refuses bad dtypes, lengths,
alignments, devices and storages on CPU tensors, each with its message, before anything is recorded (the storage's size is the
one thing it has to ask the sorter for; where the arrays live relative to the keys is checked before whether that is a GPU, so
only that last refusal needs none of the others)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from vulkan_radix_sort_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
NAME = "vrdxHipCmdWideValueSortSegmented"
TWIN = "vrdxHipCmdSortSegmentedKeyValue"
METHOD = "cmd_wide_value_sort_segmented"
CTYPES = {"VkCommandBuffer": ctypes.c_void_p, "VrdxSorter": ctypes.c_void_p, "VkBuffer": ctypes.c_void_p,
          "VkQueryPool": ctypes.c_void_p, "VkDeviceSize": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}


def _declarations():
    """name -> (type, name) of every parameter, in order, of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(vrdx[A-Z]\w+)\s*\(([^)]*)\)\s*;", text):
        out[name] = [tuple(p.split()) for p in params.split(",") if p.strip() and p.strip() != "void"]
    return out


def test_header_library_and_python_agree_on_the_name_and_its_position():
    import vulkan_radix_sort_amd as vrdx
    declared = _declarations()
    lib = vrdx.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vrdx.library_path()], capture_output=True, text=True, check=True).stdout
    assert NAME in declared and f" T {NAME}\n" in nm and getattr(lib, NAME) is not None
    assert [(call.c_name, call.method) for call in api.WIDE_VALUE_SEGMENTED_CALLS] == [(NAME, METHOD)]
    assert callable(getattr(vrdx.Sorter, METHOD))
    # directly in front of the wide-value group, which stays 7 from the end; the ordered group stays last
    symbols = api.EXPORTED_SYMBOLS
    at = symbols.index(NAME)
    assert symbols[at + 1] == "vrdxHipGetSorterWideValueStorageRequirements" and at + 1 + 4 == len(symbols) - 7
    assert symbols[-7:] == tuple(call.c_name for call in api.ORDERED_SORT_CALLS) + ("vrdxHipDescribeOrderedSortPlan",)
    assert symbols.count(NAME) == 1 and len(set(symbols)) == len(symbols)
    # the other tables are what they were
    assert [call.c_name for call in api.WIDE_VALUE_CALLS] == ["vrdxHipCmdWideValueSort", "vrdxHipCmdWideValueSortIndirect"]
    assert len(api.RECORDING_CALLS) == 24 and len(api.ORDERED_SORT_CALLS) == 6
    assert not set(api.WIDE_VALUE_SEGMENTED_CALLS) & set(api.RECORDING_CALLS + api.ORDERED_SORT_CALLS + api.WIDE_VALUE_CALLS)
    assert not re.fullmatch(r"vrdx(Hip)?CmdSort\w*", NAME)
    for name in ("sort_segments_key_value64", "WIDE_VALUE_SEGMENTED_CALLS"):
        assert name in vrdx.__all__ and hasattr(vrdx, name), name


def test_the_header_section_stands_behind_the_wide_value_block():
    text = open(HEADER).read()
    assert text.index("void vrdxHipDescribeWideValueSortPlan") < text.index("Segmented sort of 32-bit keys with 64-bit values") \
        < text.index(f"void {NAME}(") < text.index("HIP-side companions of the Vulkan objects")
    assert len(re.findall(r"#define VRDX_HIP_WIDE_VALUE_\w+", text)) == 4   # the four forms of the flat call, no new one
    block = text[text.index("Segmented sort of 32-bit keys with 64-bit values"):text.index(f"void {NAME}(")]
    for phrase in ("valuesOffset a multiple of 8", "VRDX_HIP_STATUS_SEGMENTS_INVALID", "VRDX_HIP_STATUS_COUNT_CLAMPED",
                   "VRDX_HIP_VERDICT_NONE", "vrdxHipGetSorterWideValueStorageRequirements", "read on the device only",
                   "not written at all", "all 15 slots", "stream capture", "same segmentCount"):
        assert phrase in block, phrase


def test_the_declaration_the_row_and_the_method_follow_from_the_twin():
    (call,) = api.WIDE_VALUE_SEGMENTED_CALLS
    declared = _declarations()
    declaration = declared[NAME]
    assert declaration == declared[TWIN]   # the arguments of vrdxHipCmdSortSegmentedKeyValue, name for name
    assert call.facts == (32, True, False, True, None)
    assert call.argtypes == [CTYPES[c_type] for c_type, _ in declaration]
    lib = api.load_library()
    assert list(getattr(lib, NAME).argtypes) == call.argtypes and getattr(lib, NAME).restype is None
    assert call.argtypes == list(getattr(lib, TWIN).argtypes)
    method = getattr(api.Sorter, METHOD)
    parameters = inspect.signature(method).parameters
    assert list(parameters) == ["self", "command_buffer", "max_element_count", "segment_count", "offsets", "offsets_offset", "keys",
                                "keys_offset", "values", "values_offset", "storage", "storage_offset", "query_pool", "query"]
    assert list(parameters) == list(inspect.signature(api.Sorter.cmd_sort_segmented_key_value).parameters)
    assert [p.default for p in parameters.values()][-2:] == [None, 0]
    assert method.__qualname__ == f"Sorter.{METHOD}" and method.__doc__ == f"``{NAME}``: {call.doc}"


def test_the_facts_of_every_other_row_are_what_they_were():
    """RecordingCall.facts learnt the one name and nothing else"""
    for call in api.RECORDING_CALLS:
        segmented, wide, extra, key_value, indirect = re.fullmatch(
            r"vrdx(?:Hip)?CmdSort(Segmented)?(64)?(Bits|Ordered)?(KeyValue)?(Indirect)?", call.c_name).groups()
        assert call.facts == (64 if wide else 32, bool(segmented), bool(indirect), bool(key_value), extra), call.c_name
    for call in api.ORDERED_SORT_CALLS:
        assert call.facts == (32, "Segmented" in call.c_name, "Indirect" in call.c_name, "KeyValue" in call.c_name, "Ordered")
    for call in api.WIDE_VALUE_CALLS:
        assert call.facts == (32, False, "Indirect" in call.c_name, True, None)


class _RecordingLibrary:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name,) + args)


def test_the_method_forwards_in_the_header_order():
    sorter = api.Sorter.__new__(api.Sorter)
    sorter.handle = None   # (so that __del__ has nothing to destroy)
    sorter._lib = _RecordingLibrary()
    method = getattr(sorter, METHOD)
    names = list(inspect.signature(method).parameters)
    sentinels = [1000 + 7 * i for i in range(len(names))]
    want = (NAME, sentinels[0], 99) + tuple(sentinels[1:])
    assert len(want) == 1 + len(_declarations()[NAME])
    for how in ("positional", "defaults", "keywords"):
        sorter.handle = 99
        if how == "positional":
            method(*sentinels)
        elif how == "defaults":
            method(*sentinels[:-2])
        else:
            method(**dict(reversed(list(zip(names, sentinels)))))
        sorter.handle = None
        assert sorter._lib.calls.pop() == (want[:-2] + (None, 0) if how == "defaults" else want), how


class _NoLibraryCall:
    """stands in for the sorter: any use of it is a library call the host checks should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"the front end reached the sorter ({name}) with arguments it should have refused")


class _SizedSorter:
    """a sorter that answers the storage question and must not be asked to record"""

    def __init__(self, size):
        self._size, self.asked = size, []

    def wide_value_storage_requirements(self, n):
        self.asked.append(n)
        return api.VrdxSorterStorageRequirements(self._size, api.STORAGE_USAGE)

    def __getattr__(self, name):
        raise AssertionError(f"the front end reached the sorter ({name}) with arguments it should have refused")


def test_the_front_end_signature():
    from vulkan_radix_sort_amd import sort_segments_key_value64
    parameters = inspect.signature(sort_segments_key_value64).parameters
    assert list(parameters) == ["sorter", "keys", "offsets", "values", "storage"] and parameters["storage"].default is None
    assert parameters["values"].default is inspect.Parameter.empty


def test_the_front_end_refuses_on_cpu_tensors_before_any_library_call():
    import torch
    from vulkan_radix_sort_amd import sort_segments_key_value64 as front_end
    none = _NoLibraryCall()
    keys = torch.zeros(16, dtype=torch.int32)
    offsets = torch.tensor([0, 7, 16], dtype=torch.int32)
    values = torch.zeros(16, dtype=torch.int64)
    # dtypes
    for bad in (torch.int64, torch.float32, torch.int16):
        with pytest.raises(TypeError, match=r"keys must hold 4-byte integers \(int32 or uint32, sorted as uint32\), got"):
            front_end(none, torch.zeros(16, dtype=bad), offsets, values)
    for bad in (torch.int64, torch.float32, torch.uint8):
        with pytest.raises(TypeError, match=r"offsets must hold 4-byte integers \(int32 or uint32\), got"):
            front_end(none, keys, torch.zeros(3, dtype=bad), values)
    for bad in (torch.int32, torch.float32, torch.int16):
        with pytest.raises(TypeError, match=r"values must hold 8-byte elements \(int64, uint64 or float64\), got"):
            front_end(none, keys, offsets, torch.zeros(16, dtype=bad))
    with pytest.raises(TypeError, match="values must be a torch.Tensor, got NoneType"):
        front_end(none, keys, offsets, None)
    # shapes and lengths
    with pytest.raises(ValueError, match="keys must be one-dimensional"):
        front_end(none, torch.zeros((4, 4), dtype=torch.int32), offsets, values)
    with pytest.raises(ValueError, match="offsets must be one-dimensional"):
        front_end(none, keys, torch.zeros((1, 3), dtype=torch.int32), values)
    with pytest.raises(ValueError, match=r"offsets must hold segment_count \+ 1 >= 1 entries"):
        front_end(none, keys, torch.zeros(0, dtype=torch.int32), values)
    with pytest.raises(ValueError, match="values hold 15 elements, keys 16"):
        front_end(none, keys, offsets, torch.zeros(15, dtype=torch.float64))
    with pytest.raises(ValueError, match="values must be contiguous"):
        front_end(none, keys, offsets, torch.zeros(32, dtype=torch.int64)[::2])

    # 8-byte elements that start 4 bytes off (torch itself hands out no such view: a tensor that says so of itself)
    class Misaligned(torch.Tensor):
        def data_ptr(self):
            return super().data_ptr() + 4

    misaligned = torch.zeros(16, dtype=torch.float64).as_subclass(Misaligned)
    assert misaligned.data_ptr() % 8 == 4
    with pytest.raises(ValueError, match="values must start on an 8-byte boundary"):
        front_end(none, keys, offsets, misaligned)
    # devices: every array where the keys are
    with pytest.raises(ValueError, match="offsets is on meta, keys are on cpu"):
        front_end(none, keys, torch.zeros(3, dtype=torch.int32, device="meta"), values)
    with pytest.raises(ValueError, match="values is on meta, keys are on cpu"):
        front_end(none, keys, offsets, torch.zeros(16, dtype=torch.int64, device="meta"))
    # the storage
    with pytest.raises(TypeError, match="storage must be a contiguous uint8 torch.Tensor"):
        front_end(none, keys, offsets, values, storage=torch.zeros(1 << 16, dtype=torch.int32))
    with pytest.raises(ValueError, match="storage is on meta, keys are on cpu"):
        front_end(none, keys, offsets, values, storage=torch.zeros(1 << 16, dtype=torch.uint8, device="meta"))
    base = torch.zeros((1 << 16) + 32, dtype=torch.uint8)
    lead = (4 - base.data_ptr()) % 16
    with pytest.raises(ValueError, match="storage must start on a 16-byte boundary"):
        front_end(none, keys, offsets, values, storage=base[lead:lead + (1 << 16)])
    sized = _SizedSorter(1 << 16)
    aligned = (0 - base.data_ptr()) % 16
    with pytest.raises(ValueError, match="storage holds 65535 bytes, the sort needs 65536"):
        front_end(sized, keys, offsets, values, storage=base[aligned:aligned + (1 << 16) - 1])
    assert sized.asked == [16]
    # and last, with everything else in order: the place must be a GPU
    sized = _SizedSorter(1 << 16)
    for storage in (None, base[aligned:aligned + (1 << 16)]):
        with pytest.raises(ValueError, match="keys must live on a GPU, got cpu"):
            front_end(sized, keys, offsets, values, storage=storage)
    for good in (torch.float64, torch.int64):   # (both value types get that far)
        with pytest.raises(ValueError, match="keys must live on a GPU, got cpu"):
            front_end(sized, keys, offsets, torch.zeros(16, dtype=good))


def test_the_messages_of_the_flat_front_end_did_not_change():
    """sort_key_value64 still asks first that the keys live on a GPU"""
    import torch
    from vulkan_radix_sort_amd import sort_key_value64
    with pytest.raises(ValueError, match="keys must live on a GPU, got cpu"):
        sort_key_value64(_NoLibraryCall(), torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.int32))
