"""CPU-only checks of the sorts of 32-bit keys with 64-bit values (vrdxHipCmdWideValueSort[Indirect],
vrdxHipGetSorterWideValueStorageRequirements, vrdxHipDescribeWideValueSortPlan): the header declares the two recording calls
with the arguments of vrdxCmdSortKeyValue[Indirect], the library exports all four names, the ctypes signatures and the generated
Sorter.cmd_wide_value_sort* methods follow the header's order, api.WIDE_VALUE_CALLS is a table of its own next to the closed
RECORDING_CALLS, the storage requirement is the key+value requirement plus 12 bytes per element plus a fixed pad, and
sort_key_value64 refuses bad dtypes, shapes, lengths, devices, views and storages on the host before anything is recorded.

Like every other front end, sort_key_value64 asks first that the keys live on a GPU, so without one only the keys' refusals can
be reached; the refusals of values, count and storage -- still host-side, still nothing recorded -- are in the two tests
marked `gpu`, as in tests/test_ordered_sort_abi.py.  The same holds for the describe call beyond the clamp, which needs a
sorter."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from vulkan_radix_sort_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
TWINS = {"vrdxHipCmdWideValueSort": "vrdxCmdSortKeyValue", "vrdxHipCmdWideValueSortIndirect": "vrdxCmdSortKeyValueIndirect"}
METHODS = ("cmd_wide_value_sort", "cmd_wide_value_sort_indirect")
NAMES = ("vrdxHipGetSorterWideValueStorageRequirements",) + tuple(TWINS) + ("vrdxHipDescribeWideValueSortPlan",)
CTYPES = {"VkCommandBuffer": ctypes.c_void_p, "VrdxSorter": ctypes.c_void_p, "VkBuffer": ctypes.c_void_p,
          "VkQueryPool": ctypes.c_void_p, "VkDeviceSize": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}


def _declarations():
    """name -> (type, name) of every parameter, in order, of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(vrdx[A-Z]\w+)\s*\(([^)]*)\)\s*;", text):
        out[name] = [tuple(p.split()) for p in params.split(",") if p.strip() and p.strip() != "void"]
    return out


def test_header_library_and_python_agree_on_the_four_names():
    import vulkan_radix_sort_amd as vrdx
    declared = _declarations()
    lib = vrdx.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vrdx.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in declared, name
        assert name in vrdx.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None, name
        assert f" T {name}\n" in nm, name
    for method in METHODS + ("wide_value_storage_requirements", "describe_wide_value_sort_plan"):
        assert callable(getattr(vrdx.Sorter, method)), method
    assert [call.c_name for call in api.WIDE_VALUE_CALLS] == list(TWINS)
    assert [call.method for call in api.WIDE_VALUE_CALLS] == list(METHODS)
    # in front of the ordered 32-bit group, which stays the last one
    at = api.EXPORTED_SYMBOLS.index(NAMES[0])
    assert api.EXPORTED_SYMBOLS[at:at + 4] == NAMES and at + 4 == len(api.EXPORTED_SYMBOLS) - 7
    assert len(api.RECORDING_CALLS) == 24 and not set(api.WIDE_VALUE_CALLS) & set(api.RECORDING_CALLS + api.ORDERED_SORT_CALLS)
    for name in ("sort_key_value64", "VrdxHipWideValuePlanInfo", "WIDE_VALUE_FORM_NAMES"):
        assert name in vrdx.__all__ and hasattr(vrdx, name), name
    assert declared["vrdxHipGetSorterWideValueStorageRequirements"] == declared["vrdxGetSorterKeyValueStorageRequirements"]
    assert declared["vrdxHipDescribeWideValueSortPlan"] == [("VrdxSorter", "sorter"), ("uint32_t", "elementCount"),
                                                            ("VrdxHipWideValuePlanInfo*", "info")]


def test_the_forms_and_the_info_structure_of_the_header_and_of_python():
    text = open(HEADER).read()
    defines = {name: int(value.rstrip("uU"), 0) for name, value in re.findall(r"#define (VRDX_HIP_WIDE_VALUE_\w+) (\w+)", text)}
    assert defines == {"VRDX_HIP_WIDE_VALUE_NONE": 0, "VRDX_HIP_WIDE_VALUE_ONE_WORKGROUP": 1, "VRDX_HIP_WIDE_VALUE_GATHER": 2,
                       "VRDX_HIP_WIDE_VALUE_TWO_SORTS": 3}
    assert api.WIDE_VALUE_FORM_NAMES == {0: "none", 1: "one-workgroup", 2: "gather", 3: "two-sorts"}
    struct = re.search(r"typedef struct VrdxHipWideValuePlanInfo \{(.*?)\} VrdxHipWideValuePlanInfo;", text, flags=re.S).group(1)
    fields = re.findall(r"uint32_t (\w+);", struct)
    assert fields == [name for name, _ in api.VrdxHipWideValuePlanInfo._fields_]
    assert all(ctype is ctypes.c_uint32 for _, ctype in api.VrdxHipWideValuePlanInfo._fields_)
    block = text[text.index("32-bit keys with 64-bit values"):text.index("void vrdxHipGetSorterWideValueStorageRequirements")]
    for phrase in ("valuesOffset a multiple of 8", "VRDX_HIP_STATUS_COUNT_CLAMPED", "neither read nor written", "nothing writes it",
                   "ONE_WORKGROUP", "GATHER", "TWO_SORTS", "Out of scope"):
        assert phrase in block, phrase


@pytest.mark.parametrize("call", api.WIDE_VALUE_CALLS, ids=lambda call: call.c_name)
def test_rows_signatures_and_methods_follow_from_the_header(call):
    declared = _declarations()
    declaration = declared[call.c_name]
    assert declaration == declared[TWINS[call.c_name]]   # the arguments of the twin, name for name
    assert call.facts == (32, False, "Indirect" in call.c_name, True, None)
    assert call.argtypes == [CTYPES[c_type] for c_type, _ in declaration]
    lib = api.load_library()
    assert list(getattr(lib, call.c_name).argtypes) == call.argtypes and getattr(lib, call.c_name).restype is None
    assert call.argtypes == list(getattr(lib, TWINS[call.c_name]).argtypes)
    method = getattr(api.Sorter, call.method)
    parameters = inspect.signature(method).parameters
    snake = lambda name: re.sub(r"([A-Z])", lambda m: "_" + m.group(1).lower(),  # noqa: E731
                                name if name == "commandBuffer" else re.sub(r"Buffer$", "", name))
    want = ["self" if name == "sorter" else snake(name) for _, name in declaration]
    want.insert(0, want.pop(1))
    assert list(parameters) == want
    assert [p.default for p in parameters.values()][-2:] == [None, 0]
    assert method.__qualname__ == f"Sorter.{call.method}" and method.__doc__ == f"``{call.c_name}``: {call.doc}"


def test_the_facts_of_every_other_row_are_what_they_were():
    """RecordingCall.facts learnt the two names and nothing else"""
    for call in api.RECORDING_CALLS:
        segmented, wide, extra, key_value, indirect = re.fullmatch(
            r"vrdx(?:Hip)?CmdSort(Segmented)?(64)?(Bits|Ordered)?(KeyValue)?(Indirect)?", call.c_name).groups()
        assert call.facts == (64 if wide else 32, bool(segmented), bool(indirect), bool(key_value), extra), call.c_name
    for call in api.ORDERED_SORT_CALLS:
        assert call.facts == (32, "Segmented" in call.c_name, "Indirect" in call.c_name, "KeyValue" in call.c_name, "Ordered")


class _RecordingLibrary:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name,) + args)


def _sorter():
    sorter = api.Sorter.__new__(api.Sorter)
    sorter.handle = None   # (so that __del__ has nothing to destroy)
    sorter._lib = _RecordingLibrary()
    return sorter


@pytest.mark.parametrize("call", api.WIDE_VALUE_CALLS, ids=lambda call: call.method)
def test_methods_forward_in_the_header_order(call):
    sorter = _sorter()
    method = getattr(sorter, call.method)
    names = list(inspect.signature(method).parameters)
    sentinels = [1000 + 7 * i for i in range(len(names))]
    want = (call.c_name, sentinels[0], 99) + tuple(sentinels[1:])
    assert len(want) == 1 + len(_declarations()[call.c_name])
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


def _requirement(path):
    """the three calculators through a C program of their own: the layout functions need no device"""
    src = path / "requirement.cc"
    src.write_text(
        '#include <cstdio>\n#include "vulkan_radix_sort_amd/csrc/vrdx_layout.h"\n'
        "int main() {\n"
        "  const unsigned sizes[] = {0u, 1u, 2u, 31u, 32u, 33u, 8192u, 8193u, 100003u, 1u << 24, VRDX_MAX_ELEMENTS};\n"
        "  for (unsigned n : sizes) {\n"
        "    const unsigned long long inner = vrdx::MakeLayout(n, VRDX_STORAGE_ALIGN, 0).keyValueSize;\n"
        "    for (unsigned long long address = 0; address < 256; address += 16)\n"
        '      std::printf("%u %llu %llu %llu\\n", n, address, inner,\n'
        "                  (unsigned long long)vrdx::MakeWideValueLayout(n, VRDX_STORAGE_ALIGN, address).size);\n"
        "  }\n  return 0;\n}\n")
    exe = path / "requirement"
    subprocess.run(["g++", "-std=c++17", "-I", ROOT, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(src), "-o", str(exe)], check=True)
    return [tuple(int(x) for x in line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                          check=True).stdout.splitlines()]


def test_the_storage_requirement(tmp_path):
    """the key+value requirement + 12 N + the fixed pad (112 bytes in front of A, 124 in front of B and of C), whatever the
    address the storage is handed over at"""
    rows = _requirement(tmp_path)
    assert len(rows) == 11 * 16
    for n, address, inner, size in rows:
        assert size == inner + 12 * n + 112 + 2 * 124, (n, address)


class _NoLibraryCall:
    """stands in for the sorter: any use of it is a library call the host checks should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"the front end reached the sorter ({name}) with arguments it should have refused")


def test_the_front_end_signature():
    from vulkan_radix_sort_amd import sort_key_value64
    assert list(inspect.signature(sort_key_value64).parameters) == ["sorter", "keys", "values", "count", "storage"]
    assert inspect.signature(sort_key_value64).parameters["count"].default is None


def test_bad_arguments_are_refused_before_any_library_call():
    import torch
    from vulkan_radix_sort_amd import sort_key_value64
    none = _NoLibraryCall()
    keys = torch.zeros(16, dtype=torch.int32)
    values = torch.zeros(16, dtype=torch.int64)
    for bad in (torch.zeros(16, dtype=torch.int64), torch.zeros(16, dtype=torch.float32), torch.zeros(16, dtype=torch.int16)):
        with pytest.raises(TypeError, match="keys must hold 4-byte integers"):
            sort_key_value64(none, bad, values)
    with pytest.raises(TypeError, match="keys must be a torch.Tensor"):
        sort_key_value64(none, [1, 2], values)
    with pytest.raises(ValueError, match="one-dimensional"):
        sort_key_value64(none, torch.zeros((4, 4), dtype=torch.int32), values)
    with pytest.raises(ValueError, match="contiguous"):
        sort_key_value64(none, torch.zeros(32, dtype=torch.int32)[::2], values)
    with pytest.raises(ValueError, match="keys must live on a GPU"):
        sort_key_value64(none, keys, values)


class _SizedSorter:
    """a sorter that answers the storage question and must not be asked to record"""

    def __init__(self, size):
        self._size, self.asked = size, []

    def wide_value_storage_requirements(self, n):
        self.asked.append(n)
        return api.VrdxSorterStorageRequirements(self._size, api.STORAGE_USAGE)

    def __getattr__(self, name):
        raise AssertionError(f"the front end reached the sorter ({name}) with arguments it should have refused")


@pytest.mark.gpu
def test_values_counts_and_storages_are_refused_before_anything_is_recorded():
    """what is checked behind the keys' device needs keys on a GPU; still nothing is recorded"""
    import torch
    from vulkan_radix_sort_amd import sort_key_value64
    keys = torch.zeros(16, dtype=torch.int32, device="cuda")
    values = torch.zeros(16, dtype=torch.int64, device="cuda")
    none = _NoLibraryCall()
    for bad in (torch.int32, torch.float32, torch.int16):
        with pytest.raises(TypeError, match="values must hold 8-byte elements"):
            sort_key_value64(none, keys, torch.zeros(16, dtype=bad, device="cuda"))
    with pytest.raises(ValueError, match="values hold 15 elements, keys 16"):
        sort_key_value64(none, keys, torch.zeros(15, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="values must live on a GPU"):
        sort_key_value64(none, keys, torch.zeros(16, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        sort_key_value64(none, keys, torch.zeros(32, dtype=torch.int64, device="cuda")[::2])
    # 8-byte elements that start 4 bytes off (torch itself hands out no such view: a tensor that says so of itself)
    class Misaligned(torch.Tensor):
        def data_ptr(self):
            return super().data_ptr() + 4

    misaligned = torch.zeros(16, dtype=torch.int64, device="cuda").as_subclass(Misaligned)
    assert misaligned.data_ptr() % 8 == 4 and isinstance(misaligned, torch.Tensor)
    with pytest.raises(ValueError, match="values must start on an 8-byte boundary"):
        sort_key_value64(none, keys, misaligned)
    with pytest.raises(ValueError, match="count must hold one element"):
        sort_key_value64(none, keys, values, count=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError, match="count must hold"):
        sort_key_value64(none, keys, values, count=torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError, match="storage must be a contiguous uint8"):
        sort_key_value64(none, keys, values, storage=torch.zeros(1 << 20, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="storage is on cpu"):
        sort_key_value64(none, keys, values, storage=torch.zeros(1 << 20, dtype=torch.uint8))
    with pytest.raises(ValueError, match="16-byte boundary"):
        sort_key_value64(none, keys, values, storage=torch.zeros((1 << 20) + 4, dtype=torch.uint8, device="cuda")[4:])
    sized = _SizedSorter(1 << 20)
    with pytest.raises(ValueError, match="storage holds 1048575 bytes, the sort needs 1048576"):
        sort_key_value64(sized, keys, values, storage=torch.zeros((1 << 20) - 1, dtype=torch.uint8, device="cuda"))
    assert sized.asked == [16]


@pytest.mark.gpu
def test_the_requirement_of_the_library_is_the_layouts(tmp_path):
    import vulkan_radix_sort_amd as vrdx
    with vrdx.Sorter() as sorter:
        for n, address, inner, size in _requirement(tmp_path):
            if address == 0:
                assert sorter.key_value_storage_requirements(n).size == inner
                req = sorter.wide_value_storage_requirements(n)
                assert (req.size, req.usage) == (size, api.STORAGE_USAGE), n


@pytest.mark.gpu
def test_the_description_at_the_clamp_and_beyond():
    """2^30 - 4 and every count beyond it describe the same plan: the describe call clamps like the recorder"""
    import vulkan_radix_sort_amd as vrdx
    fields = [name for name, _ in api.VrdxHipWideValuePlanInfo._fields_]
    with vrdx.Sorter() as sorter:
        def described(n):
            info = sorter.describe_wide_value_sort_plan(n)
            return [int(getattr(info, name)) for name in fields]
        at_the_clamp = described(0x3FFFFFFC)
        assert sorter.describe_wide_value_sort_plan(0x3FFFFFFC).name == "two-sorts"
        for beyond in (0x3FFFFFFD, 0x40000000, 0x80000000, 0xFFFFFFFF):
            assert described(beyond) == at_the_clamp, beyond
        assert described(0) == [0, 0, 0, 0, 8192, at_the_clamp[5]]
