"""CPU-only checks of the key orders of the 32-bit sorts (vrdxHipCmdOrderedSort[KeyValue][Indirect],
vrdxHipCmdOrderedSortSegmented[KeyValue]): the header declares the six functions as their twins with the order word in front
of storageBuffer and defines the three key types, the library exports them, the ctypes signatures and the generated
Sorter.cmd_ordered_sort* methods follow the header's order, api.ORDERED_SORT_CALLS is a table of its own next to the closed
RECORDING_CALLS, and sort_ordered / sort_segments_ordered refuse bad orders, dtypes, shapes, devices and storages on the host
before any library call."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from vulkan_radix_sort_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
TWINS = {"vrdxHipCmdOrderedSort": "vrdxCmdSort",
         "vrdxHipCmdOrderedSortKeyValue": "vrdxCmdSortKeyValue",
         "vrdxHipCmdOrderedSortIndirect": "vrdxCmdSortIndirect",
         "vrdxHipCmdOrderedSortKeyValueIndirect": "vrdxCmdSortKeyValueIndirect",
         "vrdxHipCmdOrderedSortSegmented": "vrdxHipCmdSortSegmented",
         "vrdxHipCmdOrderedSortSegmentedKeyValue": "vrdxHipCmdSortSegmentedKeyValue"}
METHODS = ("cmd_ordered_sort", "cmd_ordered_sort_key_value", "cmd_ordered_sort_indirect", "cmd_ordered_sort_key_value_indirect",
           "cmd_ordered_sort_segmented", "cmd_ordered_sort_segmented_key_value")
CTYPES = {"VkCommandBuffer": ctypes.c_void_p, "VrdxSorter": ctypes.c_void_p, "VkBuffer": ctypes.c_void_p,
          "VkQueryPool": ctypes.c_void_p, "VkDeviceSize": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}


def _declarations():
    """name -> (type, name) of every parameter, in order, of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(vrdx[A-Z]\w+)\s*\(([^)]*)\)\s*;", text):
        out[name] = [tuple(p.split()) for p in params.split(",") if p.strip() and p.strip() != "void"]
    return out


def test_header_library_and_python_agree_on_the_six_entry_points():
    import vulkan_radix_sort_amd as vrdx
    declared = _declarations()
    lib = vrdx.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vrdx.library_path()], capture_output=True, text=True, check=True).stdout
    for name in list(TWINS) + ["vrdxHipDescribeOrderedSortPlan"]:
        assert name in declared, name
        assert name in vrdx.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None, name
        assert f" T {name}\n" in nm, name
    for method in METHODS + ("describe_ordered_sort_plan",):
        assert callable(getattr(vrdx.Sorter, method)), method
    assert [call.c_name for call in api.ORDERED_SORT_CALLS] == list(TWINS)
    assert [call.method for call in api.ORDERED_SORT_CALLS] == list(METHODS)
    assert api.EXPORTED_SYMBOLS[-7:] == tuple(TWINS) + ("vrdxHipDescribeOrderedSortPlan",)   # the last hand-written group
    assert not set(api.ORDERED_SORT_CALLS) & set(api.RECORDING_CALLS)
    for name in ("KEY32_UINT32", "KEY32_INT32", "KEY32_FLOAT32", "KEY32_ORDERS", "order_word32", "sort_ordered", "sort_segments_ordered"):
        assert name in vrdx.__all__ and hasattr(vrdx, name), name


def test_the_key_types_of_the_header_and_of_python():
    import vulkan_radix_sort_amd as vrdx
    text = open(HEADER).read()
    defines = {name: int(value.rstrip("uU"), 0) for name, value in re.findall(r"#define (VRDX_HIP_KEY32_\w+) (\w+)", text)}
    assert defines == {"VRDX_HIP_KEY32_UINT32": 0, "VRDX_HIP_KEY32_INT32": 1, "VRDX_HIP_KEY32_FLOAT32": 2}
    assert (vrdx.KEY32_UINT32, vrdx.KEY32_INT32, vrdx.KEY32_FLOAT32) == (0, 1, 2)
    assert vrdx.KEY32_ORDERS == {"uint32": 0, "int32": 1, "float32": 2}
    assert vrdx.order_word32("uint32") == 0 and vrdx.order_word32("int32", True) == 0x101 and vrdx.order_word32("float32") == 2
    assert vrdx.order_word32("float32", descending=True) == (vrdx.KEY32_FLOAT32 | vrdx.ORDER_DESCENDING) == 0x102
    for bad in ("float64", "uint64", "signed", "", "FLOAT32"):
        with pytest.raises(ValueError, match="order must be one of 'uint32', 'int32', 'float32'"):
            vrdx.order_word32(bad)
    for bad in (2, None, b"int32"):
        with pytest.raises(TypeError, match="order must be one of"):
            vrdx.order_word32(bad)
    # what the header has to say about the float order and about what is left out
    block = text[text.index("Key orders of the 32-bit sorts"):text.index("#define VRDX_HIP_KEY32_UINT32")]
    for phrase in ("totalOrder", "torch.sort puts ALL NaNs last", "-0.0 sorts in front of +0.0", "[13,14]", "Out of scope"):
        assert phrase in block, phrase


def test_each_call_is_its_twin_with_the_order_in_front_of_the_storage():
    declared = _declarations()
    for ordered, twin in TWINS.items():
        want = list(declared[twin])
        at = [name for _, name in want].index("storageBuffer")
        want[at:at] = [("uint32_t", "order")]
        assert declared[ordered] == want, ordered
        assert want[at - 1][1] in ("keysOffset", "valuesOffset")


@pytest.mark.parametrize("call", api.ORDERED_SORT_CALLS, ids=lambda call: call.c_name)
def test_rows_signatures_and_methods_follow_from_the_header(call):
    declaration = _declarations()[call.c_name]
    key_bits, segmented, indirect, key_value, extra = call.facts
    assert (key_bits, extra) == (32, "Ordered")
    assert (segmented, indirect, key_value) == ("Segmented" in call.c_name, "Indirect" in call.c_name, "KeyValue" in call.c_name)
    assert call.argtypes == [CTYPES[c_type] for c_type, _ in declaration]
    lib = api.load_library()
    assert list(getattr(lib, call.c_name).argtypes) == call.argtypes and getattr(lib, call.c_name).restype is None
    twin = getattr(lib, TWINS[call.c_name])
    want = list(twin.argtypes)
    want[-4:-4] = [ctypes.c_uint32]
    assert call.argtypes == want
    method = getattr(api.Sorter, call.method)
    parameters = inspect.signature(method).parameters
    snake = lambda name: re.sub(r"([A-Z])", lambda m: "_" + m.group(1).lower(),  # noqa: E731
                                name if name == "commandBuffer" else re.sub(r"Buffer$", "", name))
    want = ["self" if name == "sorter" else snake(name) for _, name in declaration]
    want.insert(0, want.pop(1))
    assert list(parameters) == want
    assert [p.default for p in parameters.values()][-2:] == [None, 0]
    assert method.__qualname__ == f"Sorter.{call.method}" and method.__doc__ == f"``{call.c_name}``: {call.doc}"


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


@pytest.mark.parametrize("call", api.ORDERED_SORT_CALLS, ids=lambda call: call.method)
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


def test_the_dispatcher_of_the_ordered_table():
    class Tensor:
        def __init__(self, address):
            self.address = address

        def data_ptr(self):
            return self.address

    keys, storage, offsets, count, values = (Tensor(a) for a in (11, 12, 13, 14, 15))
    for call in api.ORDERED_SORT_CALLS:
        _, segmented, indirect, key_value, _ = call.facts
        sorter = _sorter()
        api.record_ordered_sort(sorter, 5, 100, offsets if segmented else None, 3 if segmented else None,
                                count if indirect else None, keys, values if key_value else None, 0x102, storage)
        want = [call.c_name, 5, None, 100] + ([3, 13, 0] if segmented else []) + ([14, 0] if indirect else []) + [11, 0]
        want += ([15, 0] if key_value else []) + [0x102, 12, 0, None, 0]
        assert sorter._lib.calls == [tuple(want)], call.c_name
    with pytest.raises(TypeError, match="no ordered recording call"):
        api.record_ordered_sort(_sorter(), 5, 100, offsets, 3, count, keys, None, 1, storage)
    # record_sort stays closed: no row of RECORDING_CALLS takes 32-bit keys with an order
    with pytest.raises(TypeError, match="no recording call takes"):
        api.record_sort(_sorter(), 32, 5, 100, None, None, None, keys, None, None, 1, storage)


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, uint32_t, VkBuffer, VkDeviceSize,\n"
        "               VkQueryPool, uint32_t) = vrdxHipCmdOrderedSort;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "                VkDeviceSize, uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) =\n"
        "      vrdxHipCmdOrderedSortKeyValueIndirect;\n"
        "  void (*segments)(VkCommandBuffer, VrdxSorter, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize,\n"
        "                   VkBuffer, VkDeviceSize, uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) =\n"
        "      vrdxHipCmdOrderedSortSegmentedKeyValue;\n"
        "  void (*describe)(VrdxSorter, uint32_t, int, uint32_t, VrdxHipPlanInfo*) = vrdxHipDescribeOrderedSortPlan;\n"
        "  uint32_t order = VRDX_HIP_KEY32_FLOAT32 | VRDX_HIP_ORDER_DESCENDING;\n"
        "  return (keys != 0 && pairs != 0 && segments != 0 && describe != 0 && order == 0x102u && VRDX_HIP_KEY32_UINT32 == 0u &&\n"
        "          VRDX_HIP_KEY32_INT32 == 1u) ? 0 : 1;\n}\n")
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "s.o")],
                   check=True)


class _NoLibraryCall:
    """stands in for the sorter: any use of it is a library call the host checks should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"the front end reached the sorter ({name}) with arguments it should have refused")


def _front_ends():
    import torch
    from vulkan_radix_sort_amd import sort_ordered, sort_segments_ordered
    offsets = torch.tensor([0, 16], dtype=torch.int32)
    return [("sort_ordered", lambda keys, **kw: sort_ordered(_NoLibraryCall(), keys, **kw)),
            ("sort_segments_ordered", lambda keys, **kw: sort_segments_ordered(_NoLibraryCall(), keys, offsets, **kw))]


def test_the_front_ends_signatures():
    from vulkan_radix_sort_amd import sort_ordered, sort_segments_ordered
    assert list(inspect.signature(sort_ordered).parameters) == ["sorter", "keys", "values", "storage", "count", "order", "descending"]
    assert list(inspect.signature(sort_segments_ordered).parameters) == ["sorter", "keys", "offsets", "values", "storage", "order",
                                                                         "descending"]
    for fn in (sort_ordered, sort_segments_ordered):
        parameters = inspect.signature(fn).parameters
        assert parameters["order"].default == "uint32" and parameters["descending"].default is False


def test_bad_arguments_are_refused_before_any_library_call():
    import torch
    ints = torch.zeros(16, dtype=torch.int32)
    floats = torch.zeros(16, dtype=torch.float32)
    for name, call in _front_ends():
        for bad in ("float64", "int64", "signed", "", "FLOAT32"):
            with pytest.raises(ValueError, match="order must be one of"):
                call(ints, order=bad)
        for bad in (2, 0x102, True, None, b"int32"):
            with pytest.raises(TypeError, match="order must be one of"):
                call(ints, order=bad)
        with pytest.raises(TypeError, match="descending must be a bool"):
            call(ints, order="int32", descending=1)
        # float32 tensors: only under order="float32"
        for order in ("uint32", "int32"):
            with pytest.raises(TypeError, match="keys must hold 4-byte integers"):
                call(floats, order=order)
        with pytest.raises(TypeError, match="keys must hold 4-byte integers"):
            call(floats)
        for order in ("uint32", "int32", "float32"):
            for bad in (torch.zeros(16, dtype=torch.float64), torch.zeros(16, dtype=torch.int64), torch.zeros(16, dtype=torch.float16)):
                with pytest.raises(TypeError, match="keys must hold"):
                    call(bad, order=order)
            with pytest.raises(TypeError, match="keys must be a torch.Tensor"):
                call([1.0, 2.0], order=order)
            with pytest.raises(ValueError, match="one-dimensional"):
                call(torch.zeros((4, 4), dtype=torch.int32), order=order)
            with pytest.raises(ValueError, match="contiguous"):
                call(torch.zeros(32, dtype=torch.int32)[::2], order=order)
        # everything about the order in order: CPU tensors are what is left to refuse
        for keys, order in ((floats, "float32"), (ints, "float32"), (ints, "int32"), (ints, "uint32")):
            with pytest.raises(ValueError, match="keys must live on a GPU"):
                call(keys, order=order, descending=True)


@pytest.mark.gpu
def test_values_counts_offsets_and_storages_are_refused_before_any_library_call():
    """what is checked behind the keys' device needs keys on a GPU; still no library call"""
    import torch
    from vulkan_radix_sort_amd import sort_ordered, sort_segments_ordered
    keys = torch.zeros(16, dtype=torch.float32, device="cuda")
    offsets = torch.tensor([0, 16], dtype=torch.int32, device="cuda")
    none = _NoLibraryCall()
    for call in (lambda **kw: sort_ordered(none, keys, order="float32", **kw),
                 lambda **kw: sort_segments_ordered(none, keys, offsets, order="float32", **kw)):
        with pytest.raises(TypeError, match="values must hold"):
            call(values=torch.zeros(16, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError, match="values hold 15 elements, keys 16"):
            call(values=torch.zeros(15, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError, match="values must live on a GPU"):
            call(values=torch.zeros(16, dtype=torch.int32))
        with pytest.raises(TypeError, match="storage must be a contiguous uint8"):
            call(storage=torch.zeros(1 << 20, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError, match="storage is on cpu"):
            call(storage=torch.zeros(1 << 20, dtype=torch.uint8))
        with pytest.raises(ValueError, match="16-byte boundary"):
            call(storage=torch.zeros((1 << 20) + 4, dtype=torch.uint8, device="cuda")[4:])
    with pytest.raises(ValueError, match="count must hold one element"):
        sort_ordered(none, keys, count=torch.zeros(2, dtype=torch.int32, device="cuda"), order="float32")
    with pytest.raises(TypeError, match="count must hold"):
        sort_ordered(none, keys, count=torch.zeros(1, dtype=torch.int64, device="cuda"), order="float32")
    with pytest.raises(TypeError, match="offsets must hold"):
        sort_segments_ordered(none, keys, offsets.to(torch.int64), order="float32")
    with pytest.raises(ValueError, match="offsets must live on a GPU"):
        sort_segments_ordered(none, keys, offsets.cpu(), order="float32")


class _Recorder:
    """a sorter that notes which recording call the front end makes"""

    def __init__(self, sorter):
        self._sorter, self.calls = sorter, []

    def __getattr__(self, name):
        attribute = getattr(self._sorter, name)
        if name.startswith("cmd_"):
            self.calls.append(name)
        return attribute


@pytest.mark.gpu
def test_the_front_ends_take_the_ordered_calls():
    import torch
    import vulkan_radix_sort_amd as vrdx
    with vrdx.Sorter() as real:
        s = _Recorder(real)
        keys = torch.arange(64, 0, -1, dtype=torch.int32, device="cuda")
        floats = torch.randn(64, dtype=torch.float32, device="cuda")
        values = torch.arange(64, dtype=torch.int32, device="cuda")
        count = torch.tensor([40], dtype=torch.int32, device="cuda")
        offsets = torch.tensor([0, 30, 64], dtype=torch.int32, device="cuda")
        vrdx.sort_ordered(s, keys)
        vrdx.sort_ordered(s, floats, values, order="float32", descending=True)
        vrdx.sort_ordered(s, keys, count=count, order="int32")
        vrdx.sort_ordered(s, floats, values, count=count, order="float32")
        vrdx.sort_segments_ordered(s, keys, offsets, order="int32", descending=True)
        vrdx.sort_segments_ordered(s, floats, offsets, values, order="float32")
        assert s.calls == list(METHODS)
        torch.cuda.synchronize()
        assert real.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0
