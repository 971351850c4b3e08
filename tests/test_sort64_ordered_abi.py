"""CPU-only checks of the key orders of the 64-bit sorts (vrdxHipCmdSort64Ordered[KeyValue][Indirect],
vrdxHipCmdSortSegmented64Ordered[KeyValue]): the header declares the six functions with the order word right behind the
keys (and values) arguments and defines the order word's constants, the library exports them, the ctypes signatures take the
arguments in the documented order, and sort64 / sort_segments64 refuse bad orders and dtypes on the host before any library
call, while order=None stays the path it was."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
TWINS = {"vrdxHipCmdSort64Ordered": "vrdxHipCmdSort64",
         "vrdxHipCmdSort64OrderedKeyValue": "vrdxHipCmdSort64KeyValue",
         "vrdxHipCmdSort64OrderedIndirect": "vrdxHipCmdSort64Indirect",
         "vrdxHipCmdSort64OrderedKeyValueIndirect": "vrdxHipCmdSort64KeyValueIndirect",
         "vrdxHipCmdSortSegmented64Ordered": "vrdxHipCmdSortSegmented64",
         "vrdxHipCmdSortSegmented64OrderedKeyValue": "vrdxHipCmdSortSegmented64KeyValue"}
METHODS = ("cmd_sort64_ordered", "cmd_sort64_ordered_key_value", "cmd_sort64_ordered_indirect",
           "cmd_sort64_ordered_key_value_indirect", "cmd_sort_segmented64_ordered", "cmd_sort_segmented64_ordered_key_value")


def _declarations():
    """name -> parameter names, in order, of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(vrdx[A-Z]\w+)\s*\(([^)]*)\)\s*;", text):
        out[name] = [p.split()[-1].lstrip("*") for p in params.split(",") if p.strip() and p.strip() != "void"]
    return out


def test_header_library_and_python_agree_on_the_six_entry_points():
    import vulkan_radix_sort_amd as vrdx
    declared = _declarations()
    lib = vrdx.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vrdx.library_path()], capture_output=True, text=True, check=True).stdout
    for name in TWINS:
        assert name in declared, name
        assert name in vrdx.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None, name
        assert f" T {name}\n" in nm, name
    for method in METHODS:
        assert callable(getattr(vrdx.Sorter, method)), method


def test_the_order_word_of_the_header_and_of_python():
    import vulkan_radix_sort_amd as vrdx
    text = open(HEADER).read()
    defines = {name: int(value.rstrip("uU"), 0) for name, value in re.findall(r"#define (VRDX_HIP_(?:KEY|ORDER)_\w+) (\w+)", text)}
    assert defines == {"VRDX_HIP_KEY_UINT64": 0, "VRDX_HIP_KEY_INT64": 1, "VRDX_HIP_KEY_FLOAT64": 2,
                       "VRDX_HIP_ORDER_DESCENDING": 0x100}
    assert (vrdx.KEY_UINT64, vrdx.KEY_INT64, vrdx.KEY_FLOAT64, vrdx.ORDER_DESCENDING) == (0, 1, 2, 0x100)
    assert vrdx.order_word("uint64") == 0 and vrdx.order_word("int64", True) == 0x101 and vrdx.order_word("float64") == 2
    with pytest.raises(ValueError):
        vrdx.order_word("float32")
    with pytest.raises(TypeError):
        vrdx.order_word(2)
    # what the header has to say about the float order
    assert "totalOrder" in text and "torch.sort puts ALL NaNs last" in text and "-0.0 sorts in front of +0.0" in text


def test_the_order_sits_right_behind_the_keys_and_values():
    """each call is its twin with `order` inserted in front of storageBuffer, the position beginBit / endBit have in
    vrdxHipCmdSortBits*"""
    declared = _declarations()
    for ordered, twin in TWINS.items():
        want = list(declared[twin])
        at = want.index("storageBuffer")
        want[at:at] = ["order"]
        assert declared[ordered] == want, ordered
        assert want[at - 1] in ("keysOffset", "valuesOffset")


def test_ctypes_signatures_take_the_documented_order():
    import vulkan_radix_sort_amd as vrdx
    lib = vrdx.load_library()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for ordered, twin in TWINS.items():
        want = list(getattr(lib, twin).argtypes)
        want[-4:-4] = [u32]   # in front of storageBuffer, storageOffset, queryPool, query
        assert list(getattr(lib, ordered).argtypes) == want, ordered
        assert getattr(lib, ordered).restype is None
    assert list(lib.vrdxHipCmdSort64Ordered.argtypes) == [vp, vp, u32, vp, u64, u32, vp, u64, vp, u32]
    assert list(lib.vrdxHipCmdSortSegmented64OrderedKeyValue.argtypes) == [vp, vp, u32, u32, vp, u64, vp, u64, vp, u64, u32, vp,
                                                                          u64, vp, u32]


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, uint32_t, VkBuffer, VkDeviceSize,\n"
        "               VkQueryPool, uint32_t) = vrdxHipCmdSort64Ordered;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkBuffer,\n"
        "                VkDeviceSize, uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) =\n"
        "      vrdxHipCmdSort64OrderedKeyValueIndirect;\n"
        "  void (*segments)(VkCommandBuffer, VrdxSorter, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize,\n"
        "                   uint32_t, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSortSegmented64Ordered;\n"
        "  uint32_t order = VRDX_HIP_KEY_FLOAT64 | VRDX_HIP_ORDER_DESCENDING;\n"
        "  return (keys != 0 && pairs != 0 && segments != 0 && order == 0x102u && VRDX_HIP_KEY_UINT64 == 0u &&\n"
        "          VRDX_HIP_KEY_INT64 == 1u) ? 0 : 1;\n}\n")
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "s.o")],
                   check=True)


class _NoLibraryCall:
    """stands in for the sorter: any use of it is a library call the host checks should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"the front end reached the sorter ({name}) with arguments it should have refused")


def _front_ends():
    import torch
    from vulkan_radix_sort_amd import sort64, sort_segments64
    offsets = torch.tensor([0, 16], dtype=torch.int32)
    return [("sort64", lambda keys, **kw: sort64(_NoLibraryCall(), keys, **kw)),
            ("sort_segments64", lambda keys, **kw: sort_segments64(_NoLibraryCall(), keys, offsets, **kw))]


def test_the_front_ends_take_order_and_descending():
    from vulkan_radix_sort_amd import sort64, sort_segments64
    for fn in (sort64, sort_segments64):
        parameters = inspect.signature(fn).parameters
        assert parameters["order"].default is None and parameters["descending"].default is False


def test_bad_orders_and_dtypes_are_refused_before_any_library_call():
    import torch
    ints = torch.zeros(16, dtype=torch.int64)
    floats = torch.zeros(16, dtype=torch.float64)
    for name, call in _front_ends():
        for bad in ("float32", "int32", "signed", "", "FLOAT64"):
            with pytest.raises(ValueError, match="order must be one of"):
                call(ints, order=bad)
        for bad in (2, 0x102, True, b"int64"):
            with pytest.raises(TypeError, match="order must be one of"):
                call(ints, order=bad)
        with pytest.raises(ValueError, match="descending=True needs an order"):
            call(ints, descending=True)
        with pytest.raises(TypeError, match="descending must be a bool"):
            call(ints, order="int64", descending=1)
        # float64 tensors: only under order="float64"
        with pytest.raises(TypeError, match="keys must hold 8-byte integers"):
            call(floats)                      # (today's behaviour)
        for order in ("uint64", "int64"):
            with pytest.raises(TypeError, match="keys must hold 8-byte integers"):
                call(floats, order=order)
        for order in ("uint64", "int64", "float64"):
            for bad in (torch.zeros(16, dtype=torch.float32), torch.zeros(16, dtype=torch.int32)):
                with pytest.raises(TypeError):
                    call(bad, order=order)
            with pytest.raises(TypeError):
                call([1.0, 2.0], order=order)
            with pytest.raises(ValueError, match="one-dimensional"):
                call(torch.zeros((4, 4), dtype=torch.int64), order=order)
        # everything about the order in order: CPU tensors are what is left to refuse
        for keys, order in ((floats, "float64"), (ints, "float64"), (ints, "int64"), (ints, "uint64"), (ints, None)):
            with pytest.raises(ValueError, match="keys must live on a GPU"):
                call(keys, order=order)
        with pytest.raises(ValueError, match="keys must live on a GPU"):
            call(floats, order="float64", descending=True)


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
def test_order_none_is_the_path_it_was_and_an_order_takes_the_ordered_calls():
    import torch
    import vulkan_radix_sort_amd as vrdx
    with vrdx.Sorter() as real:
        s = _Recorder(real)
        keys = torch.arange(64, 0, -1, dtype=torch.int64, device="cuda")
        values = torch.arange(64, dtype=torch.int32, device="cuda")
        count = torch.tensor([40], dtype=torch.int32, device="cuda")
        offsets = torch.tensor([0, 30, 64], dtype=torch.int32, device="cuda")
        vrdx.sort64(s, keys)
        vrdx.sort64(s, keys, values)
        vrdx.sort64(s, keys, count=count)
        vrdx.sort64(s, keys, values, count=count)
        vrdx.sort_segments64(s, keys, offsets)
        vrdx.sort_segments64(s, keys, offsets, values)
        assert s.calls == ["cmd_sort64", "cmd_sort64_key_value", "cmd_sort64_indirect", "cmd_sort64_key_value_indirect",
                           "cmd_sort_segmented64", "cmd_sort_segmented64_key_value"]
        s.calls.clear()
        floats = torch.randn(64, dtype=torch.float64, device="cuda")
        vrdx.sort64(s, keys, order="uint64")
        vrdx.sort64(s, floats, values, order="float64", descending=True)
        vrdx.sort64(s, keys, count=count, order="int64")
        vrdx.sort64(s, floats, values, count=count, order="float64")
        vrdx.sort_segments64(s, keys, offsets, order="int64", descending=True)
        vrdx.sort_segments64(s, floats, offsets, values, order="float64")
        assert s.calls == ["cmd_sort64_ordered", "cmd_sort64_ordered_key_value", "cmd_sort64_ordered_indirect",
                           "cmd_sort64_ordered_key_value_indirect", "cmd_sort_segmented64_ordered",
                           "cmd_sort_segmented64_ordered_key_value"]
        torch.cuda.synchronize()
        assert real.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0
