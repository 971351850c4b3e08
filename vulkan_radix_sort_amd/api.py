"""ctypes binding of libvrdx_hip.so -- the vrdx* entry points of include/vk_radix_sort.h.

Mirrors the reference interface (src/vk_radix_sort.h.in:11-81 under /root/reference):

=============================================  ==============================================
reference (C++ / Vulkan)                        here
=============================================  ==============================================
``vrdxCreateSorter(&info, &sorter)``            ``Sorter(device=None)`` (raises ``VrdxError``)
``vrdxDestroySorter(sorter)``                   ``Sorter.destroy()`` / context manager
``vrdxGetSorterStorageRequirements``            ``Sorter.storage_requirements(n)``
``vrdxGetSorterKeyValueStorageRequirements``    ``Sorter.key_value_storage_requirements(n)``
``vrdxCmdSort``                                 ``Sorter.cmd_sort(stream, n, keys, keys_off, storage, storage_off, pool, query)``
``vrdxCmdSortIndirect``                         ``Sorter.cmd_sort_indirect(...)``
``vrdxCmdSortKeyValue``                         ``Sorter.cmd_sort_key_value(...)``
``vrdxCmdSortKeyValueIndirect``                 ``Sorter.cmd_sort_key_value_indirect(...)``
=============================================  ==============================================

The HIP-only recording calls (segmented, 64-bit, by a bit range, in a key order) stand next to those four in
``RECORDING_CALLS``, one row each: the exported names, the ctypes signatures and the ``Sorter.cmd_*`` methods all come from
that table.  The ordered sorts of 32-bit keys (``vrdxHipCmdOrderedSort*``: int32, float32, descending) have a second table of the
same kind, ``ORDERED_SORT_CALLS``, and ``record_ordered_sort`` next to ``record_sort``.

``VkCommandBuffer`` is a ``hipStream_t`` (an ``int`` handle, e.g. ``torch.cuda.current_stream().cuda_stream``),
``VkBuffer`` is a device address (``tensor.data_ptr()``), offsets are bytes.  Like the reference,
the ``cmd_*`` calls validate nothing and never block the host.
"""
from __future__ import annotations

import ctypes
import linecache
import os
import re
from typing import NamedTuple, Optional

VK_SUCCESS = 0
VK_NOT_READY = 1
VK_ERROR_OUT_OF_HOST_MEMORY = -1
VK_ERROR_INITIALIZATION_FAILED = -3
VK_ERROR_FEATURE_NOT_PRESENT = -8

# VK_BUFFER_USAGE_STORAGE_BUFFER_BIT | VK_BUFFER_USAGE_TRANSFER_DST_BIT
STORAGE_USAGE = 0x20 | 0x02


class RecordingCall(NamedTuple):
    """One vrdx*CmdSort* entry point: its C name, the ``Sorter`` method that forwards to it and that method's docstring (what
    stands behind the C name, which the method puts in front).  The name says what the call takes --
    ``vrdx[Hip]CmdSort[Segmented][64][Bits|Ordered][KeyValue][Indirect]``, or, for the rows of ``ORDERED_SORT_CALLS``,
    ``vrdxHipCmdOrderedSort[Segmented][KeyValue][Indirect]`` -- and the argument list follows from that alone,
    always in this order (``parameters``):

        commandBuffer, sorter, count, [segmentCount, offsets, offsetsOffset | indirect, indirectOffset], keys, keysOffset,
        [values, valuesOffset], [beginBit, endBit | order], storage, storageOffset, queryPool, query

    No call is both segmented and indirect.  A new variant is a new row."""
    c_name: str
    method: str
    doc: str

    @property
    def facts(self):
        """(key bits, segmented, indirect, key+value, None | "Bits" | "Ordered"), parsed from the C name"""
        ordered32 = re.fullmatch(r"vrdxHipCmdOrderedSort(Segmented)?(KeyValue)?(Indirect)?", self.c_name)
        wide_value = re.fullmatch(r"vrdxHipCmdWideValueSort(Indirect)?", self.c_name)
        range_sort = re.fullmatch(r"vrdxHipCmdRangeSort(KeyValue)?(Indirect)?", self.c_name)
        balanced = re.fullmatch(r"vrdxHipCmdBalancedSortSegmented(KeyValue)?", self.c_name)
        if balanced:   # the rows of BALANCED_SEGMENTED_CALLS: the arguments of vrdxHipCmdSortSegmented[KeyValue]
            return 32, True, False, bool(balanced.group(1)), None
        if range_sort:   # the rows of RANGE_SORT_CALLS: the arguments of vrdxHipCmdSortBits*
            return 32, False, bool(range_sort.group(2)), bool(range_sort.group(1)), "Bits"
        if self.c_name == "vrdxHipCmdWideValueSortSegmented":   # the row of WIDE_VALUE_SEGMENTED_CALLS
            return 32, True, False, True, None
        if wide_value:   # the rows of WIDE_VALUE_CALLS: uint32 keys, always with values (of 8 bytes: the argument list is the same)
            return 32, False, bool(wide_value.group(1)), True, None
        if ordered32:   # the ordered 32-bit sorts carry the word in front: their names are not of the CmdSort family
            segmented, key_value, indirect = ordered32.groups()
            wide, extra = None, "Ordered"
        else:
            segmented, wide, extra, key_value, indirect = re.fullmatch(
                r"vrdx(?:Hip)?CmdSort(Segmented)?(64)?(Bits|Ordered)?(KeyValue)?(Indirect)?", self.c_name).groups()
        assert not (segmented and indirect), self.c_name
        return 64 if wide else 32, bool(segmented), bool(indirect), bool(key_value), extra

    @property
    def parameters(self):
        """(Python name, ctypes type) of every argument but the sorter, in the C order"""
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        _, segmented, indirect, key_value, extra = self.facts
        out = [("command_buffer", vp), ("max_element_count" if segmented or indirect else "element_count", u32)]
        if segmented:
            out += [("segment_count", u32), ("offsets", vp), ("offsets_offset", u64)]
        if indirect:
            out += [("indirect", vp), ("indirect_offset", u64)]
        out += [("keys", vp), ("keys_offset", u64)]
        if key_value:
            out += [("values", vp), ("values_offset", u64)]
        out += {None: [], "Bits": [("begin_bit", u32), ("end_bit", u32)], "Ordered": [("order", u32)]}[extra]
        return out + [("storage", vp), ("storage_offset", u64), ("query_pool", vp), ("query", u32)]

    @property
    def argtypes(self):
        types = [ctype for _, ctype in self.parameters]
        return types[:1] + [ctypes.c_void_p] + types[1:]   # the sorter comes second


_CALL = RecordingCall
RECORDING_CALLS = (
    # the reference's four (src/vk_radix_sort.h.in:46-81)
    _CALL("vrdxCmdSort", "cmd_sort",
          "uint32 keys, ascending, in place; storage of ``storage_requirements(n)`` bytes."),
    _CALL("vrdxCmdSortIndirect", "cmd_sort_indirect",
          "``cmd_sort`` of the first min(count, ``max_element_count``) keys, the count one uint32 at "
          "``indirect + indirect_offset`` that is read on the device."),
    _CALL("vrdxCmdSortKeyValue", "cmd_sort_key_value",
          "the same as ``cmd_sort`` with values that travel with their keys; storage of "
          "``key_value_storage_requirements(n)`` bytes."),
    _CALL("vrdxCmdSortKeyValueIndirect", "cmd_sort_key_value_indirect",
          "``cmd_sort_indirect`` with values that travel with their keys."),
    # many independent arrays in one call
    _CALL("vrdxHipCmdSortSegmented", "cmd_sort_segmented",
          "segment i = elements [o[i], o[i + 1]) of the keys, o = segment_count + 1 uint32 "
          "offsets read on the device; every segment sorted on its own, in place."),
    _CALL("vrdxHipCmdSortSegmentedKeyValue", "cmd_sort_segmented_key_value",
          "the same with values that travel with their keys."),
    # uint64 keys
    _CALL("vrdxHipCmdSort64", "cmd_sort64",
          "uint64 keys (``keys_offset`` a multiple of 8), ascending and stable, in place; storage of "
          "``storage_requirements64(n)`` bytes."),
    _CALL("vrdxHipCmdSort64KeyValue", "cmd_sort64_key_value",
          "the same with one uint32 value per key; storage of "
          "``storage_requirements64(n, key_value=True)`` bytes."),
    _CALL("vrdxHipCmdSort64Indirect", "cmd_sort64_indirect",
          "``cmd_sort64`` of the first min(count, ``max_element_count``) keys, the count one "
          "uint32 at ``indirect + indirect_offset`` that is read on the device; storage of "
          "``storage_requirements64(max_element_count)`` bytes."),
    _CALL("vrdxHipCmdSort64KeyValueIndirect", "cmd_sort64_key_value_indirect",
          "the same with one uint32 value per key; storage of "
          "``storage_requirements64(max_element_count, key_value=True)`` bytes."),
    # many independent arrays of uint64 keys in one call
    _CALL("vrdxHipCmdSortSegmented64", "cmd_sort_segmented64",
          "``cmd_sort_segmented`` of uint64 keys (``keys_offset`` a multiple of 8); storage of "
          "``storage_requirements64(max_element_count)`` bytes."),
    _CALL("vrdxHipCmdSortSegmented64KeyValue", "cmd_sort_segmented64_key_value",
          "the same with one uint32 value per key; storage of "
          "``storage_requirements64(max_element_count, key_value=True)`` bytes."),
    # by a bit range of the key: the range sits right behind the keys (and values)
    _CALL("vrdxHipCmdSortBits", "cmd_sort_bits",
          "stable sort by the bits [begin_bit, end_bit) of the uint32 keys, which move whole; storage "
          "of ``storage_requirements(n)`` bytes.  Up to 16384 elements (more are refused, except with [0, 32))."),
    _CALL("vrdxHipCmdSortBitsKeyValue", "cmd_sort_bits_key_value",
          "the same with values that travel with their keys; storage of "
          "``key_value_storage_requirements(n)`` bytes."),
    _CALL("vrdxHipCmdSortBitsIndirect", "cmd_sort_bits_indirect",
          "``cmd_sort_bits`` of the first min(count, ``max_element_count``) keys, the count "
          "one uint32 at ``indirect + indirect_offset`` that is read on the device."),
    _CALL("vrdxHipCmdSortBitsKeyValueIndirect", "cmd_sort_bits_key_value_indirect",
          "the same with values that travel with their keys."),
    _CALL("vrdxHipCmdSortSegmentedBits", "cmd_sort_segmented_bits",
          "``cmd_sort_segmented`` by the bits [begin_bit, end_bit) of the keys -- every "
          "segment stable by that field, keys moved whole; segments of any size."),
    _CALL("vrdxHipCmdSortSegmentedBitsKeyValue", "cmd_sort_segmented_bits_key_value",
          "the same with values that travel with their keys."),
    # int64, float64 and descending orders of the uint64 sorts: the order word sits where the bit-range sorts have their range
    _CALL("vrdxHipCmdSort64Ordered", "cmd_sort64_ordered",
          "``cmd_sort64`` in the order of the word ``order`` (``KEY_UINT64``, ``KEY_INT64`` or "
          "``KEY_FLOAT64``, ``| ORDER_DESCENDING``): stable in both directions, keys come back bit for bit."),
    _CALL("vrdxHipCmdSort64OrderedKeyValue", "cmd_sort64_ordered_key_value",
          "the same with one uint32 value per key."),
    _CALL("vrdxHipCmdSort64OrderedIndirect", "cmd_sort64_ordered_indirect",
          "``cmd_sort64_indirect`` in the order of the word ``order``."),
    _CALL("vrdxHipCmdSort64OrderedKeyValueIndirect", "cmd_sort64_ordered_key_value_indirect",
          "the same with one uint32 value per key."),
    _CALL("vrdxHipCmdSortSegmented64Ordered", "cmd_sort_segmented64_ordered",
          "``cmd_sort_segmented64`` with every segment in the order of the word "
          "``order``."),
    _CALL("vrdxHipCmdSortSegmented64OrderedKeyValue", "cmd_sort_segmented64_ordered_key_value",
          "the same with one uint32 value per key."),
)

# int32, float32 and descending orders of the uint32 sorts: a table of its own (the CmdSort family above is closed), the same
# kind of row; the order word sits where the 64-bit ordered sorts have theirs
ORDERED_SORT_CALLS = (
    _CALL("vrdxHipCmdOrderedSort", "cmd_ordered_sort",
          "``cmd_sort`` in the order of the word ``order`` (``KEY32_UINT32``, ``KEY32_INT32`` or ``KEY32_FLOAT32``, "
          "``| ORDER_DESCENDING``): stable in both directions, keys come back bit for bit."),
    _CALL("vrdxHipCmdOrderedSortKeyValue", "cmd_ordered_sort_key_value",
          "the same with values that travel with their keys."),
    _CALL("vrdxHipCmdOrderedSortIndirect", "cmd_ordered_sort_indirect",
          "``cmd_sort_indirect`` in the order of the word ``order``."),
    _CALL("vrdxHipCmdOrderedSortKeyValueIndirect", "cmd_ordered_sort_key_value_indirect",
          "the same with values that travel with their keys."),
    _CALL("vrdxHipCmdOrderedSortSegmented", "cmd_ordered_sort_segmented",
          "``cmd_sort_segmented`` with every segment in the order of the word ``order``."),
    _CALL("vrdxHipCmdOrderedSortSegmentedKeyValue", "cmd_ordered_sort_segmented_key_value",
          "the same with values that travel with their keys."),
)

# uint32 keys with values of 8 bytes: a third table (the names are outside the CmdSort family on purpose), the same kind of row;
# the arguments are those of vrdxCmdSortKeyValue[Indirect]
WIDE_VALUE_CALLS = (
    _CALL("vrdxHipCmdWideValueSort", "cmd_wide_value_sort",
          "``cmd_sort_key_value`` with values of 8 opaque bytes each (``values_offset`` a multiple of 8); storage of "
          "``wide_value_storage_requirements(n)`` bytes."),
    _CALL("vrdxHipCmdWideValueSortIndirect", "cmd_wide_value_sort_indirect",
          "``cmd_wide_value_sort`` of the first min(count, ``max_element_count``) elements, the count one uint32 at "
          "``indirect + indirect_offset`` that is read on the device; storage of "
          "``wide_value_storage_requirements(max_element_count)`` bytes."),
)

# the segmented form of it: a one-row table of its own (WIDE_VALUE_CALLS stays the two flat calls); the arguments are those of
# vrdxHipCmdSortSegmentedKeyValue
WIDE_VALUE_SEGMENTED_CALLS = (
    _CALL("vrdxHipCmdWideValueSortSegmented", "cmd_wide_value_sort_segmented",
          "``cmd_sort_segmented_key_value`` with values of 8 opaque bytes each (``values_offset`` a multiple of 8); storage of "
          "``wide_value_storage_requirements(max_element_count)`` bytes."),
)

# by a bit range of the key at every size: a table of its own next to the others (RECORDING_CALLS stays as it is), the same
# kind of row; the arguments are those of vrdxHipCmdSortBits[KeyValue][Indirect], name for name
RANGE_SORT_CALLS = (
    _CALL("vrdxHipCmdRangeSort", "cmd_range_sort",
          "``cmd_sort_bits`` with no size at which a range is refused: up to 16384 elements the same launch, beyond that "
          "count, scan and scatter per digit of the range over up to one chunk per compute unit; storage of "
          "``storage_requirements(n)`` bytes."),
    _CALL("vrdxHipCmdRangeSortKeyValue", "cmd_range_sort_key_value",
          "the same with values that travel with their keys; storage of ``key_value_storage_requirements(n)`` bytes."),
    _CALL("vrdxHipCmdRangeSortIndirect", "cmd_range_sort_indirect",
          "``cmd_range_sort`` of the first min(count, ``max_element_count``) keys, the count one uint32 at "
          "``indirect + indirect_offset`` that is read on the device."),
    _CALL("vrdxHipCmdRangeSortKeyValueIndirect", "cmd_range_sort_key_value_indirect",
          "the same with values that travel with their keys."),
)

# the segmented sort that spreads huge segments over every compute unit: a table of its own (RECORDING_CALLS stays as it is);
# the arguments are those of vrdxHipCmdSortSegmented[KeyValue], name for name
BALANCED_SEGMENTED_CALLS = (
    _CALL("vrdxHipCmdBalancedSortSegmented", "cmd_balanced_sort_segmented",
          "``cmd_sort_segmented`` with one difference: a segment that is long and longer than its share of the chip is cut "
          "into pieces that many workgroups sort together; the result is the same bit for bit."),
    _CALL("vrdxHipCmdBalancedSortSegmentedKeyValue", "cmd_balanced_sort_segmented_key_value",
          "the same with values that travel with their keys; storage of ``key_value_storage_requirements(n)`` bytes."),
)


def _exported_symbols():
    """Everything the library exports, in the order this tuple has always had: the entry points that record no sort, by hand,
    each group followed by the next so many rows of RECORDING_CALLS."""
    layout = (
        # the reference's eight entry points (src/vk_radix_sort.h.in:24-81)
        (("vrdxCreateSorter", "vrdxDestroySorter", "vrdxGetSorterStorageRequirements",
          "vrdxGetSorterKeyValueStorageRequirements"), 4),
        # HIP companions of the Vulkan objects callers create themselves; behind them the segmented sorts
        (("vrdxHipCreateQueryPool", "vrdxHipDestroyQueryPool", "vrdxHipGetQueryPoolResults", "vrdxHipReadStatus",
          "vrdxHipReadSorterStatus", "vrdxHipRecheck", "vrdxHipEventOverheadNs", "vrdxHipDescribePlan",
          "vrdxHipReadPlanVerdict", "vrdxHipReadPlanCounters", "vrdxHipVersionString"), 2),
        # uint64 keys: plain, segmented; then the four sorts by a bit range
        (("vrdxHipGetSorter64StorageRequirements", "vrdxHipGetSorter64KeyValueStorageRequirements"), 10),
        # behind it the segmented sorts by a bit range and the ordered 64-bit sorts
        (("vrdxHipDescribeSortBitsPlan",), 8),
    )
    rows = iter(RECORDING_CALLS)
    for names, recording in layout:
        yield from names
        yield from (next(rows).c_name for _ in range(recording))
    assert next(rows, None) is None, "a row of RECORDING_CALLS is missing from EXPORTED_SYMBOLS"
    # the range sorts at every size: behind the rows of RECORDING_CALLS (the groups below keep their distance from the end)
    yield from (call.c_name for call in RANGE_SORT_CALLS)
    yield "vrdxHipDescribeRangeSortPlan"
    # uint32 keys with 8-byte values: the segmented call, then the flat group
    yield from (call.c_name for call in WIDE_VALUE_SEGMENTED_CALLS)
    yield "vrdxHipGetSorterWideValueStorageRequirements"
    yield from (call.c_name for call in WIDE_VALUE_CALLS)
    yield "vrdxHipDescribeWideValueSortPlan"
    # the ordered 32-bit sorts
    yield from (call.c_name for call in ORDERED_SORT_CALLS)
    yield "vrdxHipDescribeOrderedSortPlan"


EXPORTED_SYMBOLS = tuple(_exported_symbols())
# what include/vk_radix_sort_balanced.h declares: a tuple of its own, EXPORTED_SYMBOLS is what include/vk_radix_sort.h declares
BALANCED_EXPORTED_SYMBOLS = tuple(call.c_name for call in BALANCED_SEGMENTED_CALLS) + (
    "vrdxHipDescribeBalancedSegmentedPlan", "vrdxHipReadBalancedSplit")


def _compiled(name, source, **names):
    """The function ``name`` that ``source`` defines, compiled once with ``names`` in reach (the technique of
    ``collections.namedtuple`` and ``dataclasses``); tracebacks and ``inspect.getsource`` find the text under a file name of
    its own."""
    filename = f"<vrdx binding {name}>"
    namespace = dict(names, __name__=__name__)
    exec(compile(source, filename, "exec"), namespace)
    linecache.cache[filename] = (len(source), None, source.splitlines(True), filename)
    return namespace[name]


def _recorder(call: RecordingCall):
    """``record_sort``'s way to ``call``: a function of everything ``record_sort`` takes that lays out what this call takes
    in the canonical order, every byte offset 0, and calls the method on the sorter it is handed.  Compiled from the row like
    the methods themselves (``_recording_method``), for the same reason."""
    spelled = {"command_buffer": "stream", "element_count": "count", "max_element_count": "count",
               "begin_bit": "bit_range[0]", "end_bit": "bit_range[1]"}
    arguments = ["0" if name.endswith("_offset") else f"{name}.data_ptr()" if ctype is ctypes.c_void_p and name not in spelled
                 else spelled.get(name, name) for name, ctype in call.parameters[:-2]]
    return _compiled(f"record_{call.method}",
                     f"def record_{call.method}(sorter, stream, count, offsets, segment_count, indirect, keys, values, "
                     f"bit_range, order, storage):\n    sorter.{call.method}({', '.join(arguments)})\n")


def _takes(key_bits, segmented, indirect, key_value, extra):
    return key_bits, segmented, indirect, key_value, extra == "Bits", extra == "Ordered"


_RECORDERS = {_takes(*call.facts): _recorder(call) for call in RECORDING_CALLS}


def record_sort(sorter, key_bits, stream, count, offsets, segment_count, indirect, keys, values, bit_range, order, storage):
    """Records the one sort of RECORDING_CALLS that takes what the caller has, on ``sorter`` (anything with the ``cmd_*``
    methods), the arguments in the calls' own order.  ``key_bits``: 32 or 64; ``offsets`` (with ``segment_count``), ``indirect``
    (the count tensor), ``keys``, ``values`` and ``storage``: objects with a ``data_ptr()``, handed over at byte offset 0;
    ``bit_range``: (begin_bit, end_bit); ``order``: the order word.  ``None`` selects the call without that argument; a
    combination no row has is a TypeError.  Every argument is positional: the torch front ends call this once per sort, and
    keywords cost them more than the rest of the function."""
    takes = (key_bits, offsets is not None, indirect is not None, values is not None, bit_range is not None, order is not None)
    recorder = _RECORDERS.get(takes)
    if recorder is None:
        raise TypeError(f"no recording call takes (key bits, offsets, indirect, values, bit range, order) = {takes}")
    recorder(sorter, stream, count, offsets, segment_count, indirect, keys, values, bit_range, order, storage)


_ORDERED_RECORDERS = {_takes(*call.facts)[1:4]: _recorder(call) for call in ORDERED_SORT_CALLS}


_RANGE_RECORDERS = {_takes(*call.facts)[2:4]: _recorder(call) for call in RANGE_SORT_CALLS}


def record_range_sort(sorter, stream, count, indirect, keys, values, bit_range, storage):
    """``record_sort`` for the rows of RANGE_SORT_CALLS: records the one range sort that takes what the caller has.
    ``bit_range``: (begin_bit, end_bit), always handed on; ``indirect`` / ``values``: ``None`` selects the call without."""
    _RANGE_RECORDERS[(indirect is not None, values is not None)](sorter, stream, count, None, None, indirect, keys, values,
                                                                  bit_range, None, storage)


def record_ordered_sort(sorter, stream, count, offsets, segment_count, indirect, keys, values, order, storage):
    """``record_sort`` for the rows of ORDERED_SORT_CALLS: records the one ordered sort of uint32 keys that takes what the caller
    has.  ``order``: the order word, always handed on; ``offsets`` / ``indirect`` / ``values``: ``None`` selects the call without
    that argument; offsets together with a count is a TypeError, as no row takes both."""
    takes = (offsets is not None, indirect is not None, values is not None)
    recorder = _ORDERED_RECORDERS.get(takes)
    if recorder is None:
        raise TypeError(f"no ordered recording call takes (offsets, indirect, values) = {takes}")
    recorder(sorter, stream, count, offsets, segment_count, indirect, keys, values, None, order, storage)


# the order word of vrdxHipCmdSort64Ordered* and vrdxHipCmdSortSegmented64Ordered* (include/vk_radix_sort.h): one key type,
# ORDER_DESCENDING or-ed in or not
KEY_UINT64 = 0
KEY_INT64 = 1
KEY_FLOAT64 = 2
ORDER_DESCENDING = 0x100
KEY_ORDERS = {"uint64": KEY_UINT64, "int64": KEY_INT64, "float64": KEY_FLOAT64}


def order_word(order: str, descending: bool = False) -> int:
    """The order word for ``order`` in ``KEY_ORDERS`` (``"uint64"``, ``"int64"``, ``"float64"``) and a direction."""
    if not isinstance(order, str):
        raise TypeError(f"order must be one of {', '.join(map(repr, KEY_ORDERS))}, got {type(order).__name__}")
    if order not in KEY_ORDERS:
        raise ValueError(f"order must be one of {', '.join(map(repr, KEY_ORDERS))}, got {order!r}")
    return KEY_ORDERS[order] | (ORDER_DESCENDING if descending else 0)



# the key types of vrdxHipCmdOrderedSort* (include/vk_radix_sort.h); the direction bit is ORDER_DESCENDING
KEY32_UINT32 = 0
KEY32_INT32 = 1
KEY32_FLOAT32 = 2
KEY32_ORDERS = {"uint32": KEY32_UINT32, "int32": KEY32_INT32, "float32": KEY32_FLOAT32}


def order_word32(order: str, descending: bool = False) -> int:
    """The order word for ``order`` in ``KEY32_ORDERS`` (``"uint32"``, ``"int32"``, ``"float32"``) and a direction."""
    if not isinstance(order, str):
        raise TypeError(f"order must be one of {', '.join(map(repr, KEY32_ORDERS))}, got {type(order).__name__}")
    if order not in KEY32_ORDERS:
        raise ValueError(f"order must be one of {', '.join(map(repr, KEY32_ORDERS))}, got {order!r}")
    return KEY32_ORDERS[order] | (ORDER_DESCENDING if descending else 0)


# bits of vrdxHipReadSorterStatus (include/vk_radix_sort.h)
STATUS_LOOKBACK_GAVE_UP = 0x00000001
STATUS_RANK_ORDER = 0x00000002
STATUS_SEGMENTS_INVALID = 0x00000004
STATUS_COUNT_CLAMPED = 0x40000000
STATUS_ENQUEUE_REFUSED = 0x80000000

# VRDX_HIP_PLAN_* (include/vk_radix_sort.h)
PLAN_NAMES = {0: "none", 1: "one-workgroup", 2: "four-passes", 3: "hybrid-8", 4: "hybrid-9", 5: "msd"}

# VRDX_HIP_VERDICT_* (include/vk_radix_sort.h): what the DEVICE made of the plan of the last sort on a storage
VERDICT_NONE = 0
VERDICT_HYBRID8_RUNS = 1
VERDICT_HYBRID8_DECLINED = 2
VERDICT_MSD_RUNS = 3
VERDICT_MSD_SORTED = 4


class VrdxError(RuntimeError):
    """A vrdx* call returned a VkResult other than VK_SUCCESS."""

    def __init__(self, what: str, result: int):
        super().__init__(f"{what} failed with VkResult {result}")
        self.result = result


class VrdxSorterCreateInfo(ctypes.Structure):
    # src/vk_radix_sort.h.in:18-22
    _fields_ = [("physicalDevice", ctypes.c_void_p), ("device", ctypes.c_void_p),
                ("pipelineCache", ctypes.c_void_p)]


class VrdxSorterStorageRequirements(ctypes.Structure):
    # src/vk_radix_sort.h.in:28-31
    _fields_ = [("size", ctypes.c_uint64), ("usage", ctypes.c_uint32)]


class VrdxHipPlanInfo(ctypes.Structure):
    # include/vk_radix_sort.h
    _fields_ = [("plan", ctypes.c_uint32), ("bits", ctypes.c_uint32), ("bytesPerElement", ctypes.c_uint32),
                ("fallbackBytesPerElement", ctypes.c_uint32), ("launches", ctypes.c_uint32)]

    @property
    def name(self) -> str:
        return PLAN_NAMES.get(int(self.plan), "?")


# VRDX_HIP_WIDE_VALUE_* (include/vk_radix_sort.h)
WIDE_VALUE_FORM_NAMES = {0: "none", 1: "one-workgroup", 2: "gather", 3: "two-sorts"}


class VrdxHipWideValuePlanInfo(ctypes.Structure):
    # include/vk_radix_sort.h
    _fields_ = [("form", ctypes.c_uint32), ("launches", ctypes.c_uint32), ("bytesPerElement", ctypes.c_uint32),
                ("innerPlan", ctypes.c_uint32), ("oneWorkgroupMax", ctypes.c_uint32), ("twoSortsFrom", ctypes.c_uint32)]

    @property
    def name(self) -> str:
        return WIDE_VALUE_FORM_NAMES.get(int(self.form), "?")


# VRDX_HIP_RANGE_SORT_* (include/vk_radix_sort.h)
RANGE_SORT_FORM_NAMES = {0: "none", 1: "one-workgroup", 2: "whole-key", 3: "chunked"}


class VrdxHipRangeSortPlanInfo(ctypes.Structure):
    # include/vk_radix_sort.h
    _fields_ = [("form", ctypes.c_uint32), ("chunks", ctypes.c_uint32), ("keysPerChunk", ctypes.c_uint32),
                ("digits", ctypes.c_uint32), ("launches", ctypes.c_uint32), ("bytesPerElementPerPass", ctypes.c_uint32),
                ("bytesPerElementCopyBack", ctypes.c_uint32)]

    @property
    def name(self) -> str:
        return RANGE_SORT_FORM_NAMES.get(int(self.form), "?")


# VRDX_HIP_BALANCED_* (include/vk_radix_sort_balanced.h)
BALANCED_FORM_NAMES = {0: "none", 1: "twin", 2: "balanced"}


class VrdxHipBalancedSegmentedPlanInfo(ctypes.Structure):
    # include/vk_radix_sort_balanced.h
    _fields_ = [("form", ctypes.c_uint32), ("launches", ctypes.c_uint32), ("spreadFrom", ctypes.c_uint32),
                ("spreadShares", ctypes.c_uint32), ("spreadCap", ctypes.c_uint32), ("pieceCap", ctypes.c_uint32),
                ("minPieceKeys", ctypes.c_uint32)]

    @property
    def name(self) -> str:
        return BALANCED_FORM_NAMES.get(int(self.form), "?")


class VrdxHipBalancedSplitInfo(ctypes.Structure):
    # include/vk_radix_sort_balanced.h
    _fields_ = [("listedSegments", ctypes.c_uint32), ("spreadSegments", ctypes.c_uint32), ("pieces", ctypes.c_uint32),
                ("pieceKeys", ctypes.c_uint32)]


def in_tree_library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvrdx_hip.so")


def library_path() -> str:
    """The in-tree libvrdx_hip.so.  VRDX_LIBRARY names another BUILD of the same library instead (the -DVRDX_TESTING
    build of two tests, a tuning variant of tools/); it is never a fallback: a missing file is an error either way,
    and ``load_library`` says on stderr that the override is active and refuses a library of another version."""
    override = os.environ.get("VRDX_LIBRARY")
    if override:
        return os.path.abspath(override)
    return in_tree_library_path()


_LIB: Optional[ctypes.CDLL] = None


def load_library() -> ctypes.CDLL:
    """Loads libvrdx_hip.so.  There is deliberately no fallback of any kind."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `make -C vulkan_radix_sort_amd/csrc` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    if path != in_tree_library_path():
        # A stale VRDX_LIBRARY (left behind by a tuning script, or the test build with its injection hooks) silently
        # changes what production code runs: say so, and insist on the same version and ABI.
        import sys
        missing = [name for name in EXPORTED_SYMBOLS + BALANCED_EXPORTED_SYMBOLS if not hasattr(lib, name)]
        if missing:
            raise ImportError(f"VRDX_LIBRARY={path} does not export {', '.join(missing)}: not a build of this library")
        lib.vrdxHipVersionString.restype = ctypes.c_char_p
        theirs = lib.vrdxHipVersionString().decode()
        if os.path.exists(in_tree_library_path()):
            own = ctypes.CDLL(in_tree_library_path())
            own.vrdxHipVersionString.restype = ctypes.c_char_p
            ours = own.vrdxHipVersionString().decode()
            if theirs.split()[:2] != ours.split()[:2]:
                raise ImportError(f"VRDX_LIBRARY={path} is '{theirs}', the in-tree library is '{ours}': version mismatch")
        print(f"vulkan_radix_sort_amd: VRDX_LIBRARY override active, loaded {path} ({theirs})", file=sys.stderr)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.vrdxCreateSorter.restype = ctypes.c_int32
    lib.vrdxCreateSorter.argtypes = [ctypes.POINTER(VrdxSorterCreateInfo), ctypes.POINTER(vp)]
    lib.vrdxDestroySorter.restype = None
    lib.vrdxDestroySorter.argtypes = [vp]
    for name in ("vrdxGetSorterStorageRequirements", "vrdxGetSorterKeyValueStorageRequirements",
                 "vrdxHipGetSorter64StorageRequirements", "vrdxHipGetSorter64KeyValueStorageRequirements",
                 "vrdxHipGetSorterWideValueStorageRequirements"):
        fn = getattr(lib, name)
        fn.restype = None
        fn.argtypes = [vp, u32, ctypes.POINTER(VrdxSorterStorageRequirements)]
    for call in RECORDING_CALLS + ORDERED_SORT_CALLS + WIDE_VALUE_CALLS + WIDE_VALUE_SEGMENTED_CALLS + RANGE_SORT_CALLS + \
        BALANCED_SEGMENTED_CALLS:
        fn = getattr(lib, call.c_name)
        fn.restype = None
        fn.argtypes = call.argtypes
    lib.vrdxHipDescribeWideValueSortPlan.restype = None
    lib.vrdxHipDescribeWideValueSortPlan.argtypes = [vp, u32, ctypes.POINTER(VrdxHipWideValuePlanInfo)]
    lib.vrdxHipDescribeOrderedSortPlan.restype = None
    lib.vrdxHipDescribeOrderedSortPlan.argtypes = [vp, u32, ctypes.c_int, u32, ctypes.POINTER(VrdxHipPlanInfo)]
    lib.vrdxHipDescribeRangeSortPlan.restype = None
    lib.vrdxHipDescribeRangeSortPlan.argtypes = [vp, u32, ctypes.c_int, u32, u32, ctypes.POINTER(VrdxHipRangeSortPlanInfo)]
    lib.vrdxHipDescribeBalancedSegmentedPlan.restype = None
    lib.vrdxHipDescribeBalancedSegmentedPlan.argtypes = [vp, u32, u32, ctypes.c_int, ctypes.POINTER(VrdxHipBalancedSegmentedPlanInfo)]
    lib.vrdxHipReadBalancedSplit.restype = ctypes.c_int32
    lib.vrdxHipReadBalancedSplit.argtypes = [vp, vp, vp, u64, u32, ctypes.POINTER(VrdxHipBalancedSplitInfo)]
    lib.vrdxHipDescribeSortBitsPlan.restype = None
    lib.vrdxHipDescribeSortBitsPlan.argtypes = [vp, u32, ctypes.c_int, u32, u32, ctypes.POINTER(VrdxHipPlanInfo)]
    lib.vrdxHipCreateQueryPool.restype = ctypes.c_int32
    lib.vrdxHipCreateQueryPool.argtypes = [u32, ctypes.POINTER(vp)]
    lib.vrdxHipDestroyQueryPool.restype = None
    lib.vrdxHipDestroyQueryPool.argtypes = [vp]
    lib.vrdxHipGetQueryPoolResults.restype = ctypes.c_int32
    lib.vrdxHipGetQueryPoolResults.argtypes = [vp, u32, u32, ctypes.POINTER(u64)]
    lib.vrdxHipReadStatus.restype = u32
    lib.vrdxHipReadStatus.argtypes = [vp, vp, u64]
    lib.vrdxHipReadSorterStatus.restype = u32
    lib.vrdxHipReadSorterStatus.argtypes = [vp, vp]
    lib.vrdxHipRecheck.restype = ctypes.c_int32
    lib.vrdxHipRecheck.argtypes = [vp]
    lib.vrdxHipEventOverheadNs.restype = u64
    lib.vrdxHipEventOverheadNs.argtypes = [vp]
    lib.vrdxHipDescribePlan.restype = None
    lib.vrdxHipDescribePlan.argtypes = [vp, u32, ctypes.c_int, ctypes.POINTER(VrdxHipPlanInfo)]
    lib.vrdxHipReadPlanVerdict.restype = u32
    lib.vrdxHipReadPlanVerdict.argtypes = [vp, vp, u64]
    lib.vrdxHipReadPlanCounters.restype = ctypes.c_int32
    lib.vrdxHipReadPlanCounters.argtypes = [vp, vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.vrdxHipVersionString.restype = ctypes.c_char_p
    lib.vrdxHipVersionString.argtypes = []
    _LIB = lib
    return lib


def version_string() -> str:
    return load_library().vrdxHipVersionString().decode()


def event_overhead_ns(command_buffer) -> int:
    """``vrdxHipEventOverheadNs``: what a pair of event records adds to the kernel between them on this stream (ns),
    measured against a kernel that times itself with the device's wall clock.  Raises if the calibration failed."""
    ns = int(load_library().vrdxHipEventOverheadNs(_handle(command_buffer)))
    if ns == 0xFFFFFFFFFFFFFFFF:
        raise VrdxError("vrdxHipEventOverheadNs", -4)
    return ns


def _handle(x) -> Optional[int]:
    if x is None:
        return None
    return int(x) or None


class QueryPool:
    """HIP stand-in for a VkQueryPool of timestamp queries (hipEvent_t per slot)."""

    def __init__(self, count: int = 15):
        self._lib = load_library()
        h = ctypes.c_void_p()
        r = self._lib.vrdxHipCreateQueryPool(count, ctypes.byref(h))
        if r != VK_SUCCESS:
            raise VrdxError("vrdxHipCreateQueryPool", r)
        self.handle = h.value
        self.count = count

    def results_ns(self, first: int = 0, count: Optional[int] = None):
        """vkGetQueryPoolResults analogue: ns since slot `first` for each slot (stream must be done)."""
        count = self.count - first if count is None else count
        data = (ctypes.c_uint64 * count)()
        r = self._lib.vrdxHipGetQueryPoolResults(self.handle, first, count, data)
        if r != VK_SUCCESS:
            raise VrdxError("vrdxHipGetQueryPoolResults", r)
        return [int(x) for x in data]

    def destroy(self):
        if self.handle:
            self._lib.vrdxHipDestroyQueryPool(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Sorter:
    """VrdxSorter.  ``device`` is a HIP ordinal, or None for the current device."""

    def __init__(self, device: Optional[int] = None):
        self._lib = load_library()
        info = VrdxSorterCreateInfo()
        encoded = None if device is None else device + 1  # VRDX_HIP_DEVICE(ordinal)
        info.physicalDevice = encoded
        info.device = encoded
        info.pipelineCache = None
        h = ctypes.c_void_p()
        r = self._lib.vrdxCreateSorter(ctypes.byref(info), ctypes.byref(h))
        if r != VK_SUCCESS:
            raise VrdxError("vrdxCreateSorter", r)
        self.handle = h.value

    # -- lifetime ---------------------------------------------------------------------------
    def destroy(self):
        if getattr(self, "handle", None):
            self._lib.vrdxDestroySorter(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- storage ----------------------------------------------------------------------------
    def storage_requirements(self, max_element_count: int) -> VrdxSorterStorageRequirements:
        req = VrdxSorterStorageRequirements()
        self._lib.vrdxGetSorterStorageRequirements(self.handle, max_element_count, ctypes.byref(req))
        return req

    def key_value_storage_requirements(self, max_element_count: int) -> VrdxSorterStorageRequirements:
        req = VrdxSorterStorageRequirements()
        self._lib.vrdxGetSorterKeyValueStorageRequirements(self.handle, max_element_count, ctypes.byref(req))
        return req

    def storage_requirements64(self, max_element_count: int, key_value: bool = False) -> VrdxSorterStorageRequirements:
        """``vrdxHipGetSorter64[KeyValue]StorageRequirements``: the storage of a sort of uint64 keys."""
        req = VrdxSorterStorageRequirements()
        fn = (self._lib.vrdxHipGetSorter64KeyValueStorageRequirements if key_value
              else self._lib.vrdxHipGetSorter64StorageRequirements)
        fn(self.handle, max_element_count, ctypes.byref(req))
        return req

    def wide_value_storage_requirements(self, max_element_count: int) -> VrdxSorterStorageRequirements:
        """``vrdxHipGetSorterWideValueStorageRequirements``: the storage of a sort of uint32 keys with 8-byte values."""
        req = VrdxSorterStorageRequirements()
        self._lib.vrdxHipGetSorterWideValueStorageRequirements(self.handle, max_element_count, ctypes.byref(req))
        return req

    # -- recording: the cmd_* methods, one per row of RECORDING_CALLS, are attached below the class ------------------

    # -- diagnostics ------------------------------------------------------------------------
    def read_status(self, command_buffer, storage, storage_offset=0) -> int:
        return int(self._lib.vrdxHipReadStatus(_handle(command_buffer), _handle(storage), storage_offset))

    def read_sorter_status(self, command_buffer) -> int:
        """OR of the failure bits of every sort recorded with this sorter since the previous call,
        whatever storage they used (``vrdxHipReadSorterStatus``); synchronises the stream."""
        return int(self._lib.vrdxHipReadSorterStatus(self.handle, _handle(command_buffer)))


    def describe_plan(self, element_count: int, key_value: bool) -> VrdxHipPlanInfo:
        """``vrdxHipDescribePlan``: the plan this sorter records for that many elements and the HBM bytes per element it
        moves (what a whole-sort roofline figure is priced with)."""
        info = VrdxHipPlanInfo()
        self._lib.vrdxHipDescribePlan(self.handle, element_count, 1 if key_value else 0, ctypes.byref(info))
        return info

    def describe_sort_bits_plan(self, element_count: int, key_value: bool, begin_bit: int, end_bit: int) -> VrdxHipPlanInfo:
        """``vrdxHipDescribeSortBitsPlan``: the plan ``cmd_sort_bits*`` records for that many elements and that range."""
        info = VrdxHipPlanInfo()
        self._lib.vrdxHipDescribeSortBitsPlan(self.handle, element_count, 1 if key_value else 0, begin_bit, end_bit,
                                              ctypes.byref(info))
        return info

    def describe_range_sort_plan(self, element_count: int, key_value: bool, begin_bit: int,
                                 end_bit: int) -> VrdxHipRangeSortPlanInfo:
        """``vrdxHipDescribeRangeSortPlan``: the form ``cmd_range_sort*`` records for that many elements and that range
        (``.name``), its chunks, digits and launches, and the HBM bytes per element of an active pass and of the copy back."""
        info = VrdxHipRangeSortPlanInfo()
        self._lib.vrdxHipDescribeRangeSortPlan(self.handle, element_count, 1 if key_value else 0, begin_bit, end_bit,
                                               ctypes.byref(info))
        return info

    def describe_balanced_segmented_plan(self, max_element_count: int, segment_count: int,
                                         key_value: bool) -> VrdxHipBalancedSegmentedPlanInfo:
        """``vrdxHipDescribeBalancedSegmentedPlan``: the form ``cmd_balanced_sort_segmented*`` records under that bound
        (``.name``), its launches, the two constants of the rule, the caps of spread segments and pieces, and the smallest
        piece length."""
        info = VrdxHipBalancedSegmentedPlanInfo()
        self._lib.vrdxHipDescribeBalancedSegmentedPlan(self.handle, max_element_count, segment_count, 1 if key_value else 0,
                                                       ctypes.byref(info))
        return info

    def read_balanced_split(self, command_buffer, storage, max_element_count: int, storage_offset=0) -> VrdxHipBalancedSplitInfo:
        """``vrdxHipReadBalancedSplit``: what the device decided in the last ``cmd_balanced_sort_segmented*`` on this storage,
        recorded with this ``max_element_count``: listed segments, spread segments, pieces, piece length.  Synchronises the
        stream."""
        info = VrdxHipBalancedSplitInfo()
        r = self._lib.vrdxHipReadBalancedSplit(_handle(command_buffer), self.handle, _handle(storage), storage_offset,
                                               max_element_count, ctypes.byref(info))
        if r != VK_SUCCESS:
            raise VrdxError("vrdxHipReadBalancedSplit", r)
        return info

    def describe_ordered_sort_plan(self, element_count: int, key_value: bool, order: int) -> VrdxHipPlanInfo:
        """``vrdxHipDescribeOrderedSortPlan``: the plan ``cmd_ordered_sort*`` records for that many elements and that order word
        (beyond one workgroup: ``describe_plan``'s, plus two launches and 16 bytes per element)."""
        info = VrdxHipPlanInfo()
        self._lib.vrdxHipDescribeOrderedSortPlan(self.handle, element_count, 1 if key_value else 0, order, ctypes.byref(info))
        return info

    def describe_wide_value_sort_plan(self, element_count: int) -> VrdxHipWideValuePlanInfo:
        """``vrdxHipDescribeWideValueSortPlan``: the form ``cmd_wide_value_sort*`` records for that many elements (``.name``),
        its launches and HBM bytes per element, and the two sizes at which the form changes."""
        info = VrdxHipWideValuePlanInfo()
        self._lib.vrdxHipDescribeWideValueSortPlan(self.handle, element_count, ctypes.byref(info))
        return info

    def read_plan_verdict(self, command_buffer, storage, storage_offset=0) -> int:
        """``vrdxHipReadPlanVerdict``: what the device made of the plan of the last sort on this storage (``VERDICT_*``):
        ``describe_plan`` is the host's intention, this is what ran.  Synchronises the stream."""
        return int(self._lib.vrdxHipReadPlanVerdict(_handle(command_buffer), _handle(storage), storage_offset))

    def plan_taken(self, command_buffer, storage, storage_offset=0) -> bool:
        """True when the two-trip plan recorded for the last sort on this storage (hybrid-8 or msd) actually ran."""
        return self.read_plan_verdict(command_buffer, storage, storage_offset) in (
            VERDICT_HYBRID8_RUNS, VERDICT_MSD_RUNS, VERDICT_MSD_SORTED)

    def read_plan_counters(self, command_buffer):
        """``vrdxHipReadPlanCounters``: (sorts recorded with the MSD plan in front, how many of them the device turned
        down) since the sorter was created.  Synchronises the stream."""
        recorded, declined = ctypes.c_uint32(0), ctypes.c_uint32(0)
        r = self._lib.vrdxHipReadPlanCounters(self.handle, _handle(command_buffer), ctypes.byref(recorded),
                                              ctypes.byref(declined))
        if r != VK_SUCCESS:
            raise VrdxError("vrdxHipReadPlanCounters", r)
        return int(recorded.value), int(declined.value)

    def recheck(self) -> None:
        """``vrdxHipRecheck``: repeats the device check behind the one-atomic ranking and falls back to the ballot
        ranking for later sorts if it fails (synchronous, ~1 ms)."""
        r = self._lib.vrdxHipRecheck(self.handle)
        if r != VK_SUCCESS:
            raise VrdxError("vrdxHipRecheck", r)


def _pool(p) -> Optional[int]:
    if p is None:
        return None
    if isinstance(p, QueryPool):
        return p.handle
    return _handle(p)


def _recording_method(call: RecordingCall):
    """``Sorter.<call.method>``, compiled from source text built from the row, so that a call costs what a hand-written method
    costs: pointer-like arguments go through ``_handle``, the query pool through ``_pool``, everything else as it comes,
    ``self.handle`` second."""
    names = [name for name, _ in call.parameters]
    forwarded = ["_pool(query_pool)" if name == "query_pool" else f"_handle({name})" if ctype is ctypes.c_void_p else name
                 for name, ctype in call.parameters]
    forwarded.insert(1, "self.handle")
    method = _compiled(call.method, f"def {call.method}(self, {', '.join(names[:-2])}, query_pool=None, query=0):\n"
                                    f"    self._lib.{call.c_name}({', '.join(forwarded)})\n", _handle=_handle, _pool=_pool)
    method.__qualname__ = f"Sorter.{call.method}"
    method.__doc__ = f"``{call.c_name}``: {call.doc}"
    return method


for _call in RECORDING_CALLS + ORDERED_SORT_CALLS + WIDE_VALUE_CALLS + WIDE_VALUE_SEGMENTED_CALLS + RANGE_SORT_CALLS + \
        BALANCED_SEGMENTED_CALLS:
    setattr(Sorter, _call.method, _recording_method(_call))
