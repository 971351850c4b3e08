"""One guarded call of the range sorts at every size (the rows of vulkan_radix_sort_amd.api.RANGE_SORT_CALLS) for
tests/test_range_sort_gpu.py, through guarded_call.guarded_call itself: that function dispatches on RECORDING_CALLS only, and the
range sorts take the arguments of vrdxHipCmdSortBits*, name for name -- so the sorter it is handed is one whose
cmd_sort_bits* methods ARE the cmd_range_sort* methods, and everything else (guard bytes around keys, values and count word,
the poisoned storage between its bands, the status word) is checked as for every other recording call."""
from guarded_call import (BAND_BYTE, GUARD_BYTE, POISON_BYTE, ballot_sorter, guarded_call, poisoned_storage, sorter,  # noqa: F401
                          to_device, to_host, torch_mod)
from vulkan_radix_sort_amd import api

_AS_RANGE_SORT = {bits.method: ranged.method for bits in api.RECORDING_CALLS for ranged in api.RANGE_SORT_CALLS
                  if bits.facts == ranged.facts}
assert sorted(_AS_RANGE_SORT) == ["cmd_sort_bits", "cmd_sort_bits_indirect", "cmd_sort_bits_key_value",
                                  "cmd_sort_bits_key_value_indirect"]


class AsRangeSort:
    """`sorter` with vrdxHipCmdRangeSort* where vrdxHipCmdSortBits* are asked for"""

    def __init__(self, sorter):
        self._sorter = sorter

    def __getattr__(self, name):
        return getattr(self._sorter, _AS_RANGE_SORT.get(name, name))


def range_call(torch, sorter, keys, values, begin, end, **kw):
    """guarded_call of the range sort that takes what the caller hands in; `recorded` follows the range alone (no size is
    refused)"""
    return guarded_call(torch, AsRangeSort(sorter), keys, values, bit_range=(begin, end), **kw)
