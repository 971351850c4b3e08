"""One guarded call of the balanced segmented sorts (the rows of vulkan_radix_sort_amd.api.BALANCED_SEGMENTED_CALLS) for
tests/test_balanced_segmented_gpu.py, through guarded_call.guarded_call itself: that function dispatches on RECORDING_CALLS
only, and the balanced calls take the arguments of vrdxHipCmdSortSegmented[KeyValue], name for name -- so the sorter it is
handed is one whose cmd_sort_segmented* methods ARE the cmd_balanced_sort_segmented* methods, and everything else (guard bytes
around keys, values and offsets, the poisoned storage between its bands, the status word) is checked as for every other
recording call."""
from guarded_call import (BAND_BYTE, GUARD_BYTE, POISON_BYTE, ballot_sorter, guarded_call, poisoned_storage, sorter,  # noqa: F401
                          to_device, to_host, torch_mod)
from vulkan_radix_sort_amd import api

_AS_BALANCED = {twin.method: balanced.method for twin in api.RECORDING_CALLS for balanced in api.BALANCED_SEGMENTED_CALLS
                if twin.facts == balanced.facts}
assert sorted(_AS_BALANCED) == ["cmd_sort_segmented", "cmd_sort_segmented_key_value"]


class AsBalanced:
    """`sorter` with vrdxHipCmdBalancedSortSegmented* where vrdxHipCmdSortSegmented* are asked for"""

    def __init__(self, sorter):
        self._sorter = sorter

    def __getattr__(self, name):
        return getattr(self._sorter, _AS_BALANCED.get(name, name))


def balanced_call(torch, sorter, keys, values, offsets, **kw):
    """guarded_call of the balanced segmented sort that takes what the caller hands in"""
    return guarded_call(torch, AsBalanced(sorter), keys, values, offsets=offsets, **kw)


def twin_call(torch, sorter, keys, values, offsets, **kw):
    """the same call of vrdxHipCmdSortSegmented[KeyValue]"""
    return guarded_call(torch, sorter, keys, values, offsets=offsets, **kw)
