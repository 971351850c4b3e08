"""Segmented sort of 32-bit keys held in torch tensors that spreads huge segments over every compute unit.

``sort_segments_balanced(sorter, keys, offsets)`` is ``sort_segments`` with one difference on the device: a segment that is
long (more than 65536 keys) and longer than three times its share of the chip is cut into pieces that many workgroups sort
together (``vrdxHipCmdBalancedSortSegmented[KeyValue]``).  The result is the same bit for bit: every segment
``keys[offsets[i]:offsets[i + 1]]`` ascending as uint32 and stable, ``values`` travelling with their keys.  Use it where a few
segments may be very large; where the large segments always fill the chip ``sort_segments`` records 14 launches fewer.

The checks are those of ``sort_segments``, in its order.  No data is read on the host -- which segments are spread is decided
on the device -- so the call does not synchronise and can be captured into a ``torch.cuda.graph``; it runs on torch's current
stream.  ``sorter.read_balanced_split(stream, storage, keys.numel())`` says afterwards what the device decided.
"""
from __future__ import annotations

from . import _checks as check
from .api import BALANCED_SEGMENTED_CALLS, Sorter, _recorder

_RECORDERS = {call.facts[3]: _recorder(call) for call in BALANCED_SEGMENTED_CALLS}   # by key+value or not


def sort_segments_balanced(sorter: Sorter, keys, offsets, values=None, storage=None):
    """Sorts ``keys[offsets[i]:offsets[i + 1]]`` for every ``i < offsets.numel() - 1`` in place (values, if given, travel
    with their keys).  ``storage``: a uint8 tensor of at least ``sorter.[key_value_]storage_requirements(keys.numel())``
    bytes on the keys' device, allocated here when omitted.  Returns the storage used (one sort in flight per storage)."""
    import torch

    what = "4-byte integers (int32 or uint32, sorted as uint32)"
    check.check_tensor(torch, "keys", keys, check.integer_dtypes(torch)[0], what, gpu=True)
    device = keys.device
    check.check_offsets(torch, offsets, what, device)
    if values is not None:
        check.check_values(torch, values, keys, what, device)
    n = check.key_count(keys)
    required = (sorter.key_value_storage_requirements(n) if values is not None else sorter.storage_requirements(n)).size
    if storage is not None:
        check.check_storage(torch, storage, device)
    storage = check.storage_or_new(torch, storage, required, device)
    # (sorter, stream, count, offsets, segment count, indirect, keys, values, bit range, order, storage)
    _RECORDERS[values is not None](sorter, torch.cuda.current_stream(device).cuda_stream, n, offsets, offsets.numel() - 1, None,
                                   keys, values, None, None, storage)
    return storage
