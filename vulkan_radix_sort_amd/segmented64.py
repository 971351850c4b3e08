"""Segmented sort of 64-bit keys held in torch tensors: many independent arrays, packed back to back, in one recorded call.

``sort_segments64(sorter, keys, offsets)`` sorts every segment ``keys[offsets[i]:offsets[i + 1]]`` of a one-dimensional
``torch.int64`` (or ``torch.uint64``) tensor on its own, ascending as uint64 and stably, in place, on torch's current stream
(``vrdxHipCmdSortSegmented64[KeyValue]``); ``values``, 4-byte integers of the same length, travel with their keys.  An
``int64`` tensor with negative entries ends with them behind the others inside each segment, unless an order is asked for:
``order="int64"``, ``order="float64"`` (a ``torch.float64`` tensor, IEEE-754 totalOrder) and ``descending=True`` are those
of ``sort64`` (``vrdxHipCmdSortSegmented64Ordered[KeyValue]``).  As with ``sort_segments`` the
offsets stay on the device and only dtypes, shapes and devices are checked on the host, so the call does not synchronise
and can be captured into a ``torch.cuda.graph``; offsets that decrease or end behind ``keys.numel()`` leave their segment
alone and raise ``STATUS_SEGMENTS_INVALID``.
"""
from __future__ import annotations

from . import _checks as check
from .api import Sorter, record_sort


def sort_segments64(sorter: Sorter, keys, offsets, values=None, storage=None, order=None, descending=False):
    """Sorts ``keys[offsets[i]:offsets[i + 1]]`` for every ``i < offsets.numel() - 1`` in place as uint64 (values, if given,
    travel with their keys).  ``storage``: a uint8 tensor of at least
    ``sorter.storage_requirements64(keys.numel(), key_value=values is not None)`` bytes on the keys' device whose address is
    a multiple of 16, allocated here when omitted.  ``order``, ``descending``: as for ``sort64``; ``order=None`` with
    ``descending=False`` is the unsigned ascending sort.  Returns the storage used (one sort in flight per storage)."""
    import torch

    word = check.check_keys(torch, keys, order, descending)
    device = keys.device
    check.check_offsets(torch, offsets, "4-byte integers (int32 or uint32)", device)
    if values is not None:
        check.check_values(torch, values, keys, "4-byte integers (int32 or uint32)", device)
    n = check.key_count(keys)
    if storage is not None:
        check.check_storage(torch, storage, device, True)
    required = sorter.storage_requirements64(n, key_value=values is not None).size
    storage = check.storage_or_new(torch, storage, required, device)
    # (sorter, key bits, stream, count, offsets, segment count, indirect, keys, values, bit range, order, storage)
    record_sort(sorter, 64, torch.cuda.current_stream(device).cuda_stream, n, offsets, offsets.numel() - 1, None, keys, values,
                None, word, storage)
    return storage
