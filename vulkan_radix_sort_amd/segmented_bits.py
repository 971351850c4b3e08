"""Segmented sort of torch tensors by a bit range of the key.

``sort_segments_bits(sorter, keys, offsets, begin_bit, end_bit)`` sorts every segment ``keys[offsets[i]:offsets[i + 1]]`` on
its own, in place and stably, ascending by the field ``(key >> begin_bit) & (2**(end_bit - begin_bit) - 1)``: keys of equal
field keep their input order and every key comes back whole (``vrdxHipCmdSortSegmentedBits[KeyValue]``; CUB's
``DeviceSegmentedRadixSort`` with ``begin_bit`` / ``end_bit``).  ``values``, 4-byte integers of the same length, travel with
their keys.

``0 <= begin_bit <= end_bit <= 32``; an empty range leaves everything as it is, the range of all 32 bits is
``sort_segments``.  Segments may have any size: unlike ``sort_bits`` there is no count at which a range is refused.  A
segment of more than 16384 elements is sorted by one workgroup, so one huge segment is correct and slow.

The arguments are checked like those of ``sort_segments`` and the range like that of ``sort_bits``, on the host and before
anything is recorded -- types, dtypes, shapes, the range and the lengths first, then where the tensors live; the offsets'
values are never read, so the call does not synchronise and can be captured into a ``torch.cuda.graph``.  Offsets that decrease or end behind ``keys.numel()`` leave their segment alone and raise
``STATUS_SEGMENTS_INVALID``.
"""
from __future__ import annotations

from . import _checks as check
from .api import Sorter, record_sort


def sort_segments_bits(sorter: Sorter, keys, offsets, begin_bit, end_bit, values=None, storage=None):
    """Sorts ``keys[offsets[i]:offsets[i + 1]]`` for every ``i < offsets.numel() - 1`` in place by the bits
    [begin_bit, end_bit) of the keys (values, if given, travel with their keys).  ``storage``: a uint8 tensor of at least
    ``sorter.[key_value_]storage_requirements(keys.numel())`` bytes on the keys' device, allocated here when omitted.
    Returns the storage used (one sort in flight per storage)."""
    import torch

    check.check_bit_range(begin_bit, end_bit)
    check.check_tensor(torch, "keys", keys, check.integer_dtypes(torch)[0],
                       "4-byte integers (int32 or uint32, ordered as uint32 fields)")
    check.check_offsets(torch, offsets, "4-byte integers (int32 or uint32)")
    if values is not None:
        check.check_values(torch, values, keys, "4-byte integers (int32 or uint32)")
    n = check.key_count(keys)
    if storage is not None:
        check.check_storage(torch, storage)
    # where they live
    check.check_device("keys", keys)
    device = keys.device
    for name, t in (("offsets", offsets), ("values", values), ("storage", storage)):
        if t is not None:
            check.check_device(name, t, device)
    required = (sorter.key_value_storage_requirements(n) if values is not None else sorter.storage_requirements(n)).size
    storage = check.storage_or_new(torch, storage, required, device)
    # (sorter, key bits, stream, count, offsets, segment count, indirect, keys, values, bit range, order, storage)
    record_sort(sorter, 32, torch.cuda.current_stream(device).cuda_stream, n, offsets, offsets.numel() - 1, None, keys, values,
                (begin_bit, end_bit), None, storage)
    return storage
