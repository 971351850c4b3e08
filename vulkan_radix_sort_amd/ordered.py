"""Sorts of 32-bit keys in a key order: int32, float32, descending.

``sort_ordered(sorter, keys, order="float32")`` sorts a one-dimensional ``torch.float32`` tensor (or 4-byte integers holding
float32 bits) in IEEE-754 totalOrder, ``order="int32"`` sorts 4-byte integers as signed, ``order="uint32"`` as unsigned, and
``descending=True`` reverses any of the three -- stably in both directions, in place, on torch's current stream
(``vrdxHipCmdOrderedSort[KeyValue][Indirect]``).  ``sort_segments_ordered(sorter, keys, offsets, ...)`` does the same for every
segment ``keys[offsets[i]:offsets[i + 1]]`` (``vrdxHipCmdOrderedSortSegmented[KeyValue]``).  totalOrder is ``torch.sort``'s order
except that NaNs with the sign bit set come first instead of last and that -0.0 sorts in front of +0.0 instead of equal to it.
Up to 16384 keys, and in every segment, the order is applied between the kernels' loads and stores (a few percent at most); a
flat sort of more keys pays two streaming launches over the keys around the unordered sort.  Everything is checked on the host before anything is recorded, no data is read, so the
calls do not synchronise and can be captured into a ``torch.cuda.graph``.
"""
from __future__ import annotations

from . import _checks as check
from .api import Sorter, record_ordered_sort


def _storage(torch, sorter, storage, n, key_value, device):
    if storage is not None:
        check.check_storage(torch, storage, device, True)
    required = (sorter.key_value_storage_requirements(n) if key_value else sorter.storage_requirements(n)).size
    return check.storage_or_new(torch, storage, required, device)


def sort_ordered(sorter: Sorter, keys, values=None, storage=None, count=None, order="uint32", descending=False):
    """Sorts ``keys`` in place in the order ``order`` (``"uint32"``, ``"int32"`` or ``"float32"``; ``descending``: the reverse
    of it, equal keys still in input order); ``values``, 4-byte integers of the same length, travel with their keys.
    ``storage``: a uint8 tensor of at least ``sorter.[key_value_]storage_requirements(keys.numel())`` bytes on the keys' device
    whose address is a multiple of 16, allocated here when omitted.  ``count``: a one-element int32 / uint32 tensor on the keys'
    device; only the first min(count, keys.numel()) elements are sorted, the count is read on the device and must not be part
    of ``storage``.  Returns the storage used (one sort in flight per storage)."""
    import torch

    word = check.check_keys32(torch, keys, order, descending)
    device = keys.device
    if values is not None:
        check.check_values(torch, values, keys, "4-byte integers (int32 or uint32)", device)
    if count is not None:
        check.check_count(torch, count, "one element", device)
    n = check.key_count(keys)
    storage = _storage(torch, sorter, storage, n, values is not None, device)
    # (sorter, stream, count, offsets, segment count, indirect, keys, values, order, storage)
    record_ordered_sort(sorter, torch.cuda.current_stream(device).cuda_stream, n, None, None, count, keys, values, word, storage)
    return storage


def sort_segments_ordered(sorter: Sorter, keys, offsets, values=None, storage=None, order="uint32", descending=False):
    """Sorts ``keys[offsets[i]:offsets[i + 1]]`` for every ``i < offsets.numel() - 1`` in place in the order ``order``
    (``descending``: the reverse of it); ``offsets``: 4-byte integers on the keys' device, read on the device only; ``values``
    and ``storage`` as for ``sort_ordered``.  Offsets that decrease or end behind ``keys.numel()`` leave their segment alone
    and raise ``STATUS_SEGMENTS_INVALID``.  Returns the storage used."""
    import torch

    word = check.check_keys32(torch, keys, order, descending)
    device = keys.device
    check.check_offsets(torch, offsets, "4-byte integers (int32 or uint32)", device)
    if values is not None:
        check.check_values(torch, values, keys, "4-byte integers (int32 or uint32)", device)
    n = check.key_count(keys)
    storage = _storage(torch, sorter, storage, n, values is not None, device)
    record_ordered_sort(sorter, torch.cuda.current_stream(device).cuda_stream, n, offsets, offsets.numel() - 1, None, keys, values,
                        word, storage)
    return storage
