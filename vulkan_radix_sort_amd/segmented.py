"""Segmented sort of torch tensors: many independent arrays, packed back to back, in one recorded call.

``sort_segments(sorter, keys, offsets)`` sorts every segment ``keys[offsets[i]:offsets[i + 1]]`` on its own, ascending as
uint32 and stably, in place, on torch's current stream (``vrdxHipCmdSortSegmented[KeyValue]``).  The offsets stay on the
device: this module checks dtypes, shapes and devices on the host and never reads the offsets' values, so the call does not
synchronise and can be captured into a ``torch.cuda.graph``.  Offsets that decrease or end behind ``keys.numel()`` leave
their segment alone and raise ``STATUS_SEGMENTS_INVALID`` (``Sorter.read_status`` / ``Sorter.read_sorter_status``).
"""
from __future__ import annotations

from . import _checks as check
from ._checks import MAX_ELEMENTS  # noqa: F401 -- importable from here as it always was
from .api import Sorter, record_sort


def sort_segments(sorter: Sorter, keys, offsets, values=None, storage=None):
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
    # (sorter, key bits, stream, count, offsets, segment count, indirect, keys, values, bit range, order, storage)
    record_sort(sorter, 32, torch.cuda.current_stream(device).cuda_stream, n, offsets, offsets.numel() - 1, None, keys, values,
                None, None, storage)
    return storage
