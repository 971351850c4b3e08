"""Sort of 32-bit keys with 64-bit values held in torch tensors.

``sort_key_value64(sorter, keys, values)`` sorts a one-dimensional ``torch.int32`` (or ``torch.uint32``) tensor ascending as
uint32 and stably, in place, on torch's current stream (``vrdxHipCmdWideValueSort``); ``values``, a ``torch.int64`` or
``torch.float64`` tensor of the same length, travel with their keys as 8 opaque bytes each -- an index as every torch index
tensor holds it, a float64, a pointer, a pair of uint32 ids.  Everything is checked on the host before anything is recorded, no
data is read, so the call does not synchronise and can be captured into a ``torch.cuda.graph``.

``sort_key_value64(sorter, keys, values, count=t)`` sorts only the first ``t`` elements, ``t`` a one-element ``int32`` /
``uint32`` tensor on the keys' device that is read on the GPU when the sort runs (``vrdxHipCmdWideValueSortIndirect``);
``keys.numel()`` is the bound -- a count beyond it is clamped to it -- and sizes the storage; elements from the count on are
left alone.

``sort_segments_key_value64(sorter, keys, offsets, values)`` sorts every segment ``keys[offsets[i]:offsets[i + 1]]`` on its
own, ascending as uint32 and stably, in place, the 8-byte ``values`` travelling with their keys
(``vrdxHipCmdWideValueSortSegmented``): per-row argsort with int64 indices, per-expert token lists.  As with ``sort_segments``
the offsets stay on the device; offsets that decrease or end behind ``keys.numel()`` leave their segment alone and raise
``STATUS_SEGMENTS_INVALID``.
"""
from __future__ import annotations

from . import _checks as check
from .api import Sorter


def sort_key_value64(sorter: Sorter, keys, values, count=None, storage=None):
    """Sorts ``keys`` in place as uint32, ``values`` (8 bytes each) travelling with their keys.  ``count``: a one-element
    int32 / uint32 tensor on the keys' device; only the first min(count, keys.numel()) elements are sorted, the count is read
    on the device and must not be part of ``storage``.  ``storage``: a uint8 tensor of at least
    ``sorter.wide_value_storage_requirements(keys.numel())`` bytes on the keys' device whose address is a multiple of 16,
    allocated here when omitted.  Returns the storage used (one sort in flight per storage)."""
    import torch

    check.check_tensor(torch, "keys", keys, check.integer_dtypes(torch)[0], "4-byte integers (int32 or uint32, sorted as uint32)",
                       gpu=True)
    device = keys.device
    eight_bytes = check.integer_dtypes(torch)[1] + (torch.float64,)   # int64, uint64 where this torch has it, float64
    check.check_tensor(torch, "values", values, eight_bytes, "8-byte elements (int64, uint64 or float64)", device=device)
    if values.numel() != keys.numel():
        raise ValueError(f"values hold {values.numel()} elements, keys {keys.numel()}")
    if values.data_ptr() % 8 != 0:
        raise ValueError("values must start on an 8-byte boundary")
    if count is not None:
        check.check_count(torch, count, "one element", device)
    n = check.key_count(keys)
    if storage is not None:
        check.check_storage(torch, storage, device, True)
    required = sorter.wide_value_storage_requirements(n).size
    storage = check.storage_or_new(torch, storage, required, device)
    stream = torch.cuda.current_stream(device).cuda_stream
    if count is None:
        sorter.cmd_wide_value_sort(stream, n, keys.data_ptr(), 0, values.data_ptr(), 0, storage.data_ptr(), 0)
    else:
        sorter.cmd_wide_value_sort_indirect(stream, n, count.data_ptr(), 0, keys.data_ptr(), 0, values.data_ptr(), 0,
                                            storage.data_ptr(), 0)
    return storage


def sort_segments_key_value64(sorter: Sorter, keys, offsets, values, storage=None):
    """Sorts ``keys[offsets[i]:offsets[i + 1]]`` for every ``i < offsets.numel() - 1`` in place as uint32, ``values`` (8 bytes
    each: int64, uint64 or float64) travelling with their keys.  ``offsets``: int32 / uint32, one-dimensional, at least one
    entry, on the keys' device.  ``storage``: a uint8 tensor of at least
    ``sorter.wide_value_storage_requirements(keys.numel())`` bytes on the keys' device whose address is a multiple of 16,
    allocated here when omitted.  Returns the storage used (one sort in flight per storage).

    Types, shapes and lengths are checked first, then that every array lives where the keys live, then the storage, and last
    that this place is a GPU: every refusal but the last can be met without one."""
    import torch

    four_bytes, eight_bytes = check.integer_dtypes(torch)
    check.check_tensor(torch, "keys", keys, four_bytes, "4-byte integers (int32 or uint32, sorted as uint32)")
    check.check_offsets(torch, offsets, "4-byte integers (int32 or uint32)")
    check.check_tensor(torch, "values", values, eight_bytes + (torch.float64,), "8-byte elements (int64, uint64 or float64)")
    if values.numel() != keys.numel():
        raise ValueError(f"values hold {values.numel()} elements, keys {keys.numel()}")
    if values.data_ptr() % 8 != 0:
        raise ValueError("values must start on an 8-byte boundary")
    n = check.key_count(keys)
    device = keys.device
    for name, t in (("offsets", offsets), ("values", values)):
        if t.device != device:
            raise ValueError(f"{name} is on {t.device}, keys are on {device}")
    if storage is not None:
        check.check_storage(torch, storage, device, True)
    required = sorter.wide_value_storage_requirements(n).size
    if storage is not None:
        check.storage_or_new(torch, storage, required, device)   # (too small: refused)
    check.check_device("keys", keys)
    if storage is None:
        storage = check.storage_or_new(torch, None, required, device)
    sorter.cmd_wide_value_sort_segmented(torch.cuda.current_stream(device).cuda_stream, n, offsets.numel() - 1,
                                         offsets.data_ptr(), 0, keys.data_ptr(), 0, values.data_ptr(), 0,
                                         storage.data_ptr(), 0)
    return storage
