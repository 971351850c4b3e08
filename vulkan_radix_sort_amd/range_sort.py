"""Sort of 32-bit keys held in torch tensors by a bit range of the key, at every size.

``sort_range(sorter, keys, begin_bit, end_bit)`` is ``sort_bits`` without its bound on the number of keys: it reorders a
one-dimensional ``torch.int32`` (or ``torch.uint32``) tensor in place, ascending by the field
``(key >> begin_bit) & (2**(end_bit - begin_bit) - 1)`` and stably -- keys of equal field keep their input order, every key
comes back whole, and ``values``, 4-byte integers of the same length, travel with their keys
(``vrdxHipCmdRangeSort[KeyValue]``; CUB's ``begin_bit`` / ``end_bit``).

``0 <= begin_bit <= end_bit <= 32``; an empty range leaves everything as it is, the range of all 32 bits is the whole-key
sort.  Up to 16384 keys the call records what ``sort_bits`` records; beyond that the chunked form, one count, scan and
scatter per digit of the range (``sorter.describe_range_sort_plan`` says which).

The checks are those of ``sort_bits``, in its order, without the bound: types, dtypes, shapes, the range and the lengths
first, then where the tensors live.  No data is read, so the call does not synchronise and can be captured into a
``torch.cuda.graph``; it runs on torch's current stream.

``sort_range(..., count=t)`` sorts only ``keys[:t]`` (and ``values[:t]``), ``t`` a one-element ``int32`` / ``uint32`` tensor on
the keys' device that is read on the GPU when the sort runs (``vrdxHipCmdRangeSort[KeyValue]Indirect``).  ``keys.numel()`` is
the bound -- a count beyond it is clamped to it -- and sizes the storage; elements from the count on are left alone.
"""
from __future__ import annotations

from . import _checks as check
from .api import Sorter, record_range_sort


def sort_range(sorter: Sorter, keys, begin_bit, end_bit, values=None, count=None, storage=None):
    """Sorts ``keys`` in place by their bits [begin_bit, end_bit) (``values``, if given, travel with their keys).
    ``storage``: a uint8 tensor of at least ``sorter.storage_requirements(keys.numel())`` bytes
    (``key_value_storage_requirements`` with values) on the keys' device whose address is a multiple of 16, allocated here
    when omitted.  ``count``: a one-element int32 / uint32 tensor on the keys' device; only the first
    min(count, keys.numel()) elements are sorted, the count is read on the device and must not be part of ``storage``.
    Returns the storage used (one sort in flight per storage)."""
    import torch

    check.check_tensor(torch, "keys", keys, check.integer_dtypes(torch)[0],
                       "4-byte integers (int32 or uint32, ordered as uint32 fields)")
    if values is not None:
        check.check_values(torch, values, keys, "4-byte integers (int32 or uint32)")
    check.check_bit_range(begin_bit, end_bit)
    n = check.key_count(keys)
    if count is not None:
        check.check_count(torch, count)
    if storage is not None:
        check.check_storage(torch, storage)
    # where they live
    check.check_device("keys", keys)
    device = keys.device
    for name, t in (("values", values), ("count", count), ("storage", storage)):
        if t is not None:
            check.check_device(name, t, device)
    if storage is not None:
        check.check_storage_aligned(storage)
    required = (sorter.key_value_storage_requirements(n) if values is not None else sorter.storage_requirements(n)).size
    storage = check.storage_or_new(torch, storage, required, device)
    record_range_sort(sorter, torch.cuda.current_stream(device).cuda_stream, n, count, keys, values, (begin_bit, end_bit),
                      storage)
    return storage
