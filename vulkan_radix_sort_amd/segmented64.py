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

from .api import Sorter
from .segmented import MAX_ELEMENTS, _four_byte_integer_dtypes
from .sort64 import _check_array, _check_keys


def sort_segments64(sorter: Sorter, keys, offsets, values=None, storage=None, order=None, descending=False):
    """Sorts ``keys[offsets[i]:offsets[i + 1]]`` for every ``i < offsets.numel() - 1`` in place as uint64 (values, if given,
    travel with their keys).  ``storage``: a uint8 tensor of at least
    ``sorter.storage_requirements64(keys.numel(), key_value=values is not None)`` bytes on the keys' device whose address is
    a multiple of 16, allocated here when omitted.  ``order``, ``descending``: as for ``sort64``; ``order=None`` with
    ``descending=False`` is the unsigned ascending sort.  Returns the storage used (one sort in flight per storage)."""
    import torch

    four = _four_byte_integer_dtypes(torch)
    word = _check_keys(torch, keys, order, descending)
    _check_array(torch, "offsets", offsets, four, "4-byte integers (int32 or uint32)", keys.device)
    if offsets.numel() < 1:
        raise ValueError("offsets must hold segment_count + 1 >= 1 entries")
    if values is not None:
        _check_array(torch, "values", values, four, "4-byte integers (int32 or uint32)", keys.device)
        if values.numel() != keys.numel():
            raise ValueError(f"values hold {values.numel()} elements, keys {keys.numel()}")
    n = keys.numel()
    if n > MAX_ELEMENTS:
        raise ValueError(f"{n} keys: at most {MAX_ELEMENTS} per call")
    segment_count = offsets.numel() - 1
    if storage is not None:
        if not isinstance(storage, torch.Tensor) or storage.dtype != torch.uint8 or not storage.is_contiguous():
            raise TypeError("storage must be a contiguous uint8 torch.Tensor")
        if storage.device != keys.device:
            raise ValueError(f"storage is on {storage.device}, keys are on {keys.device}")
        if storage.data_ptr() % 16 != 0:
            raise ValueError("storage must start on a 16-byte boundary")
    required = sorter.storage_requirements64(n, key_value=values is not None).size
    if storage is None:
        storage = torch.empty(required, dtype=torch.uint8, device=keys.device)
    elif storage.numel() < required:
        raise ValueError(f"storage holds {storage.numel()} bytes, the sort needs {required}")
    stream = torch.cuda.current_stream(keys.device).cuda_stream
    if word is not None:
        if values is None:
            sorter.cmd_sort_segmented64_ordered(stream, n, segment_count, offsets.data_ptr(), 0, keys.data_ptr(), 0, word,
                                                storage.data_ptr(), 0)
        else:
            sorter.cmd_sort_segmented64_ordered_key_value(stream, n, segment_count, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                                          values.data_ptr(), 0, word, storage.data_ptr(), 0)
    elif values is None:
        sorter.cmd_sort_segmented64(stream, n, segment_count, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                    storage.data_ptr(), 0)
    else:
        sorter.cmd_sort_segmented64_key_value(stream, n, segment_count, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                              values.data_ptr(), 0, storage.data_ptr(), 0)
    return storage
