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

from .api import Sorter
from .segmented import MAX_ELEMENTS
from .sort_bits import _check_device, _check_tensor, _four_byte_integers


def sort_segments_bits(sorter: Sorter, keys, offsets, begin_bit, end_bit, values=None, storage=None):
    """Sorts ``keys[offsets[i]:offsets[i + 1]]`` for every ``i < offsets.numel() - 1`` in place by the bits
    [begin_bit, end_bit) of the keys (values, if given, travel with their keys).  ``storage``: a uint8 tensor of at least
    ``sorter.[key_value_]storage_requirements(keys.numel())`` bytes on the keys' device, allocated here when omitted.
    Returns the storage used (one sort in flight per storage)."""
    import torch

    for name, bit in (("begin_bit", begin_bit), ("end_bit", end_bit)):
        if isinstance(bit, bool) or not isinstance(bit, int):
            raise TypeError(f"{name} must be an int, got {type(bit).__name__}")
    if not 0 <= begin_bit <= end_bit <= 32:
        raise ValueError(f"the bit range [{begin_bit}, {end_bit}) is not inside [0, 32] with begin_bit <= end_bit")
    four_bytes = _four_byte_integers(torch)
    _check_tensor(torch, "keys", keys, four_bytes, "4-byte integers (int32 or uint32, ordered as uint32 fields)")
    _check_tensor(torch, "offsets", offsets, four_bytes, "4-byte integers (int32 or uint32)")
    if offsets.numel() < 1:
        raise ValueError("offsets must hold segment_count + 1 >= 1 entries")
    if values is not None:
        _check_tensor(torch, "values", values, four_bytes, "4-byte integers (int32 or uint32)")
        if values.numel() != keys.numel():
            raise ValueError(f"values hold {values.numel()} elements, keys {keys.numel()}")
    n = keys.numel()
    if n > MAX_ELEMENTS:
        raise ValueError(f"{n} keys: at most {MAX_ELEMENTS} per call")
    if storage is not None and (not isinstance(storage, torch.Tensor) or storage.dtype != torch.uint8
                                or not storage.is_contiguous()):
        raise TypeError("storage must be a contiguous uint8 torch.Tensor")
    # where they live
    _check_device("keys", keys, keys)
    for name, t in (("offsets", offsets), ("values", values), ("storage", storage)):
        if t is not None:
            _check_device(name, t, keys)
    segment_count = offsets.numel() - 1
    required = (sorter.key_value_storage_requirements(n) if values is not None else sorter.storage_requirements(n)).size
    if storage is None:
        storage = torch.empty(required, dtype=torch.uint8, device=keys.device)
    elif storage.numel() < required:
        raise ValueError(f"storage holds {storage.numel()} bytes, the sort needs {required}")
    stream = torch.cuda.current_stream(keys.device).cuda_stream
    if values is None:
        sorter.cmd_sort_segmented_bits(stream, n, segment_count, offsets.data_ptr(), 0, keys.data_ptr(), 0, begin_bit, end_bit,
                                       storage.data_ptr(), 0)
    else:
        sorter.cmd_sort_segmented_bits_key_value(stream, n, segment_count, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                                 values.data_ptr(), 0, begin_bit, end_bit, storage.data_ptr(), 0)
    return storage
