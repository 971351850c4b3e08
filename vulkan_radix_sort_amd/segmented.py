"""Segmented sort of torch tensors: many independent arrays, packed back to back, in one recorded call.

``sort_segments(sorter, keys, offsets)`` sorts every segment ``keys[offsets[i]:offsets[i + 1]]`` on its own, ascending as
uint32 and stably, in place, on torch's current stream (``vrdxHipCmdSortSegmented[KeyValue]``).  The offsets stay on the
device: this module checks dtypes, shapes and devices on the host and never reads the offsets' values, so the call does not
synchronise and can be captured into a ``torch.cuda.graph``.  Offsets that decrease or end behind ``keys.numel()`` leave
their segment alone and raise ``STATUS_SEGMENTS_INVALID`` (``Sorter.read_status`` / ``Sorter.read_sorter_status``).
"""
from __future__ import annotations

from .api import Sorter

MAX_ELEMENTS = 0x3FFFFFFC  # VRDX_MAX_ELEMENTS (vrdx_layout.h)


def _four_byte_integer_dtypes(torch):
    dtypes = [torch.int32]
    if hasattr(torch, "uint32"):
        dtypes.append(torch.uint32)
    return tuple(dtypes)


def _check_array(torch, name, t, device=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype not in _four_byte_integer_dtypes(torch):
        raise TypeError(f"{name} must hold 4-byte integers (int32 or uint32, sorted as uint32), got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must live on a GPU, got {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, keys are on {device}")


def sort_segments(sorter: Sorter, keys, offsets, values=None, storage=None):
    """Sorts ``keys[offsets[i]:offsets[i + 1]]`` for every ``i < offsets.numel() - 1`` in place (values, if given, travel
    with their keys).  ``storage``: a uint8 tensor of at least ``sorter.[key_value_]storage_requirements(keys.numel())``
    bytes on the keys' device, allocated here when omitted.  Returns the storage used (one sort in flight per storage)."""
    import torch

    _check_array(torch, "keys", keys)
    _check_array(torch, "offsets", offsets, keys.device)
    if offsets.numel() < 1:
        raise ValueError("offsets must hold segment_count + 1 >= 1 entries")
    if values is not None:
        _check_array(torch, "values", values, keys.device)
        if values.numel() != keys.numel():
            raise ValueError(f"values hold {values.numel()} elements, keys {keys.numel()}")
    n = keys.numel()
    if n > MAX_ELEMENTS:
        raise ValueError(f"{n} keys: at most {MAX_ELEMENTS} per call")
    segment_count = offsets.numel() - 1
    required = (sorter.key_value_storage_requirements(n) if values is not None else sorter.storage_requirements(n)).size
    if storage is None:
        storage = torch.empty(required, dtype=torch.uint8, device=keys.device)
    else:
        if not isinstance(storage, torch.Tensor) or storage.dtype != torch.uint8 or not storage.is_contiguous():
            raise TypeError("storage must be a contiguous uint8 torch.Tensor")
        if storage.device != keys.device:
            raise ValueError(f"storage is on {storage.device}, keys are on {keys.device}")
        if storage.numel() < required:
            raise ValueError(f"storage holds {storage.numel()} bytes, the sort needs {required}")
    stream = torch.cuda.current_stream(keys.device).cuda_stream
    if values is None:
        sorter.cmd_sort_segmented(stream, n, segment_count, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                  storage.data_ptr(), 0)
    else:
        sorter.cmd_sort_segmented_key_value(stream, n, segment_count, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                            values.data_ptr(), 0, storage.data_ptr(), 0)
    return storage
