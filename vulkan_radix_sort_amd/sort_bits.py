"""Sort of 32-bit keys held in torch tensors by a bit range of the key.

``sort_bits(sorter, keys, begin_bit, end_bit)`` reorders a one-dimensional ``torch.int32`` (or ``torch.uint32``) tensor in
place, ascending by the field ``(key >> begin_bit) & (2**(end_bit - begin_bit) - 1)`` and stably: keys of equal field keep
their input order, and every key comes back whole -- the bits outside the range are carried along, not compared
(``vrdxHipCmdSortBits[KeyValue]``; CUB's ``begin_bit`` / ``end_bit``).  ``values``, 4-byte integers of the same length,
travel with their keys.

``0 <= begin_bit <= end_bit <= 32``; an empty range leaves everything as it is, the range of all 32 bits is the whole-key
sort.  A range sort runs in one workgroup: ``keys.numel()`` may be at most ``MAX_RANGE_ELEMENTS`` = 16384 for any other
range (the library refuses more, and so does this function, on the host).

Everything is checked on the host before anything is recorded -- types, dtypes, shapes, the range and the lengths first,
then where the tensors live -- and no data is read, so the call does not synchronise and can be captured into a
``torch.cuda.graph``; it runs on torch's current stream.

``sort_bits(..., count=t)`` sorts only ``keys[:t]`` (and ``values[:t]``), ``t`` a one-element ``int32`` / ``uint32`` tensor on
the keys' device that is read on the GPU when the sort runs (``vrdxHipCmdSortBits[KeyValue]Indirect``).  ``keys.numel()`` is
the bound -- a count beyond it is clamped to it -- and sizes the storage; elements from the count on are left alone.
"""
from __future__ import annotations

from .api import Sorter

MAX_ELEMENTS = 0x3FFFFFFC   # VRDX_MAX_ELEMENTS (vrdx_layout.h)
MAX_RANGE_ELEMENTS = 16384  # kSmallSortMaxElements (vrdx_kernels.h): range sorts are one-workgroup sorts


def _four_byte_integers(torch):
    return (torch.int32, torch.uint32) if hasattr(torch, "uint32") else (torch.int32,)


def _check_tensor(torch, name, t, dtypes, what, elements=None):
    """what can be told of a tensor wherever it lives"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must hold {what}, got {t.dtype}")
    if elements is not None and t.numel() != elements:
        raise ValueError(f"{name} must hold {elements} element(s), got shape {tuple(t.shape)}")
    if elements is None and t.dim() != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_device(name, t, keys):
    if t.device.type != "cuda":
        raise ValueError(f"{name} must live on a GPU, got {t.device}")
    if t.device != keys.device:
        raise ValueError(f"{name} is on {t.device}, keys are on {keys.device}")


def sort_bits(sorter: Sorter, keys, begin_bit, end_bit, values=None, count=None, storage=None):
    """Sorts ``keys`` in place by their bits [begin_bit, end_bit) (``values``, if given, travel with their keys).
    ``storage``: a uint8 tensor of at least ``sorter.storage_requirements(keys.numel())`` bytes
    (``key_value_storage_requirements`` with values) on the keys' device whose address is a multiple of 16, allocated here
    when omitted.  ``count``: a one-element int32 / uint32 tensor on the keys' device; only the first
    min(count, keys.numel()) elements are sorted, the count is read on the device and must not be part of ``storage``.
    Returns the storage used (one sort in flight per storage)."""
    import torch

    four_bytes = _four_byte_integers(torch)
    _check_tensor(torch, "keys", keys, four_bytes, "4-byte integers (int32 or uint32, ordered as uint32 fields)")
    if values is not None:
        _check_tensor(torch, "values", values, four_bytes, "4-byte integers (int32 or uint32)")
        if values.numel() != keys.numel():
            raise ValueError(f"values hold {values.numel()} elements, keys {keys.numel()}")
    for name, bit in (("begin_bit", begin_bit), ("end_bit", end_bit)):
        if isinstance(bit, bool) or not isinstance(bit, int):
            raise TypeError(f"{name} must be an int, got {type(bit).__name__}")
    if not 0 <= begin_bit <= end_bit <= 32:
        raise ValueError(f"the bit range [{begin_bit}, {end_bit}) is not inside [0, 32] with begin_bit <= end_bit")
    n = keys.numel()
    if n > MAX_ELEMENTS:
        raise ValueError(f"{n} keys: at most {MAX_ELEMENTS} per call")
    if n > MAX_RANGE_ELEMENTS and 0 < end_bit - begin_bit < 32:
        raise ValueError(f"{n} keys: a sort by a bit range takes at most {MAX_RANGE_ELEMENTS} (only [0, 32) takes more)")
    if count is not None:
        _check_tensor(torch, "count", count, four_bytes, "a 4-byte integer (int32 or uint32)", elements=1)
    if storage is not None and (not isinstance(storage, torch.Tensor) or storage.dtype != torch.uint8
                                or not storage.is_contiguous()):
        raise TypeError("storage must be a contiguous uint8 torch.Tensor")
    # where they live
    _check_device("keys", keys, keys)
    for name, t in (("values", values), ("count", count), ("storage", storage)):
        if t is not None:
            _check_device(name, t, keys)
    if storage is not None and storage.data_ptr() % 16 != 0:
        raise ValueError("storage must start on a 16-byte boundary")
    required = (sorter.key_value_storage_requirements(n) if values is not None else sorter.storage_requirements(n)).size
    if storage is None:
        storage = torch.empty(required, dtype=torch.uint8, device=keys.device)
    elif storage.numel() < required:
        raise ValueError(f"storage holds {storage.numel()} bytes, the sort needs {required}")
    stream = torch.cuda.current_stream(keys.device).cuda_stream
    k, s = keys.data_ptr(), storage.data_ptr()
    if count is None:
        if values is None:
            sorter.cmd_sort_bits(stream, n, k, 0, begin_bit, end_bit, s, 0)
        else:
            sorter.cmd_sort_bits_key_value(stream, n, k, 0, values.data_ptr(), 0, begin_bit, end_bit, s, 0)
    elif values is None:
        sorter.cmd_sort_bits_indirect(stream, n, count.data_ptr(), 0, k, 0, begin_bit, end_bit, s, 0)
    else:
        sorter.cmd_sort_bits_key_value_indirect(stream, n, count.data_ptr(), 0, k, 0, values.data_ptr(), 0, begin_bit,
                                                end_bit, s, 0)
    return storage
