"""Sort of 64-bit keys held in torch tensors.

``sort64(sorter, keys)`` sorts a one-dimensional ``torch.int64`` (or ``torch.uint64``) tensor ascending as uint64 and stably,
in place, on torch's current stream (``vrdxHipCmdSort64[KeyValue]``); ``values``, 4-byte integers of the same length, travel
with their keys.  An ``int64`` tensor with negative entries therefore ends with them behind the others, unless an order is
asked for: ``sort64(sorter, keys, order="int64")`` sorts as signed integers, ``order="float64"`` sorts a ``torch.float64``
tensor (or 8-byte integers holding float64 bits) in IEEE-754 totalOrder, and ``descending=True`` reverses any of the
three -- stably in both directions, in the same kernels, at no extra trip over the keys
(``vrdxHipCmdSort64Ordered[KeyValue][Indirect]``).  totalOrder is ``torch.sort``'s order except that NaNs with the sign
bit set come first instead of last and that -0.0 sorts in front of +0.0 instead of equal to it.  Everything is checked on
the host before anything is recorded, no data is read, so the call does not synchronise and can be captured into a
``torch.cuda.graph``.

``sort64(sorter, keys, count=t)`` sorts only ``keys[:t]`` (and ``values[:t]``), ``t`` a one-element ``int32`` / ``uint32``
tensor on the keys' device that is read on the GPU when the sort runs (``vrdxHipCmdSort64[KeyValue]Indirect``): a count
that a kernel produced needs no read-back, and a captured call replays on whatever the tensor holds then.  ``keys.numel()``
is the bound -- a count beyond it is clamped to it -- and sizes the storage; elements from the count on are left alone.
"""
from __future__ import annotations

from .api import Sorter, order_word
from .segmented import MAX_ELEMENTS, _four_byte_integer_dtypes


def _eight_byte_integer_dtypes(torch):
    dtypes = [torch.int64]
    if hasattr(torch, "uint64"):
        dtypes.append(torch.uint64)
    return tuple(dtypes)


def _check_array(torch, name, t, dtypes, what, device=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must hold {what}, got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must live on a GPU, got {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, keys are on {device}")


def _check_keys(torch, keys, order, descending):
    """The dtype rule of ``sort64`` and ``sort_segments64``, and the order word (None: the calls without one).  ``order=None``
    with ``descending=False`` is the unsigned sort of 8-byte integers; otherwise ``order`` names how the 64 bits are read:
    ``"uint64"`` and ``"int64"`` take the 8-byte integer dtypes, ``"float64"`` takes ``torch.float64`` and 8-byte integers
    holding the bits."""
    if not isinstance(descending, bool):
        raise TypeError(f"descending must be a bool, got {type(descending).__name__}")
    if order is None:
        if descending:
            raise ValueError('descending=True needs an order: "uint64", "int64" or "float64"')
        _check_array(torch, "keys", keys, _eight_byte_integer_dtypes(torch), "8-byte integers (int64 or uint64, sorted as uint64)")
        return None
    word = order_word(order, descending)
    integers = _eight_byte_integer_dtypes(torch)
    if order == "float64":
        _check_array(torch, "keys", keys, (torch.float64,) + integers, "float64, or 8-byte integers holding float64 bits")
    else:
        _check_array(torch, "keys", keys, integers, f"8-byte integers (int64 or uint64, sorted as {order})")
    return word


def sort64(sorter: Sorter, keys, values=None, storage=None, count=None, order=None, descending=False):
    """Sorts ``keys`` in place as uint64 (``values``, if given, travel with their keys).  ``storage``: a uint8 tensor of at
    least ``sorter.storage_requirements64(keys.numel(), key_value=values is not None)`` bytes on the keys' device whose
    address is a multiple of 16, allocated here when omitted.  ``count``: a one-element int32 / uint32 tensor on the keys'
    device; only the first min(count, keys.numel()) elements are sorted, the count is read on the device and must not be
    part of ``storage``.  ``order``: ``"uint64"``, ``"int64"`` or ``"float64"`` (IEEE-754 totalOrder; keys may then be a
    ``torch.float64`` tensor), ``descending``: the reverse of it, equal keys still in input order; ``order=None`` with
    ``descending=False`` is the unsigned ascending sort.  Returns the storage used (one sort in flight per storage)."""
    import torch

    word = _check_keys(torch, keys, order, descending)
    if values is not None:
        _check_array(torch, "values", values, _four_byte_integer_dtypes(torch), "4-byte integers (int32 or uint32)",
                     keys.device)
        if values.numel() != keys.numel():
            raise ValueError(f"values hold {values.numel()} elements, keys {keys.numel()}")
    if count is not None:
        if not isinstance(count, torch.Tensor):
            raise TypeError(f"count must be a torch.Tensor, got {type(count).__name__}")
        if count.dtype not in _four_byte_integer_dtypes(torch):
            raise TypeError(f"count must hold a 4-byte integer (int32 or uint32), got {count.dtype}")
        if count.numel() != 1:
            raise ValueError(f"count must hold one element, got shape {tuple(count.shape)}")
        if count.device.type != "cuda":
            raise ValueError(f"count must live on a GPU, got {count.device}")
        if count.device != keys.device:
            raise ValueError(f"count is on {count.device}, keys are on {keys.device}")
    n = keys.numel()
    if n > MAX_ELEMENTS:
        raise ValueError(f"{n} keys: at most {MAX_ELEMENTS} per call")
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
        if count is None:
            if values is None:
                sorter.cmd_sort64_ordered(stream, n, keys.data_ptr(), 0, word, storage.data_ptr(), 0)
            else:
                sorter.cmd_sort64_ordered_key_value(stream, n, keys.data_ptr(), 0, values.data_ptr(), 0, word,
                                                    storage.data_ptr(), 0)
        elif values is None:
            sorter.cmd_sort64_ordered_indirect(stream, n, count.data_ptr(), 0, keys.data_ptr(), 0, word, storage.data_ptr(), 0)
        else:
            sorter.cmd_sort64_ordered_key_value_indirect(stream, n, count.data_ptr(), 0, keys.data_ptr(), 0,
                                                         values.data_ptr(), 0, word, storage.data_ptr(), 0)
    elif count is None:
        if values is None:
            sorter.cmd_sort64(stream, n, keys.data_ptr(), 0, storage.data_ptr(), 0)
        else:
            sorter.cmd_sort64_key_value(stream, n, keys.data_ptr(), 0, values.data_ptr(), 0, storage.data_ptr(), 0)
    elif values is None:
        sorter.cmd_sort64_indirect(stream, n, count.data_ptr(), 0, keys.data_ptr(), 0, storage.data_ptr(), 0)
    else:
        sorter.cmd_sort64_key_value_indirect(stream, n, count.data_ptr(), 0, keys.data_ptr(), 0, values.data_ptr(), 0,
                                             storage.data_ptr(), 0)
    return storage
