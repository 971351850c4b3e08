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

from . import _checks as check
from .api import Sorter, record_sort


def sort64(sorter: Sorter, keys, values=None, storage=None, count=None, order=None, descending=False):
    """Sorts ``keys`` in place as uint64 (``values``, if given, travel with their keys).  ``storage``: a uint8 tensor of at
    least ``sorter.storage_requirements64(keys.numel(), key_value=values is not None)`` bytes on the keys' device whose
    address is a multiple of 16, allocated here when omitted.  ``count``: a one-element int32 / uint32 tensor on the keys'
    device; only the first min(count, keys.numel()) elements are sorted, the count is read on the device and must not be
    part of ``storage``.  ``order``: ``"uint64"``, ``"int64"`` or ``"float64"`` (IEEE-754 totalOrder; keys may then be a
    ``torch.float64`` tensor), ``descending``: the reverse of it, equal keys still in input order; ``order=None`` with
    ``descending=False`` is the unsigned ascending sort.  Returns the storage used (one sort in flight per storage)."""
    import torch

    word = check.check_keys(torch, keys, order, descending)
    device = keys.device
    if values is not None:
        check.check_values(torch, values, keys, "4-byte integers (int32 or uint32)", device)
    if count is not None:
        check.check_count(torch, count, "one element", device)
    n = check.key_count(keys)
    if storage is not None:
        check.check_storage(torch, storage, device, True)
    required = sorter.storage_requirements64(n, key_value=values is not None).size
    storage = check.storage_or_new(torch, storage, required, device)
    # (sorter, key bits, stream, count, offsets, segment count, indirect, keys, values, bit range, order, storage)
    record_sort(sorter, 64, torch.cuda.current_stream(device).cuda_stream, n, None, None, count, keys, values, None, word, storage)
    return storage
