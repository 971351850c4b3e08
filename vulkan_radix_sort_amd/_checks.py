"""The host-side argument checks of the five torch front ends (sort_segments, sort64, sort_segments64, sort_bits,
sort_segments_bits), each written once.  Every check raises before anything is recorded and reads no tensor data.  A front end's time is host time in front
of every sort, so the checks ask torch for as little as they can: ``keys.device`` once per call, the dtype tuples once per
process.

Known differences between the front ends.  They are behaviour -- a caller sees them in which refusal wins, or in its wording
-- so this module keeps them, and tests/golden/front_end_cases.json pins them; a change that means to unify one starts here.

* sort_segments, sort64 and sort_segments64 check where each array lives right behind its shape (``check_tensor`` with
  ``gpu=`` / ``device=``); sort_bits and sort_segments_bits check every type, shape, the range and the lengths first and every
  device afterwards (``check_device``).
* sort_segments and sort_segments_bits take a storage at any address; the other three want it on a 16-byte boundary
  (``aligned=``, ``check_storage_aligned``).
* sort_segments asks the sorter for the required size before it looks at the storage's type, the others afterwards.
* sort_segments, sort64 and sort_segments64 tell a storage on the CPU "storage is on cpu, keys are on cuda:0"
  (``check_storage`` with ``device=``); the range sorts tell it "storage must live on a GPU" (``check_device``).
* sort64 words its refusal of a count of several elements itself ("one element", ``holds=``); sort_bits says "1 element(s)".
* Each front end names what its keys, offsets and values must hold in its own words (``what``).
* sort_ordered and sort_segments_ordered (ordered.py) came later and follow sort64: ``check_keys32`` for dtype and order word,
  every array's device right behind its shape, the storage on a 16-byte boundary.
* sort_segments_key_value64 (wide_value.py) checks every type, shape, length and the values' alignment first, then that offsets,
  values and storage live where the keys live, then the storage's alignment and size, and only then that the place is a GPU.
* sort_segments_bits checks the bit range before the tensors, sort_bits behind keys and values; only sort_bits bounds the
  number of keys of a partial range (``check_range_count``).
* sort_range (range_sort.py) is sort_bits check for check, in its order, without ``check_range_count``: no size is refused.
"""
from __future__ import annotations

from .api import order_word, order_word32

MAX_ELEMENTS = 0x3FFFFFFC   # VRDX_MAX_ELEMENTS (vrdx_layout.h)
MAX_RANGE_ELEMENTS = 16384  # kSmallSortMaxElements (vrdx_kernels.h): range sorts are one-workgroup sorts

_MISALIGNED = "storage must start on a 16-byte boundary"
_INTEGER_DTYPES = None


def integer_dtypes(torch):
    """(the 4-byte integer dtypes, the 8-byte ones) of this torch"""
    global _INTEGER_DTYPES
    if _INTEGER_DTYPES is None:
        _INTEGER_DTYPES = ((torch.int32, torch.uint32) if hasattr(torch, "uint32") else (torch.int32,),
                           (torch.int64, torch.uint64) if hasattr(torch, "uint64") else (torch.int64,))
    return _INTEGER_DTYPES


def check_tensor(torch, name, t, dtypes, what, elements=None, holds=None, gpu=False, device=None):
    """What can be told of a tensor wherever it lives: its type, its dtype (``what`` it must hold, in the caller's words), that
    it is one-dimensional -- or, with ``elements``, of that many (``holds``: the caller's words for it) -- and contiguous.
    Then, for the front ends that check it right here, where it lives: on a GPU (``gpu``), on the keys' ``device``."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must hold {what}, got {t.dtype}")
    if elements is not None and t.numel() != elements:
        raise ValueError(f"{name} must hold {holds or f'{elements} element(s)'}, got shape {tuple(t.shape)}")
    if elements is None and t.dim() != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if gpu or device is not None:   # check_device, written out: one call less per tensor
        if not t.is_cuda:
            raise ValueError(f"{name} must live on a GPU, got {t.device}")
        if device is not None and t.device != device:
            raise ValueError(f"{name} is on {t.device}, keys are on {device}")


def check_device(name, t, device=None):
    """``t`` lives on a GPU, and on the keys' ``device`` (None: ``t`` is the keys)."""
    if not t.is_cuda:
        raise ValueError(f"{name} must live on a GPU, got {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, keys are on {device}")


def check_keys(torch, keys, order, descending):
    """The dtype rule of ``sort64`` and ``sort_segments64``, and the order word (None: the calls without one).  ``order=None``
    with ``descending=False`` is the unsigned sort of 8-byte integers; otherwise ``order`` names how the 64 bits are read:
    ``"uint64"`` and ``"int64"`` take the 8-byte integer dtypes, ``"float64"`` takes ``torch.float64`` and 8-byte integers
    holding the bits."""
    if not isinstance(descending, bool):
        raise TypeError(f"descending must be a bool, got {type(descending).__name__}")
    if order is None:
        if descending:
            raise ValueError('descending=True needs an order: "uint64", "int64" or "float64"')
        check_tensor(torch, "keys", keys, integer_dtypes(torch)[1], "8-byte integers (int64 or uint64, sorted as uint64)", gpu=True)
        return None
    word = order_word(order, descending)
    integers = integer_dtypes(torch)[1]
    if order == "float64":
        check_tensor(torch, "keys", keys, (torch.float64,) + integers, "float64, or 8-byte integers holding float64 bits", gpu=True)
    else:
        check_tensor(torch, "keys", keys, integers, f"8-byte integers (int64 or uint64, sorted as {order})", gpu=True)
    return word


def check_keys32(torch, keys, order, descending):
    """The dtype rule of ``sort_ordered`` and ``sort_segments_ordered``, and the order word: ``"uint32"`` and ``"int32"`` take
    the 4-byte integer dtypes, ``"float32"`` takes ``torch.float32`` and 4-byte integers holding the bits."""
    if not isinstance(descending, bool):
        raise TypeError(f"descending must be a bool, got {type(descending).__name__}")
    word = order_word32(order, descending)
    integers = integer_dtypes(torch)[0]
    if order == "float32":
        check_tensor(torch, "keys", keys, (torch.float32,) + integers, "float32, or 4-byte integers holding float32 bits", gpu=True)
    else:
        check_tensor(torch, "keys", keys, integers, f"4-byte integers (int32 or uint32, sorted as {order})", gpu=True)
    return word


def check_offsets(torch, offsets, what, device=None):
    check_tensor(torch, "offsets", offsets, integer_dtypes(torch)[0], what, device=device)
    if offsets.numel() < 1:
        raise ValueError("offsets must hold segment_count + 1 >= 1 entries")


def check_values(torch, values, keys, what, device=None):
    """4-byte integers, one per key."""
    check_tensor(torch, "values", values, integer_dtypes(torch)[0], what, device=device)
    if values.numel() != keys.numel():
        raise ValueError(f"values hold {values.numel()} elements, keys {keys.numel()}")


def check_count(torch, count, holds=None, device=None):
    """One 4-byte integer that the device reads."""
    check_tensor(torch, "count", count, integer_dtypes(torch)[0], "a 4-byte integer (int32 or uint32)", 1, holds, device=device)


def check_bit_range(begin_bit, end_bit):
    for name, bit in (("begin_bit", begin_bit), ("end_bit", end_bit)):
        if isinstance(bit, bool) or not isinstance(bit, int):
            raise TypeError(f"{name} must be an int, got {type(bit).__name__}")
    if not 0 <= begin_bit <= end_bit <= 32:
        raise ValueError(f"the bit range [{begin_bit}, {end_bit}) is not inside [0, 32] with begin_bit <= end_bit")


def key_count(keys):
    n = keys.numel()
    if n > MAX_ELEMENTS:
        raise ValueError(f"{n} keys: at most {MAX_ELEMENTS} per call")
    return n


def check_range_count(n, begin_bit, end_bit):
    if n > MAX_RANGE_ELEMENTS and 0 < end_bit - begin_bit < 32:
        raise ValueError(f"{n} keys: a sort by a bit range takes at most {MAX_RANGE_ELEMENTS} (only [0, 32) takes more)")


def check_storage(torch, storage, device=None, aligned=False):
    """A caller's storage: its type; with ``device``, that it is on the keys' device; with ``aligned``, where it starts."""
    if not isinstance(storage, torch.Tensor) or storage.dtype != torch.uint8 or not storage.is_contiguous():
        raise TypeError("storage must be a contiguous uint8 torch.Tensor")
    if device is not None and storage.device != device:
        raise ValueError(f"storage is on {storage.device}, keys are on {device}")
    if aligned and storage.data_ptr() % 16 != 0:
        raise ValueError(_MISALIGNED)


def check_storage_aligned(storage):
    if storage.data_ptr() % 16 != 0:
        raise ValueError(_MISALIGNED)


def storage_or_new(torch, storage, required, device):
    """The caller's storage if it holds ``required`` bytes, a new one on the keys' device if there is none."""
    if storage is None:
        return torch.empty(required, dtype=torch.uint8, device=device)
    if storage.numel() < required:
        raise ValueError(f"storage holds {storage.numel()} bytes, the sort needs {required}")
    return storage
