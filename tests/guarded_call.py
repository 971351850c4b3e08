"""What every GPU test of a recording call shares: the sorters of both ranking forms, host arrays to the device and back,
and ONE guarded call through the C ABI -- `guarded_call` -- for all rows of vulkan_radix_sort_amd.api.RECORDING_CALLS.  The
row is chosen by what the caller hands in, the argument list follows from the row's `parameters`; nothing here names an entry
point.  A plain module next to plan_model.py, imported the same way; the fixtures are module-scoped, so every test file that
imports them gets sorters of its own.  tests/test_guarded_call.py runs the call on the CPU against a sorter that misbehaves.

Every array the call sees lies inside an allocation of its own (the count word may share the keys'):

  keys, values     GUARD_BYTE x (FRONT + offset) | the array | GUARD_BYTE x tail (at least 256)
  count word       GUARD_BYTE x (FRONT + offset) | the word  | GUARD_BYTE x 16
  offsets          GUARD_BYTE x (FRONT + offset) | the words | GUARD_BYTE x 16
  storage          BAND_BYTE x storage_off | POISON_BYTE x requirement | BAND_BYTE x 256   (a caller's own: as it comes)

and the byte offsets go through the call's offset arguments.  FRONT is a multiple of 256, so an offset keeps its residue."""
import os
from typing import NamedTuple

import numpy as np
import pytest

from vulkan_radix_sort_amd import api

GUARD_BYTE = 0xC7    # around the caller's arrays; no byte of the other two
POISON_BYTE = 0xA5   # the storage on entry
BAND_BYTE = 0x5A     # in front of the storage offset and behind the requirement
FRONT = 256          # guard bytes in front of every array, in front of its offset
TAIL = 256           # ... and behind it, at least
BAND = 256           # bytes behind the storage requirement
NEIGHBOURS = 16      # guard bytes behind the count word and behind the offsets


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    return torch


@pytest.fixture(scope="module")
def sorter(torch_mod):
    import vulkan_radix_sort_amd as vrdx
    s = vrdx.Sorter()  # raises VrdxError if the HIP library cannot drive this GPU: no fallback
    yield s
    s.destroy()


@pytest.fixture(scope="module")
def ballot_sorter(torch_mod):
    import vulkan_radix_sort_amd as vrdx
    old = os.environ.get("VRDX_RANK")
    os.environ["VRDX_RANK"] = "ballot"  # read by vrdxCreateSorter
    try:
        s = vrdx.Sorter()
    finally:
        if old is None:
            del os.environ["VRDX_RANK"]
        else:
            os.environ["VRDX_RANK"] = old
    yield s
    s.destroy()


_SIGNED = {1: np.uint8, 4: np.int32, 8: np.int64}
_UNSIGNED = {1: np.uint8, 4: np.uint32, 8: np.uint64}


def to_device(torch, a, offset=0, tail=0, device="cuda"):
    """The host array `a` (uint8 or uint64 as it is, anything else as uint32) as a device tensor of the same bits -- uint8,
    int32 or int64 -- that lies at byte `offset` of an allocation of its own, GUARD_BYTE in front of it and in the `tail`
    bytes behind it.  `to_host(t, guarded=True)` checks those bytes; `address` splits its address for a call."""
    a = np.asarray(a)
    a = np.ascontiguousarray(a, dtype=a.dtype if a.dtype in (np.uint8, np.uint64) else np.uint32).ravel()
    assert offset % a.itemsize == 0
    raw = np.full(offset + a.nbytes + tail, GUARD_BYTE, dtype=np.uint8)
    raw[offset:offset + a.nbytes] = a.view(np.uint8)
    t = torch.from_numpy(raw).to(device)[offset:offset + a.nbytes]
    return t if a.itemsize == 1 else t.view(getattr(torch, np.dtype(_SIGNED[a.itemsize]).name))


def address(t):
    """(address of the allocation `t` lies in, byte offset of `t` in it): a call's buffer and offset arguments"""
    base = t.untyped_storage().data_ptr()
    return base, t.data_ptr() - base


def to_host(t, guarded=False, what="the array"):
    """The device tensor `t` as an unsigned host array of the same bits.  guarded: every byte of its allocation in front of
    it and behind it must be GUARD_BYTE; the message names `what` and the first offsets that differ, relative to the array's
    first byte (in front) and to the first byte behind it (behind)."""
    if guarded:
        import torch
        whole = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).cpu().numpy()
        begin = address(t)[1]
        end = begin + t.numel() * t.element_size()
        bad = np.flatnonzero(whole[:begin] != GUARD_BYTE)
        assert bad.size == 0, f"wrote in front of {what}: {bad.size} bytes, at {(bad - begin)[-8:].tolist()} from its start"
        bad = np.flatnonzero(whole[end:] != GUARD_BYTE)
        assert bad.size == 0, f"wrote behind {what}: {bad.size} bytes, at {bad[:8].tolist()} from its end"
        out = whole[begin:end].copy()
    else:
        out = t.contiguous().cpu().numpy().reshape(-1).view(np.uint8)
    return out.view(_UNSIGNED[t.element_size()])


def poisoned_storage(torch, required, storage_off=0, poison=True, device="cuda"):
    """BAND_BYTE x storage_off | POISON_BYTE (poison=False: 0) x required | BAND_BYTE x BAND"""
    storage = torch.full((storage_off + required + BAND,), BAND_BYTE, dtype=torch.uint8, device=device)
    storage[storage_off:storage_off + required] = POISON_BYTE if poison else 0
    return storage


ROWS = {call.facts: call for call in api.RECORDING_CALLS}


class Sorted(NamedTuple):
    """what `guarded_call` returns: the whole arrays as the device left them (values: None for a keys-only call), the storage
    tensor, the size of the requirement, and with keep_before the storage as it was on entry"""
    keys: np.ndarray
    values: np.ndarray
    storage: object
    required: int
    before: object


def guarded_call(torch, sorter, keys, values=None, *, offsets=None, count=None, device_count=None, count_behind_keys=None,
                 bit_range=None, order=None, keys_off=0, values_off=0, offsets_off=0, indirect_off=0, storage_off=0,
                 tail=TAIL, storage=None, poison=True, pool=None, expect_status=0, recorded=None, expect_refused=False,
                 sticky=None, keep_before=False, device="cuda"):
    """One recording call on torch's current stream, between guard bytes (the module's docstring has the layout).

    keys: uint32 or uint64, the FULL host array; values: uint32 or None; count: elementCount / maxElementCount (default: all
    of keys), which also sizes the storage requirement.  offsets: the segmented calls.  device_count: the indirect calls, the
    word the device reads -- in a buffer of its own at `indirect_off`, or with count_behind_keys = g in the keys' buffer, g
    guard bytes behind the last key.  bit_range: (beginBit, endBit); order: the order word.  A combination no row of
    RECORDING_CALLS takes is a TypeError, as in api.record_sort.

    storage: a caller's own tensor, used as it is (the bytes outside [storage_off, storage_off + requirement) are compared
    with what they were); poison=False: zeros where the requirement lies.  expect_status: the failure word in the storage,
    read whenever a sort was `recorded` (default: the count is not 0, the range is a valid non-empty one, not refused).
    expect_refused: the sorter's word is STATUS_ENQUEUE_REFUSED and no byte of the storage changed.  sticky: what
    read_sorter_status must return (None: not read -- it is state of the sorter, not of this call).  keep_before: the result
    carries a copy of the storage as it was on entry.  device: anything but "cuda" runs on stream 0 without a synchronise,
    for a sorter that works on host memory."""
    keys = np.ascontiguousarray(keys)
    key_bits = 8 * keys.dtype.itemsize
    extra = "+".join(name for name, given in (("Bits", bit_range), ("Ordered", order)) if given is not None) or None
    facts = (key_bits, offsets is not None, device_count is not None, values is not None, extra)
    call = ROWS.get(facts)
    if call is None:
        raise TypeError(f"no recording call takes (key bits, segmented, indirect, key+value, extra) = {facts}")
    count = len(keys) if count is None else count
    on_gpu = torch.device(device).type == "cuda"
    stream = torch.cuda.current_stream().cuda_stream if on_gpu else 0
    assert tail >= TAIL and keys_off % (key_bits // 8) == 0
    assert values_off % 4 == 0 and offsets_off % 4 == 0 and indirect_off % 4 == 0 and count_behind_keys in (None, 0, 4, 8, 12)

    # the arrays
    body = keys.view(np.uint8)
    word = np.array([0 if device_count is None else device_count], np.uint32)
    if count_behind_keys is not None:
        body = np.concatenate([body, np.full(count_behind_keys, GUARD_BYTE, np.uint8), word.view(np.uint8)])
    dk = to_device(torch, body, FRONT + keys_off, tail, device)
    dv = do = dc = None
    if values is not None:
        dv = to_device(torch, np.asarray(values).astype(np.uint32), FRONT + values_off, tail, device)
    if offsets is not None:
        offsets = np.asarray(offsets).astype(np.uint32)
        do = to_device(torch, offsets, FRONT + offsets_off, NEIGHBOURS, device)
    if count_behind_keys is not None:
        dc = dk[len(body) - 4:]
    elif device_count is not None:
        dc = to_device(torch, word, FRONT + indirect_off, NEIGHBOURS, device)

    # the storage
    key_value = values is not None
    req = (sorter.storage_requirements64(count, key_value) if key_bits == 64 else
           sorter.key_value_storage_requirements(count) if key_value else sorter.storage_requirements(count))
    assert req.usage == api.STORAGE_USAGE == 0x22
    end = storage_off + req.size
    if storage is None:
        storage = poisoned_storage(torch, req.size, storage_off, poison, device)
    assert storage.data_ptr() % 16 == 0 and (key_bits == 32 or storage_off % 16 == 0)
    assert all(t is None or address(t)[0] % 16 == 0 for t in (dk, dv, do, dc))
    before = storage.clone() if keep_before or expect_refused else None
    front, behind = storage[:storage_off].clone(), storage[end:].clone()

    # the call: the row's parameters in their canonical order
    given = {"command_buffer": stream, "element_count": count, "max_element_count": count, "storage": storage.data_ptr(),
             "storage_offset": storage_off, "query_pool": pool, "query": 0, "order": order}
    given["begin_bit"], given["end_bit"] = bit_range if bit_range is not None else (None, None)
    given["segment_count"] = len(offsets) - 1 if offsets is not None else None
    for name, t in (("keys", dk), ("values", dv), ("offsets", do), ("indirect", dc)):
        given[name], given[name + "_offset"] = address(t) if t is not None else (None, None)
    getattr(sorter, call.method)(*(given[name] for name, _ in call.parameters))
    if on_gpu:
        torch.cuda.synchronize()

    # the checks
    if recorded is None:
        recorded = count > 0 and not expect_refused and (bit_range is None or 0 <= bit_range[0] < bit_range[1] <= key_bits)
    if expect_refused:
        assert sorter.read_sorter_status(stream) == api.STATUS_ENQUEUE_REFUSED, "a call that must be refused was not"
        bad = torch.nonzero(storage != before).flatten()[:8].tolist()
        assert not bad, f"a refused call wrote to the storage, at bytes {bad}"
    elif recorded and expect_status is not None:
        status = sorter.read_status(stream, storage.data_ptr(), storage_off)
        assert status == expect_status, f"the failure word is {status:#x}, not {expect_status:#x}"
    if sticky is not None and not expect_refused:
        status = sorter.read_sorter_status(stream)
        assert status == sticky, f"the sorter's sticky word is {status:#x}, not {sticky:#x}"
    bad = torch.nonzero(storage[:storage_off] != front).flatten()[-8:].tolist()
    assert not bad, f"wrote in front of the storage offset {storage_off}, at bytes {bad}"
    bad = torch.nonzero(storage[end:] != behind).flatten()[:8].tolist()
    assert not bad, f"wrote behind the storage requirement of {req.size} bytes, at {bad} from its end"
    if do is not None:
        got = to_host(do, guarded=True, what="the offsets")
        assert np.array_equal(got, offsets), f"the offsets changed, at {np.flatnonzero(got != offsets)[:8].tolist()}"
    raw = to_host(dk, guarded=True, what="the keys")
    if count_behind_keys is not None:
        bad = np.flatnonzero(raw[keys.nbytes:len(raw) - 4] != GUARD_BYTE)
        assert bad.size == 0, f"wrote behind the keys: at {bad[:8].tolist()} from their end, in front of the count word"
        left = int(raw[len(raw) - 4:].view(np.uint32)[0])
        assert left == device_count, f"the count word behind the keys changed: {left}, not {device_count}"
    elif dc is not None:
        left = int(to_host(dc, guarded=True, what="the count word")[0])   # (its neighbours are guard bytes)
        assert left == device_count, f"the count word changed: {left}, not {device_count}"
    got_keys = raw[:keys.nbytes].view(keys.dtype)
    got_values = to_host(dv, guarded=True, what="the values") if dv is not None else None
    return Sorted(got_keys, got_values, storage, req.size, before)
