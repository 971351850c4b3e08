"""One guarded call of the sorts of 32-bit keys with 64-bit values (the rows of vulkan_radix_sort_amd.api.WIDE_VALUE_CALLS)
for tests/test_wide_value_gpu.py, put together from the pieces of guarded_call.py (`guarded_call` itself dispatches on
RECORDING_CALLS only): keys, values and the count word each in an allocation of their own between guard bytes -- or the count
word behind the keys in the keys' allocation --, the storage poisoned between bands, the byte offsets through the call's offset
arguments, the status word read behind the call."""
import numpy as np

from guarded_call import (BAND, FRONT, GUARD_BYTE, NEIGHBOURS, TAIL, Sorted, address, ballot_sorter, poisoned_storage,  # noqa: F401
                          sorter, to_device, to_host, torch_mod)
from vulkan_radix_sort_amd import api

ROWS = {call.facts[2]: call for call in api.WIDE_VALUE_CALLS}   # indirect or not


def wide_call(torch, sorter, keys, values, *, count=None, device_count=None, count_behind_keys=None, keys_off=0, values_off=0,
              indirect_off=0, storage_off=0, storage=None, pool=None, expect_status=0, keep_before=False, device="cuda"):
    """keys: uint32, values: uint64, the FULL host arrays; count: elementCount / maxElementCount (default: all of keys), which
    also sizes the storage requirement; device_count: the indirect call, the word the device reads -- in a buffer of its own at
    `indirect_off`, or with count_behind_keys = g in the keys' buffer, g guard bytes behind the last key.  The checks are
    guarded_call's: the guard bytes around keys, values and count word, the bytes in front of the storage offset and behind
    the requirement, the count word unchanged, the failure word."""
    keys = np.ascontiguousarray(keys, np.uint32)
    values = np.ascontiguousarray(values, np.uint64)
    assert len(keys) == len(values) and values_off % 8 == 0 and keys_off % 4 == 0 and count_behind_keys in (None, 0, 4, 8, 12)
    call = ROWS[device_count is not None]
    count = len(keys) if count is None else count
    on_gpu = torch.device(device).type == "cuda"   # (anything else: a sorter that works on host memory, stream 0)
    stream = torch.cuda.current_stream().cuda_stream if on_gpu else 0
    body = keys.view(np.uint8)
    word = np.array([0 if device_count is None else device_count], np.uint32)
    if count_behind_keys is not None:
        body = np.concatenate([body, np.full(count_behind_keys, GUARD_BYTE, np.uint8), word.view(np.uint8)])
    dk = to_device(torch, body, FRONT + keys_off, TAIL, device)
    dv = to_device(torch, values, FRONT + values_off, TAIL, device)
    dc = None
    if count_behind_keys is not None:
        dc = dk[len(body) - 4:]
    elif device_count is not None:
        dc = to_device(torch, word, FRONT + indirect_off, NEIGHBOURS, device)
    req = sorter.wide_value_storage_requirements(count)
    assert req.usage == api.STORAGE_USAGE
    end = storage_off + req.size
    if storage is None:
        storage = poisoned_storage(torch, req.size, storage_off, device=device)
    assert storage.data_ptr() % 16 == 0 and storage_off % 16 == 0
    before = storage.clone() if keep_before else None
    front, behind = storage[:storage_off].clone(), storage[end:].clone()

    given = {"command_buffer": stream, "element_count": count, "max_element_count": count, "storage": storage.data_ptr(),
             "storage_offset": storage_off, "query_pool": pool, "query": 0}
    for name, t in (("keys", dk), ("values", dv), ("indirect", dc)):
        given[name], given[name + "_offset"] = address(t) if t is not None else (None, None)
    getattr(sorter, call.method)(*(given[name] for name, _ in call.parameters))
    if on_gpu:
        torch.cuda.synchronize()

    if count > 0 and expect_status is not None:
        status = sorter.read_status(stream, storage.data_ptr(), storage_off)
        assert status == expect_status, f"the failure word is {status:#x}, not {expect_status:#x}"
    bad = torch.nonzero(storage[:storage_off] != front).flatten()[-8:].tolist()
    assert not bad, f"wrote in front of the storage offset {storage_off}, at bytes {bad}"
    bad = torch.nonzero(storage[end:] != behind).flatten()[:8].tolist()
    assert not bad, f"wrote behind the storage requirement of {req.size} bytes, at {bad} from its end"
    raw = to_host(dk, guarded=True, what="the keys")
    if count_behind_keys is not None:
        bad = np.flatnonzero(raw[keys.nbytes:len(raw) - 4] != GUARD_BYTE)
        assert bad.size == 0, f"wrote behind the keys: at {bad[:8].tolist()} from their end, in front of the count word"
        left = int(raw[len(raw) - 4:].view(np.uint32)[0])
        assert left == device_count, f"the count word behind the keys changed: {left}, not {device_count}"
    elif dc is not None:
        left = int(to_host(dc, guarded=True, what="the count word")[0])
        assert left == device_count, f"the count word changed: {left}, not {device_count}"
    got_keys = raw[:keys.nbytes].view(np.uint32)
    got_values = to_host(dv, guarded=True, what="the values")
    return Sorted(got_keys, got_values, storage, req.size, before)


def expected(keys, values, n):
    """what the call must leave: elements [0, n) by the stable argsort of the keys, the rest as it was"""
    keys, values = np.asarray(keys, np.uint32).copy(), np.asarray(values, np.uint64).copy()
    order = np.argsort(keys[:n], kind="stable")
    keys[:n], values[:n] = keys[:n][order], values[:n][order]
    return keys, values
