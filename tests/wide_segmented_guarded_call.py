"""One guarded call of the segmented sort of 32-bit keys with 64-bit values (the row of
vulkan_radix_sort_amd.api.WIDE_VALUE_SEGMENTED_CALLS) for tests/test_wide_value_segmented_gpu.py, put together from the pieces
of guarded_call.py in the manner of wide_guarded_call.py: keys, values and offsets each in an allocation of their own between
guard bytes, the storage poisoned between bands, the byte offsets through the call's offset arguments, the failure word and the
verdict word read behind the call, the sorter's word on request."""
import numpy as np

from guarded_call import (BAND, FRONT, GUARD_BYTE, NEIGHBOURS, TAIL, Sorted, address, ballot_sorter, poisoned_storage,  # noqa: F401
                          sorter, to_device, to_host, torch_mod)
from vulkan_radix_sort_amd import api

(CALL,) = api.WIDE_VALUE_SEGMENTED_CALLS


def wide_segmented_call(torch, sorter, keys, values, offsets, *, count=None, keys_off=0, values_off=0, offsets_off=0,
                        storage_off=0, storage=None, pool=None, expect_status=0, sticky=None, keep_before=False,
                        device="cuda"):
    """keys: uint32, values: uint64, the FULL host arrays; offsets: segment_count + 1 words as they go to the device; count:
    maxElementCount (default: all of keys), which also sizes the storage requirement.  The checks are guarded_call's: the guard
    bytes around keys, values and offsets, the offsets unchanged, the bytes in front of the storage offset and behind the
    requirement, the failure word (expect_status), word 1 reading VERDICT_NONE, and with `sticky` the sorter's word."""
    keys = np.ascontiguousarray(keys, np.uint32)
    values = np.ascontiguousarray(values, np.uint64)
    offsets = np.ascontiguousarray(offsets).astype(np.uint32)
    assert len(keys) == len(values) and values_off % 8 == 0 and keys_off % 4 == 0 and offsets_off % 4 == 0
    count = len(keys) if count is None else count
    on_gpu = torch.device(device).type == "cuda"   # (anything else: a sorter that works on host memory, stream 0)
    stream = torch.cuda.current_stream().cuda_stream if on_gpu else 0
    dk = to_device(torch, keys, FRONT + keys_off, TAIL, device)
    dv = to_device(torch, values, FRONT + values_off, TAIL, device)
    do = to_device(torch, offsets, FRONT + offsets_off, NEIGHBOURS, device)
    req = sorter.wide_value_storage_requirements(count)
    assert req.usage == api.STORAGE_USAGE
    end = storage_off + req.size
    if storage is None:
        storage = poisoned_storage(torch, req.size, storage_off, device=device)
    assert storage.data_ptr() % 16 == 0 and storage_off % 16 == 0 and storage.numel() >= end
    assert all(address(t)[0] % 16 == 0 for t in (dk, dv, do))
    before = storage.clone() if keep_before else None
    front, behind = storage[:storage_off].clone(), storage[end:].clone()

    given = {"command_buffer": stream, "max_element_count": count, "segment_count": len(offsets) - 1,
             "storage": storage.data_ptr(), "storage_offset": storage_off, "query_pool": pool, "query": 0}
    for name, t in (("keys", dk), ("values", dv), ("offsets", do)):
        given[name], given[name + "_offset"] = address(t)
    getattr(sorter, CALL.method)(*(given[name] for name, _ in CALL.parameters))
    if on_gpu:
        torch.cuda.synchronize()

    if count > 0 and len(offsets) > 1:
        if expect_status is not None:
            status = sorter.read_status(stream, storage.data_ptr(), storage_off)
            assert status == expect_status, f"the failure word is {status:#x}, not {expect_status:#x}"
        verdict = sorter.read_plan_verdict(stream, storage.data_ptr(), storage_off)
        assert verdict == api.VERDICT_NONE, f"word 1 reads {verdict}, not VERDICT_NONE"
    if sticky is not None:
        status = sorter.read_sorter_status(stream)
        assert status == sticky, f"the sorter's sticky word is {status:#x}, not {sticky:#x}"
    bad = torch.nonzero(storage[:storage_off] != front).flatten()[-8:].tolist()
    assert not bad, f"wrote in front of the storage offset {storage_off}, at bytes {bad}"
    bad = torch.nonzero(storage[end:] != behind).flatten()[:8].tolist()
    assert not bad, f"wrote behind the storage requirement of {req.size} bytes, at {bad} from its end"
    got = to_host(do, guarded=True, what="the offsets")
    assert np.array_equal(got, offsets), f"the offsets changed, at {np.flatnonzero(got != offsets)[:8].tolist()}"
    got_keys = to_host(dk, guarded=True, what="the keys")
    got_values = to_host(dv, guarded=True, what="the values")
    return Sorted(got_keys, got_values, storage, req.size, before)
