"""One guarded call of the ordered 32-bit sorts (the rows of vulkan_radix_sort_amd.api.ORDERED_SORT_CALLS) for
tests/test_ordered_sort_gpu.py and tests/test_ordered_sort_segmented_gpu.py, put together from the pieces of guarded_call.py
(`guarded_call` itself dispatches on RECORDING_CALLS only): every array in an allocation of its own between guard bytes, the
storage poisoned between bands, the byte offsets through the call's offset arguments.  `twin=True` records the unordered
twin of the same call instead (no order word), for the comparisons with order word 0."""
import numpy as np

from guarded_call import (BAND, FRONT, NEIGHBOURS, TAIL, Sorted, address, ballot_sorter, poisoned_storage, sorter,  # noqa: F401
                          to_device, to_host, torch_mod)
from vulkan_radix_sort_amd import api

ROWS = {call.facts[1:4]: call for call in api.ORDERED_SORT_CALLS}                     # (segmented, indirect, key+value)
TWINS = {call.facts[1:4]: call for call in api.RECORDING_CALLS if call.facts[0] == 32 and call.facts[4] is None}


def ordered_call(torch, sorter, keys, values=None, *, order, offsets=None, count=None, device_count=None, keys_off=0,
                 values_off=0, offsets_off=0, indirect_off=0, storage_off=0, storage=None, pool=None, expect_status=0,
                 expect_refused=False, twin=False, keep_before=False, device="cuda"):
    """keys: uint32, the FULL host array; count: elementCount / maxElementCount (default: all of keys), which also sizes the
    storage requirement; offsets: the segmented calls; device_count: the indirect calls.  The checks are guarded_call's: the
    guard bytes around keys, values, count word and offsets, the bytes in front of the storage offset and behind the
    requirement, the count word and the offsets unchanged, the failure word; expect_refused: the sorter's word is
    STATUS_ENQUEUE_REFUSED and no byte of the storage changed."""
    keys = np.ascontiguousarray(keys, np.uint32)
    facts = (offsets is not None, device_count is not None, values is not None)
    call = (TWINS if twin else ROWS)[facts]
    count = len(keys) if count is None else count
    on_gpu = torch.device(device).type == "cuda"   # (anything else: a sorter that works on host memory, stream 0)
    stream = torch.cuda.current_stream().cuda_stream if on_gpu else 0
    dk = to_device(torch, keys, FRONT + keys_off, TAIL, device)
    dv = do = dc = None
    if values is not None:
        dv = to_device(torch, np.asarray(values).astype(np.uint32), FRONT + values_off, TAIL, device)
    if offsets is not None:
        offsets = np.asarray(offsets).astype(np.uint32)
        do = to_device(torch, offsets, FRONT + offsets_off, NEIGHBOURS, device)
    if device_count is not None:
        dc = to_device(torch, np.array([device_count], np.uint32), FRONT + indirect_off, NEIGHBOURS, device)
    req = sorter.key_value_storage_requirements(count) if values is not None else sorter.storage_requirements(count)
    end = storage_off + req.size
    if storage is None:
        storage = poisoned_storage(torch, req.size, storage_off, device=device)
    assert storage.data_ptr() % 16 == 0 and storage_off % 16 == 0
    before = storage.clone() if keep_before or expect_refused else None
    front, behind = storage[:storage_off].clone(), storage[end:].clone()

    given = {"command_buffer": stream, "element_count": count, "max_element_count": count, "storage": storage.data_ptr(),
             "storage_offset": storage_off, "query_pool": pool, "query": 0, "order": order,
             "segment_count": len(offsets) - 1 if offsets is not None else None}
    for name, t in (("keys", dk), ("values", dv), ("offsets", do), ("indirect", dc)):
        given[name], given[name + "_offset"] = address(t) if t is not None else (None, None)
    getattr(sorter, call.method)(*(given[name] for name, _ in call.parameters))
    if on_gpu:
        torch.cuda.synchronize()

    if expect_refused:
        assert sorter.read_sorter_status(stream) == api.STATUS_ENQUEUE_REFUSED, "a call that must be refused was not"
        bad = torch.nonzero(storage != before).flatten()[:8].tolist()
        assert not bad, f"a refused call wrote to the storage, at bytes {bad}"
    elif count > 0 and (offsets is None or len(offsets) > 1) and expect_status is not None:
        status = sorter.read_status(stream, storage.data_ptr(), storage_off)
        assert status == expect_status, f"the failure word is {status:#x}, not {expect_status:#x}"
    bad = torch.nonzero(storage[:storage_off] != front).flatten()[-8:].tolist()
    assert not bad, f"wrote in front of the storage offset {storage_off}, at bytes {bad}"
    bad = torch.nonzero(storage[end:] != behind).flatten()[:8].tolist()
    assert not bad, f"wrote behind the storage requirement of {req.size} bytes, at {bad} from its end"
    if do is not None:
        assert np.array_equal(to_host(do, guarded=True, what="the offsets"), offsets), "the offsets changed"
    if dc is not None:
        left = int(to_host(dc, guarded=True, what="the count word")[0])
        assert left == device_count, f"the count word changed: {left}, not {device_count}"
    got_keys = to_host(dk, guarded=True, what="the keys")
    got_values = to_host(dv, guarded=True, what="the values") if dv is not None else None
    return Sorted(got_keys, got_values, storage, req.size, before)
