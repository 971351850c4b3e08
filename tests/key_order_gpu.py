"""What the GPU tests of the key orders of the 64-bit sorts share (tests/test_sort64_ordered_gpu.py,
tests/test_segmented64_ordered_gpu.py): one guarded call of vrdxHipCmdSort64Ordered[KeyValue][Indirect] and one of
vrdxHipCmdSortSegmented64Ordered[KeyValue].  The guard schemes are those of run64 / run64_indirect (tests/test_sort64_gpu.py,
tests/test_sort64_indirect_gpu.py) and of run_segmented64 (tests/segmented64_cases.py), with the order word passed on."""
import numpy as np

from segmented64_cases import GUARD64, _dev64, _host64
from segmented_cases import GUARD as GUARD32
from segmented_cases import _dev, _host, ballot_sorter, sorter, torch_mod  # noqa: F401
from test_sort64_gpu import GUARD, STORAGE_GUARD, _guarded, _unguard


def run64_ordered(torch, s, keys, values, word, *, count=None, device_count=None, keys_off=0, values_off=0, storage_off=0,
                  pool=None, storage_out=None, expect_refused=False):
    """One call through the C ABI with the order word `word`.  count (default: all of keys) is the elementCount, or with
    device_count the bound, the count then being read from a device word between guard words.  The rest of `keys` / `values`
    and 256 bytes more are guard bytes, the storage holds the requirement of the count (bound) between guard bytes.  Returns
    the whole arrays as the device left them."""
    import vulkan_radix_sort_amd as vrdx
    stream = torch.cuda.current_stream().cuda_stream
    n = len(keys) if count is None else count
    key_value = values is not None
    required = s.storage_requirements64(n, key_value).size
    storage = torch.full((storage_off + required + 256,), STORAGE_GUARD, dtype=torch.uint8, device="cuda")
    assert storage.data_ptr() % 16 == 0 and storage_off % 16 == 0 and keys_off % 8 == 0 and values_off % 4 == 0
    dk = _guarded(torch, keys, keys_off, 256)
    dv = _guarded(torch, values, values_off, 256) if key_value else None
    if device_count is not None:
        words = np.array([0xA5A5A5A5, device_count, 0xA5A5A5A5], dtype=np.uint32)
        indirect = torch.from_numpy(words.view(np.uint8).copy()).cuda()
        if key_value:
            s.cmd_sort64_ordered_key_value_indirect(stream, n, indirect.data_ptr(), 4, dk.data_ptr(), keys_off, dv.data_ptr(),
                                                    values_off, word, storage.data_ptr(), storage_off, pool, 0)
        else:
            s.cmd_sort64_ordered_indirect(stream, n, indirect.data_ptr(), 4, dk.data_ptr(), keys_off, word, storage.data_ptr(),
                                          storage_off, pool, 0)
    elif key_value:
        s.cmd_sort64_ordered_key_value(stream, n, dk.data_ptr(), keys_off, dv.data_ptr(), values_off, word, storage.data_ptr(),
                                       storage_off, pool, 0)
    else:
        s.cmd_sort64_ordered(stream, n, dk.data_ptr(), keys_off, word, storage.data_ptr(), storage_off, pool, 0)
    torch.cuda.synchronize()
    if expect_refused:
        assert s.read_sorter_status(stream) == vrdx.STATUS_ENQUEUE_REFUSED
        assert bool((storage == STORAGE_GUARD).all()), "a refused call wrote to the storage"
    else:
        if n > 0:  # (an empty call writes no header)
            assert s.read_status(stream, storage.data_ptr(), storage_off) == 0
        assert s.read_sorter_status(stream) == 0
        assert (storage[:storage_off].cpu().numpy() == STORAGE_GUARD).all(), "the storage in front of storageOffset was written"
        assert (storage[storage_off + required:].cpu().numpy() == STORAGE_GUARD).all(), "wrote behind the storage requirement"
    if device_count is not None:
        assert np.array_equal(indirect.cpu().numpy().view(np.uint32), words), "the count word or its neighbours were written"
    got_keys = _unguard(dk, keys_off, keys.nbytes, np.uint64)
    got_values = _unguard(dv, values_off, values.nbytes, np.uint32) if key_value else None
    if storage_out is not None:
        storage_out.append(storage)
    return got_keys, got_values


def run_segmented64_ordered(torch, s, keys, offsets, values, word, *, keys_off=0, values_off=0, storage_off=0, guard=256,
                            pool=None, expect_status=0, expect_refused=False, storage_out=None):
    """One vrdxHipCmdSortSegmented64Ordered[KeyValue] with maxElementCount = len(keys), guarded like run_segmented64: guard
    words in front of the arrays and behind maxElementCount, a guard band behind the storage requirement, the offsets
    checked to be what they were, the failure word compared with expect_status.  Returns keys and values as the device left
    them."""
    import vulkan_radix_sort_amd as vrdx
    n = len(keys)
    stream = torch.cuda.current_stream().cuda_stream
    kw, vw = guard + keys_off // 8, guard + values_off // 4
    kb = np.full(kw + n + guard, GUARD64, np.uint64)
    kb[kw:kw + n] = keys
    dk = _dev64(torch, kb)
    dv = None
    if values is not None:
        vb = np.full(vw + n + guard, GUARD32, np.uint32)
        vb[vw:vw + n] = values
        dv = _dev(torch, vb)
    ob = np.full(len(offsets) + 4, GUARD32, np.uint32)
    ob[:len(offsets)] = np.asarray(offsets, dtype=np.uint32)
    do = _dev(torch, ob)
    req = s.storage_requirements64(n, key_value=values is not None).size
    storage = torch.full((storage_off + req + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    storage[storage_off + req:] = 0x5A
    assert storage.data_ptr() % 16 == 0 and storage_off % 16 == 0
    before = storage.clone()
    if values is None:
        s.cmd_sort_segmented64_ordered(stream, n, len(offsets) - 1, do.data_ptr(), 0, dk.data_ptr(), 8 * kw, word,
                                       storage.data_ptr(), storage_off, pool, 0)
    else:
        s.cmd_sort_segmented64_ordered_key_value(stream, n, len(offsets) - 1, do.data_ptr(), 0, dk.data_ptr(), 8 * kw,
                                                 dv.data_ptr(), 4 * vw, word, storage.data_ptr(), storage_off, pool, 0)
    torch.cuda.synchronize()
    if expect_refused:
        assert s.read_sorter_status(stream) == vrdx.STATUS_ENQUEUE_REFUSED
        assert torch.equal(storage, before), "a refused call wrote to the storage"
    else:
        status = s.read_status(stream, storage.data_ptr(), storage_off)
        assert status == expect_status, (status, expect_status)
        assert s.read_sorter_status(stream) == expect_status
        assert torch.equal(storage[:storage_off], before[:storage_off]), "wrote in front of the storage offset"
        assert torch.equal(storage[storage_off + req:], before[storage_off + req:]), "wrote past the storage requirement"
    assert np.array_equal(_host(do), ob), "the offsets changed"
    hk = _host64(dk)
    assert (hk[:kw] == GUARD64).all(), "wrote in front of the keys"
    assert (hk[kw + n:] == GUARD64).all(), "wrote behind maxElementCount (keys)"
    gk, gv = hk[kw:kw + n].copy(), None
    if dv is not None:
        hv = _host(dv)
        assert (hv[:vw] == GUARD32).all(), "wrote in front of the values"
        assert (hv[vw + n:] == GUARD32).all(), "wrote behind maxElementCount (values)"
        gv = hv[vw:vw + n].copy()
    if storage_out is not None:
        storage_out.append(storage)
    return gk, gv


def assert_same(got_keys, got_values, want, what=""):
    assert np.array_equal(got_keys, want[0]), f"{what}: keys"
    if got_values is not None:
        assert np.array_equal(got_values, want[1]), f"{what}: values"
