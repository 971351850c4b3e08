"""What the GPU tests of the segmented sort share (tests/test_segmented_gpu.py, tests/test_segmented_reuse_gpu.py): the
sorters of both ranking forms, key and payload patterns, the reference -- np.lexsort((keys, segment id)) over the whole
call -- and one guarded call of vrdxHipCmdSortSegmented[KeyValue].  A plain module next to plan_model.py, imported the same
way; the fixtures are module-scoped, so every test file that imports them gets sorters of its own."""
import os

import numpy as np
import pytest

GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    return torch


@pytest.fixture(scope="module")
def sorter(torch_mod):
    import vulkan_radix_sort_amd as vrdx
    s = vrdx.Sorter()
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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def make_keys(kind, n, rng):
    if kind == "uniform":
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if kind == "all-equal":
        return np.full(n, 0xC0FFEE11, np.uint32)
    if kind == "descending":
        return (np.uint32(0xFFFFFFF0) - np.arange(n, dtype=np.uint32)).astype(np.uint32)
    if kind == "8-bit":
        return rng.integers(0, 256, size=n, dtype=np.uint64).astype(np.uint32)
    if kind == "24-bit":
        return rng.integers(0, 1 << 24, size=n, dtype=np.uint64).astype(np.uint32)
    # 0xFFFFFFFF is the pad of LoadStriped in every size class: real keys equal to it stay in front of the pads, in order
    if kind == "all-sentinel":
        return np.full(n, 0xFFFFFFFF, np.uint32)
    uniform = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if kind == "eighth-sentinel":
        return np.where(rng.integers(0, 8, size=n) == 0, np.uint32(0xFFFFFFFF), uniform).astype(np.uint32)
    if kind == "few-distinct":
        return np.array([0xFFFFFFFF, 0, 0x80000001, 0x7FFFFF00], np.uint32)[rng.integers(0, 4, size=n)]
    if kind.startswith("digit") and kind.endswith("-constant"):  # digit p the same in every key: pass p is skipped
        return uniform & np.uint32(~(0xFF << (8 * int(kind[5]))) & 0xFFFFFFFF)
    if kind == "bytes12-constant":  # passes 0 and 3 move keys, 1 and 2 are skipped: two passes, no copy back
        return (uniform & np.uint32(0xFF0000FF)) | np.uint32(0x00A5C300)
    if kind == "byte0-only":  # one pass, the lowest
        return (uniform & np.uint32(0xFF)) | np.uint32(0x12345600)
    if kind == "byte3-only":  # one pass, the highest
        return (uniform & np.uint32(0xFF000000)) | np.uint32(0x00123456)
    if kind.startswith("tile-digit"):  # the first tile of the large path holds one value of digit p, the rest is mixed
        p = int(kind[10])
        uniform[:16384] = (uniform[:16384] & np.uint32(~(0xFF << (8 * p)) & 0xFFFFFFFF)) | np.uint32(0x5A << (8 * p))
        return uniform
    raise ValueError(kind)


def payload(n):
    """Values with the top bit set, all different (the result shows the order equal keys came out in), a 0xFFFFFFFF and a
    0 (the value LoadStriped pads with) among them."""
    v = np.arange(n, dtype=np.uint32) ^ np.uint32(0x80000000)
    if n > 1:
        v[n // 3] = 0xFFFFFFFF
        v[(2 * n) // 3 + (n // 3 == (2 * n) // 3)] = 0
    return v


def expected(keys, values, offsets, max_count):
    """Every valid segment (o[i] <= o[i+1] <= max_count) stably sorted on its own, everything else as it was."""
    ek, ev = keys.copy(), (values.copy() if values is not None else None)
    o = np.asarray(offsets, dtype=np.int64)
    lengths = np.diff(o)
    if len(o) > 1 and (lengths >= 0).all() and o[-1] <= max_count:
        lo, hi = int(o[0]), int(o[-1])
        seg = np.repeat(np.arange(len(lengths)), lengths)
        order = np.lexsort((keys[lo:hi], seg))
        ek[lo:hi] = keys[lo:hi][order]
        if values is not None:
            ev[lo:hi] = values[lo:hi][order]
        return ek, ev
    for b, e in zip(o[:-1], o[1:]):
        if b <= e <= max_count:
            order = np.argsort(keys[b:e], kind="stable")
            ek[b:e] = keys[b:e][order]
            if values is not None:
                ev[b:e] = values[b:e][order]
    return ek, ev


def run_segmented(torch, sorter, keys, offsets, values=None, *, keys_off=0, values_off=0, offsets_off=0, storage_off=0,
                  guard=256, pool=None, expect_status=0, storage=None):
    """One vrdxHipCmdSortSegmented[KeyValue] with maxElementCount = len(keys): the keys (values) sit `*_off` bytes into
    buffers that carry `guard` words of GUARD behind maxElementCount, the storage has a guard band behind its requirement;
    every guard, the bytes in front of the offsets and the offsets themselves are checked afterwards.  Returns the keys and
    values as sorted by the device and the storage tensor."""
    n = len(keys)
    stream = torch.cuda.current_stream().cuda_stream

    def buffer(a, off):
        w = off // 4
        buf = np.full(w + n + guard, GUARD, np.uint32)
        buf[w:w + n] = a
        return _dev(torch, buf)

    dk = buffer(keys, keys_off)
    dv = buffer(values, values_off) if values is not None else None
    ob = np.full(offsets_off // 4 + len(offsets) + 4, GUARD, np.uint32)
    ob[offsets_off // 4:offsets_off // 4 + len(offsets)] = np.asarray(offsets, dtype=np.uint32)
    do = _dev(torch, ob)
    req = (sorter.key_value_storage_requirements(n) if values is not None else sorter.storage_requirements(n)).size
    if storage is None:
        storage = torch.full((storage_off + req + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        storage[storage_off + req:] = 0x5A
    end = storage_off + req
    front = storage[:storage_off].clone()
    behind = storage[end:].clone()
    if values is None:
        sorter.cmd_sort_segmented(stream, n, len(offsets) - 1, do.data_ptr(), offsets_off, dk.data_ptr(), keys_off,
                                  storage.data_ptr(), storage_off, pool, 0)
    else:
        sorter.cmd_sort_segmented_key_value(stream, n, len(offsets) - 1, do.data_ptr(), offsets_off, dk.data_ptr(),
                                            keys_off, dv.data_ptr(), values_off, storage.data_ptr(), storage_off, pool, 0)
    torch.cuda.synchronize()
    assert sorter.read_status(stream, storage.data_ptr(), storage_off) == expect_status
    assert bool((storage[:storage_off] == front).all()), "wrote in front of the storage offset"
    assert bool((storage[end:] == behind).all()), "wrote past the storage requirement"
    assert np.array_equal(_host(do), ob), "the offsets changed"
    outs = []
    for d, off in ((dk, keys_off), (dv, values_off)):
        if d is None:
            outs.append(None)
            continue
        h = _host(d)
        w = off // 4
        assert (h[:w] == GUARD).all(), "wrote in front of the keys / values offset"
        assert (h[w + n:] == GUARD).all(), "wrote behind maxElementCount"
        outs.append(h[w:w + n].copy())
    return outs[0], outs[1], storage


def check(got_k, got_v, keys, values, offsets, oracle=None, want=None):
    """`want`: expected(keys, values, offsets, len(keys)) where the caller has it already (the same lexsort serves the
    keys-only and the key+value run of one case)."""
    ek, ev = want if want is not None else expected(keys, values, offsets, len(keys))
    assert np.array_equal(got_k, ek)
    if values is not None:
        assert np.array_equal(got_v, ev)
    if oracle is not None:  # the checker's own sort, segment by segment, for the in-LDS sizes
        for b, e in zip(offsets[:-1], offsets[1:]):
            if 0 < e - b <= 16385:
                ok, ov, _ = oracle.sort(keys[b:e].copy(), values[b:e].copy() if values is not None else None)
                assert np.array_equal(got_k[b:e], ok)
                if values is not None:
                    assert np.array_equal(got_v[b:e], ov)


def mixed_offsets(rng, sizes, head=100, tail=77):
    sizes = list(sizes)
    rng.shuffle(sizes)
    offsets = head + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return offsets.astype(np.uint32), int(offsets[-1]) + tail
