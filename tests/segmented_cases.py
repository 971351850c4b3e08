"""What the GPU tests of the segmented sort share (tests/test_segmented_gpu.py, tests/test_segmented_reuse_gpu.py): the
sorters of both ranking forms, key and payload patterns, the reference -- np.lexsort((keys, segment id)) over the whole
call -- and the guarded call of the segmented sorts.  A plain module next to plan_model.py, imported the same way; the
fixtures are those of guarded_call.py."""
import numpy as np

from guarded_call import ballot_sorter, guarded_call, sorter, torch_mod  # noqa: F401 (fixtures, re-exported)

GUARD = 0x5A5A5A5A   # the word tests put around arrays they lay out themselves


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


def run_segmented(torch, sorter, keys, offsets, values=None, *, guard=256, bit_range=None, **kw):
    """One vrdxHipCmdSortSegmented[64][Bits][KeyValue] with maxElementCount = len(keys) (guarded_call: keys_off, values_off,
    offsets_off, storage_off, pool, expect_status, storage), `guard` guard elements behind the keys and the values; the
    failure word is read after every call.  Returns the keys and values as sorted by the device and the storage tensor."""
    got = guarded_call(torch, sorter, keys, values, offsets=offsets, bit_range=bit_range, tail=keys.itemsize * guard,
                       recorded=True, **kw)
    return got.keys, got.values, got.storage


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
