"""What the GPU tests of the segmented sort of 64-bit keys share (tests/test_segmented64_gpu.py): key patterns; the guarded
call is segmented_cases.run_segmented, which takes the key width from the keys' dtype.  The sorters of both ranking forms,
the payloads, the reference -- np.lexsort((keys, segment id)) over the whole call -- and the offset builder are those of
segmented_cases.py, which works on keys of any width.  A plain module, imported the same way."""
import numpy as np

from segmented_cases import run_segmented as run_segmented64   # (the key width is the keys' dtype)

ONES = 0xFFFFFFFFFFFFFFFF

SMALL_MAX = 4096
MID_MAX = 16384            # keys-only
MID_MAX_KEY_VALUE = 8192   # key+value
LARGE_TILE = 8192


def uniform64(n, rng):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


def make_keys64(kind, n, rng):
    u = uniform64(n, rng)
    if kind == "uniform":
        return u
    if kind == "all-equal":
        return np.full(n, 0xC0FFEE11DEADBEEF, np.uint64)
    if kind == "descending":
        return np.uint64(0xFFFFFFFFFFFFFFF0) - np.arange(n, dtype=np.uint64) * np.uint64(0x100000001)
    if kind == "low-word-only":  # the high word is constant
        return (u & np.uint64(0xFFFFFFFF)) | np.uint64(0x0123456700000000)
    if kind == "high-word-only":
        return (u & np.uint64(0xFFFFFFFF00000000)) | np.uint64(0x89ABCDEF)
    if kind == "tile_depth":  # a 16-bit tile id over the bits of a positive float depth
        tile = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
        depth = (rng.random(n, dtype=np.float32) * np.float32(100.0) + np.float32(0.1)).view(np.uint32).astype(np.uint64)
        return (tile << np.uint64(32)) | depth
    # all ones is the pad in every size class: real keys equal to it stay in front of the pads, in order
    if kind == "all-ones":
        return np.full(n, ONES, np.uint64)
    if kind == "eighth-ones":
        return np.where(rng.integers(0, 8, size=n) == 0, np.uint64(ONES), u)
    if kind == "few-distinct":
        return np.array([0, 1 << 63, (1 << 32) - 1, 1 << 32, ONES, 0x8000000000000001], np.uint64)[rng.integers(0, 6, size=n)]
    if kind.startswith("byte") and kind.endswith("-constant"):  # byte p the same in every key: pass p is skipped
        p = int(kind[4])
        return (u & np.uint64(ONES ^ (0xFF << (8 * p)))) | np.uint64(0xA5 << (8 * p))
    if kind.startswith("only-byte"):  # one pass
        p = int(kind[9])
        return (u & np.uint64(0xFF << (8 * p))) | np.uint64(0x1122334455667788 & (ONES ^ (0xFF << (8 * p))))
    if kind == "word-boundary":
        # duplicates throughout; a third of the keys differ in the low word only, a third in the high word only
        lo = rng.integers(0, 5, size=n, dtype=np.uint64) * np.uint64(0x01000001)
        hi = rng.integers(0, 5, size=n, dtype=np.uint64) * np.uint64(0x01000001)
        which = rng.integers(0, 3, size=n)
        lo = np.where(which == 1, np.uint64(7), lo)
        hi = np.where(which == 0, np.uint64(7), hi)
        return (hi << np.uint64(32)) | lo
    if kind.startswith("tile-byte"):  # the first 16384 elements hold one value of byte p, the rest is mixed
        p = int(kind[9])
        u[:16384] = (u[:16384] & np.uint64(ONES ^ (0xFF << (8 * p)))) | np.uint64(0x5A << (8 * p))
        return u
    raise ValueError(kind)


def both_forms(torch, sorter, keys, offsets, values, want=None, **kw):
    """The keys-only and the key+value run of one case against one reference."""
    from segmented_cases import expected
    ek, ev = want if want is not None else expected(keys, values, offsets, len(keys))
    gk, _, _ = run_segmented64(torch, sorter, keys, offsets, **kw)
    assert np.array_equal(gk, ek), "keys-only"
    gk, gv, _ = run_segmented64(torch, sorter, keys, offsets, values, **kw)
    assert np.array_equal(gk, ek), "key+value: keys"
    assert np.array_equal(gv, ev), "key+value: values"
