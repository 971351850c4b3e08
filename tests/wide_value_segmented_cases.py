"""What the tests of the segmented sort of 32-bit keys with 64-bit values share (vrdxHipCmdWideValueSortSegmented): the
reference, the segment sizes of each class, the key builders, the values, and a plain-numpy model of the three device forms
with plantable faults (tests/test_wide_value_segmented_cases.py checks reference and model without a GPU;
tests/test_wide_value_segmented_gpu.py holds the device to the same reference on the same cases).

The reference: np.lexsort((keys, segment id)) applied to keys and values -- elements in front of o[0] get the id -1, those from
o[segmentCount] on the id segmentCount, and all of them the key 0, so they stay where they are (the sort is stable).

The model restates the device (vrdx_kernels.hip, "segmented sort of 32-bit keys with 64-bit values"):
  small  segmented_small_wide_kernel: 2 <= n <= 4096 in LDS.  The elements are padded to whole chunks of 256 with key
         0xFFFFFFFF, LAST in memory order; the OR of key ^ key[0] over the REAL elements says which bytes vary; one stable pass
         per varying byte moves key, value low and value high together; the first n slots are stored (none if nothing varies).
         Larger segments are listed: mid up to 8192, large beyond.
  mid    segmented_mid_wide_kernel: the same for the listed segments of 4097 ... 8192 elements; it checks the class again
         and leaves a listed segment of another size alone.
  large  segmented_large_wide_kernel: the listed segments of more than 8192 elements (checked again).  A histogram of the real
         keys says which bytes take two digits at least; every such pass walks the segment in tiles of 8192, each padded like
         above and ranked stably, its sorted position q going to base[d] + q - tileStart[d] if that is < n, and base[]
         advances by the tile's counts; the passes ping-pong between the caller's range and the scratch, an odd number ends
         with a copy back, and with no pass nothing is written.
The model also counts the passes it runs: what a fault may change is (keys, values, passes).
`fault` plants ONE mistake the kernels could make; FAULTS maps each to the classes it can occur in."""
import numpy as np

SMALL_MAX = 4096   # kSegWideSmallMax (vrdx_kernels.h)
MID_MAX = 8192     # kSegWideMidMax
TILE = 8192        # kSegWideLargeTile
ONES = np.uint32(0xFFFFFFFF)
LOW = np.uint64(0xFFFFFFFF)
SHIFT = np.uint64(32)
SCRATCH = np.uint64(0xA5A5A5A5A5A5A5A5)   # what the model's scratch holds on entry

SIZES = {"small": (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096),
         "mid": (4097, 4352, 8191, 8192),     # 4352: 17 chunks, which deal unevenly over 16 waves
         "large": (8193, 8448, 16384, 16385, 24577, 40000)}

FAULTS = {
    "pads-in-mask": ("small", "mid"),             # the pads take part in the mask of varying bytes: passes that move nothing
    "skipped-pass": ("small", "mid", "large"),    # the mask is first ^ last key only: a byte that varies in between is skipped
    "value-words-swapped": ("small", "mid", "large"),   # the store puts the low word on top
    "copy-back-drops-high-word": ("large",),      # the copy back of an odd pass count moves the keys and the low words only
    # base[] is not advanced behind a tile (by its counts, the pads taken off digit 255): the next tile's runs land on this
    # one's.  (The pads' share alone cannot show: only a segment's last tile has pads, and base[] is per pass.)
    "tile-bases-not-advanced": ("large",),
    "unstable-rank": ("small", "mid", "large"),   # within a digit, later elements rank first
    "edge-8192-large": ("mid",),                  # the small kernel lists 8192 as large; the large kernel leaves it alone
    "edge-8193-mid": ("large",),                  # ... and 8193 as mid; the mid kernel leaves it alone
}

BUILDERS = ("random", "byte0", "byte1", "byte2", "byte3", "equal", "bytes02", "bytes012", "ones_third", "two_valued",
            "descending")


def make_keys(builder, n, rng):
    u32 = lambda a: np.asarray(a, np.uint64).astype(np.uint32)   # noqa: E731
    byte = lambda: u32(rng.integers(0, 256, size=n, dtype=np.uint64))   # noqa: E731
    if builder == "random":
        return u32(rng.integers(0, 1 << 32, size=n, dtype=np.uint64))
    if builder.startswith("byte") and len(builder) == 5:     # one byte varies alone
        at = int(builder[4])
        return (byte() << np.uint32(8 * at)) | (np.uint32(0x5AC3A55A) & ~np.uint32(0xFF << (8 * at)))
    if builder == "equal":        # no pass: the values keep their input order
        return np.full(n, 0x12345678, np.uint32)
    if builder == "bytes02":      # an even number of passes
        return byte() | (byte() << np.uint32(16)) | np.uint32(0x7E003C00)
    if builder == "bytes012":     # an odd number: the large form copies back
        return byte() | (byte() << np.uint32(8)) | (byte() << np.uint32(16)) | np.uint32(0x81000000)
    if builder == "ones_third":   # ties with the pads
        k = u32(rng.integers(0, 1 << 32, size=n, dtype=np.uint64))
        k[rng.integers(0, 3, size=n) == 0] = ONES
        return k
    if builder == "two_valued":   # stability shows in the values
        return rng.choice(np.array([0x80000001, 7], np.uint32), size=n)
    if builder == "descending":
        return np.uint32(0xFFFFFFF0) - np.arange(n, dtype=np.uint32) * np.uint32(3)
    raise ValueError(builder)


def make_values(n, rng):
    """never the index: a 64-bit mix of the position with both words random, the halves different"""
    at = np.arange(n, dtype=np.uint64)
    v = rng.integers(0, 1 << 64, size=n, dtype=np.uint64) ^ (at * np.uint64(0x9E3779B97F4A7C15))
    v[(v >> SHIFT) == (v & LOW)] ^= np.uint64(1)
    return v


def offsets_of(sizes, lead=0):
    """CSR offsets of neighbouring segments of these sizes, the first at element `lead`"""
    return (np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]) + lead).astype(np.uint32)


def class_case(size_class, builder, seed=0, lead=5, tail=7):
    """(keys, values, offsets) of one call that holds all sizes of the class as neighbouring segments, every segment built by
    `builder` on its own, `lead` elements in front of the first and `tail` behind the last that no segment covers"""
    rng = np.random.default_rng([seed, BUILDERS.index(builder), sorted(SIZES).index(size_class)])
    sizes = SIZES[size_class]
    parts = [make_keys("random", lead, rng)] + [make_keys(builder, n, rng) for n in sizes] + [make_keys("random", tail, rng)]
    keys = np.concatenate(parts).astype(np.uint32)
    return keys, make_values(len(keys), rng), offsets_of(sizes, lead)


def valid_segments(offsets, bound):
    """(begin, end) of the segments the device sorts: o[i] <= o[i + 1] <= bound"""
    o = np.asarray(offsets, np.int64)
    return [(int(b), int(e)) for b, e in zip(o[:-1], o[1:]) if b <= e <= bound]


def expected(keys, values, offsets, bound=None):
    """The reference.  Monotone offsets inside the bound: one lexsort by (segment id, key).  Otherwise (the tests of bad
    offsets, whose valid segments are disjoint): the same, segment by valid segment."""
    keys, values = np.asarray(keys, np.uint32).copy(), np.asarray(values, np.uint64).copy()
    bound = len(keys) if bound is None else bound
    o = np.asarray(offsets, np.int64)
    if len(o) < 2:
        return keys, values
    if np.all(o[:-1] <= o[1:]) and o[-1] <= bound:
        ids = np.searchsorted(o, np.arange(len(keys)), side="right") - 1   # -1 in front of o[0]; empty segments own nothing
        outside = (np.arange(len(keys)) < o[0]) | (np.arange(len(keys)) >= o[-1])
        ids[np.arange(len(keys)) >= o[-1]] = len(o) - 1
        order = np.lexsort((np.where(outside, 0, keys), ids))   # (stable: equal pairs, and what no segment covers, stay)
        return keys[order], values[order]
    for b, e in valid_segments(o, bound):
        order = np.argsort(keys[b:e], kind="stable")
        keys[b:e], values[b:e] = keys[b:e][order], values[b:e][order]
    return keys, values


def varying_bytes(keys):
    """how many bytes differ between any two of these keys: the passes the device runs on them"""
    keys = np.asarray(keys, np.uint32)
    if len(keys) == 0:
        return 0
    mask = int(np.bitwise_or.reduce(keys ^ keys[0]))
    return sum(1 for shift in (0, 8, 16, 24) if (mask >> shift) & 0xFF)


def _rank_order(digits, fault):
    """the order one ranking pass puts these digits in"""
    if fault == "unstable-rank":
        return np.lexsort((-np.arange(len(digits)), digits))
    return np.argsort(digits, kind="stable")


def _padded(k, lo, hi):
    n = len(k)
    slots = -(-n // 256) * 256
    pk, plo, phi = np.full(slots, ONES, np.uint32), np.full(slots, ONES, np.uint32), np.full(slots, ONES, np.uint32)
    pk[:n], plo[:n], phi[:n] = k, lo, hi
    return pk, plo, phi


def _words(values):
    return (values & LOW).astype(np.uint32), (values >> SHIFT).astype(np.uint32)


def _join(lo, hi, fault):
    if fault == "value-words-swapped":
        lo, hi = hi, lo
    return (hi.astype(np.uint64) << SHIFT) | lo.astype(np.uint64)


def _in_lds(keys, values, fault):
    """one segment in LDS, in place; returns the passes run"""
    n = len(keys)
    k, lo, hi = _padded(keys, *_words(values))
    if fault == "skipped-pass":
        mask = int(k[0] ^ k[n - 1])
    elif fault == "pads-in-mask":
        mask = int(np.bitwise_or.reduce(k ^ k[0]))
    else:
        mask = int(np.bitwise_or.reduce(k[:n] ^ k[0]))
    passes = 0
    for shift in (0, 8, 16, 24):
        if (mask >> shift) & 0xFF:
            order = _rank_order((k >> np.uint32(shift)) & np.uint32(0xFF), fault)
            k, lo, hi = k[order], lo[order], hi[order]
            passes += 1
    if passes:
        keys[:] = k[:n]
        values[:] = _join(lo[:n], hi[:n], fault)
    return passes


def _large(keys, values, fault):
    """one segment through memory, in place; returns the passes run"""
    n = len(keys)
    if fault == "skipped-pass":
        active = [shift for shift in (0, 8, 16, 24) if (int(keys[0] ^ keys[n - 1]) >> shift) & 0xFF]
    else:
        active = [shift for shift in (0, 8, 16, 24) if len(np.unique((keys >> np.uint32(shift)) & np.uint32(0xFF))) > 1]
    src_k, src_v = keys.copy(), values.copy()
    dst_k, dst_v = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, SCRATCH, np.uint64)
    in_caller = True
    for shift in active:
        counts = np.bincount(((src_k >> np.uint32(shift)) & np.uint32(0xFF)).astype(np.int64), minlength=256)
        base = np.concatenate([[0], np.cumsum(counts)[:-1]])
        for t0 in range(0, n, TILE):
            m = min(TILE, n - t0)
            k, lo, hi = _padded(src_k[t0:t0 + m], *_words(src_v[t0:t0 + m]))
            order = _rank_order((k >> np.uint32(shift)) & np.uint32(0xFF), fault)
            k, lo, hi = k[order], lo[order], hi[order]
            d = ((k >> np.uint32(shift)) & np.uint32(0xFF)).astype(np.int64)
            tile_counts = np.bincount(d, minlength=256)
            tile_start = np.concatenate([[0], np.cumsum(tile_counts)[:-1]])
            q = np.arange(m)                       # (the sorted positions behind m are the pads')
            to = base[d[:m]] + q - tile_start[d[:m]]
            ok = to < n
            dst_k[to[ok]] = k[:m][ok]
            dst_v[to[ok]] = _join(lo[:m][ok], hi[:m][ok], None)
            tile_counts[255] -= len(k) - m
            if fault != "tile-bases-not-advanced":
                base = base + tile_counts
        src_k, dst_k, src_v, dst_v = dst_k, src_k, dst_v, src_v
        in_caller = not in_caller
    if not active:
        return 0
    if in_caller:   # an even number of passes: the result lies in the caller's range
        keys[:], values[:] = src_k, src_v
    else:           # the copy back; dst_* is the caller's range as the last but one pass left it
        keys[:] = src_k
        values[:] = (dst_v & ~LOW) | (src_v & LOW) if fault == "copy-back-drops-high-word" else src_v
    if fault == "value-words-swapped":
        values[:] = (values << SHIFT) | (values >> SHIFT)
    return len(active)


def segmented_model(keys, values, offsets, bound=None, fault=None):
    """The call on the FULL arrays.  Returns (keys, values, passes) as the model leaves them, passes = the ranking passes run
    over all segments."""
    keys, values = np.asarray(keys, np.uint32).copy(), np.asarray(values, np.uint64).copy()
    bound = len(keys) if bound is None else bound
    mid_edge = {"edge-8192-large": MID_MAX - 1, "edge-8193-mid": MID_MAX + 1}.get(fault, MID_MAX)   # the small kernel's
    passes = 0
    for b, e in valid_segments(offsets, bound):
        n = e - b
        if n < 2:
            continue
        if n <= SMALL_MAX:
            passes += _in_lds(keys[b:e], values[b:e], fault)
        elif n <= mid_edge:           # listed as mid
            if n <= MID_MAX:          # (the mid kernel's own check)
                passes += _in_lds(keys[b:e], values[b:e], fault)
        elif n > MID_MAX:             # listed as large, and the large kernel's own check
            passes += _large(keys[b:e], values[b:e], fault)
    return keys, values, passes
