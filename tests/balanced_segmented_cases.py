"""The device form of the balanced segmented sort (vrdxHipCmdBalancedSortSegmented[KeyValue]) in
numpy, for tests/test_balanced_segmented_cases.py (no GPU) and tests/test_balanced_segmented_gpu.py: the split rule, the
pieces, and count, scan, scatter and copy back per spread segment, on a caller's array and a scratch array, with the mask of
active passes kept per segment.  `fault` plants one of the mistakes the form invites:

  1  counts taken once up front (from the input) instead of again in every pass
  2  bases that ignore the segment's earlier pieces
  3  bases relative to the array instead of the segment
  4  one mask for the whole call instead of one per segment
  5  copy back decided by 4 instead of by the number of active passes
  6  base[] not advanced between the tiles of a piece
  7  a piece that ends at begin + L instead of at the segment's end
  8  the share taken from totalSpread instead of totalLarge (shows in the split words, not in the keys)

`cases(cus)` are the inputs both test files run, sized by the CU count."""
import numpy as np

SPREAD_FROM = 65536
SPREAD_SHARES = 3
PIECE_MIN = 16384
TILE = 16384       # kSegLargeTile
LISTED_ABOVE = 16384
FAULTS = tuple(range(1, 9))
MAX_ELEMENTS = (1 << 30) - 4


def spread_cap(n, cus):
    return min(n // (SPREAD_FROM + 1), min((cus - 1) // SPREAD_SHARES, 256) if cus else 0)


def piece_cap(n, cus):
    s = spread_cap(n, cus)
    return min(cus, n // PIECE_MIN) + s if s else 0


def layout(n, cus, address=0, align=16):
    """MakeBalancedSegmentedLayout (vrdx_layout.h): byte offsets from the storage's first byte"""
    def up(a, b):
        return (a + b - 1) // b * b
    table_end = up(4, align) + 4 * 4 * 256
    lists = table_end + (-(address + table_end) & 127)
    mid_cap, large_cap = n // 4097, n // 16385
    out = {"midList": lists, "largeList": lists + 4 * mid_cap}
    out["restList"] = out["largeList"] + 4 * large_cap
    out["split"] = out["restList"] + 4 * large_cap
    out["spreadTable"] = out["split"] + 4 * 8
    out["pieceTable"] = out["spreadTable"] + 4 * 8 * spread_cap(n, cus)
    end = out["pieceTable"] + 4 * 4 * piece_cap(n, cus)
    out["rows"] = end + (-(address + end) & 127)
    out["keysScratch"] = out["rows"] + 1024 * piece_cap(n, cus)
    out["valuesScratch"] = out["keysScratch"] + up(4 * n, 128)
    return out


def split(offsets, cus, fault=None):
    """(listed, [(begin, end) of every spread segment, in offset order], L)"""
    offsets = np.asarray(offsets, dtype=np.int64)
    begins, ends = offsets[:-1], offsets[1:]
    lengths = ends - begins
    listed = lengths > LISTED_ABOVE
    total_large = int(lengths[listed].sum())
    if fault == 8:
        total_large = int(lengths[lengths > SPREAD_FROM].sum())
    share = -(-total_large // cus)
    spread = listed & (lengths > max(SPREAD_FROM, SPREAD_SHARES * share))
    total_spread = int(lengths[spread].sum())
    piece = max(PIECE_MIN, -(-(-(-total_spread // cus)) // 256) * 256)
    return int(listed.sum()), [(int(b), int(e)) for b, e in zip(begins[spread], ends[spread])], piece


def split_words(offsets, cus, fault=None):
    """what vrdxHipReadBalancedSplit returns: listed segments, spread segments, pieces, L"""
    listed, spread, piece = split(offsets, cus, fault)
    return listed, len(spread), sum(-(-(e - b) // piece) for b, e in spread), piece


def _digit(keys, p):
    return (keys >> np.uint32(8 * p)) & np.uint32(0xFF)


def sort_model(keys, values, offsets, cus, fault=None):
    """(keys, values, touched) after the call: the spread segments by the device form, every other segment by a stable sort;
    touched[i]: the scratch arrays were written at index i by a spread segment's pass."""
    keys = np.array(keys, dtype=np.uint32)
    values = None if values is None else np.array(values, dtype=np.uint32)
    n = len(keys)
    a = [keys, values if values is not None else np.zeros(n, np.uint32)]
    s = [np.zeros(n, np.uint32), np.zeros(n, np.uint32)]
    touched = np.zeros(n, dtype=bool)
    _, spread, piece_len = split(offsets, cus, fault)
    spread_set = set(spread)
    for b, e in zip(np.asarray(offsets[:-1], dtype=np.int64), np.asarray(offsets[1:], dtype=np.int64)):
        if (int(b), int(e)) in spread_set or e - b < 2:
            continue
        order = np.argsort(a[0][b:e], kind="stable")
        a[0][b:e] = a[0][b:e][order]
        a[1][b:e] = a[1][b:e][order]
    pieces = {}
    for b, e in spread:
        cut = []
        for k in range(-(-(e - b) // piece_len)):
            stop = b + (k + 1) * piece_len
            cut.append((b + k * piece_len, min(stop, n) if fault == 7 else min(stop, e)))
        pieces[(b, e)] = cut
    masks = {seg: 0 for seg in spread}
    first_counts = {seg: [[np.bincount(_digit(keys[pb:pe], p), minlength=256) for pb, pe in pieces[seg]] for p in range(4)]
                    for seg in spread} if fault == 1 else None

    def mask_of(seg):
        if fault == 4:
            shared = 0
            for m in masks.values():
                shared |= m
            return shared
        return masks[seg]

    def reads_scratch(seg, p):
        return bin(mask_of(seg) & ((1 << p) - 1)).count("1") & 1

    for p in range(4):
        rows = {}
        for seg in spread:   # count
            src = s if reads_scratch(seg, p) else a
            rows[seg] = (first_counts[seg][p] if fault == 1 else
                         [np.bincount(_digit(src[0][pb:pe], p), minlength=256) for pb, pe in pieces[seg]])
        positions = {}
        for seg in spread:   # scan
            b, e = seg
            total = np.sum(rows[seg], axis=0)
            positions[seg] = [r.astype(np.int64) for r in rows[seg]]   # a scan that returns leaves the counts
            if not np.any((total != 0) & (total != e - b)):
                continue
            masks[seg] |= 1 << p
            start = np.concatenate([[0], np.cumsum(total)[:-1]]) + (0 if fault == 3 else b)
            run = start.astype(np.int64)
            positions[seg] = []
            for r in rows[seg]:
                positions[seg].append(start.astype(np.int64).copy() if fault == 2 else run.copy())
                run = run + r
        sides = {seg: reads_scratch(seg, p) for seg in spread}
        active = {seg: (mask_of(seg) >> p) & 1 for seg in spread}
        for seg in spread:   # scatter
            if not active[seg]:
                continue
            b, e = seg
            src, dst = (s, a) if sides[seg] else (a, s)
            writes = []
            for (pb, pe), base in zip(pieces[seg], positions[seg]):
                base = base.copy()
                for t0 in range(pb, pe, TILE):
                    t1 = min(t0 + TILE, pe)
                    d = _digit(src[0][t0:t1], p).astype(np.int64)
                    order = np.argsort(d, kind="stable")
                    counts = np.bincount(d, minlength=256)
                    tile_start = np.concatenate([[0], np.cumsum(counts)[:-1]])
                    sorted_d = d[order]
                    to = base[sorted_d] + np.arange(t1 - t0) - tile_start[sorted_d]
                    ok = (to >= b) & (to < e)
                    writes.append((to[ok], src[0][t0:t1][order][ok], src[1][t0:t1][order][ok]))
                    if fault != 6:
                        base += counts
            for to, k, v in writes:   # (every piece reads the side as the pass found it)
                dst[0][to] = k
                dst[1][to] = v
                if dst is s:
                    touched[to] = True
    for seg in spread:   # copy back
        b, e = seg
        odd = 0 if fault == 5 else bin(mask_of(seg) & 0xF).count("1") & 1
        if odd:
            a[0][b:e] = s[0][b:e]
            a[1][b:e] = s[1][b:e]
    return a[0], (a[1] if values is not None else None), touched


def reference(keys, values, offsets):
    """np.lexsort((keys, segment id)) on the elements inside [offsets[0], offsets[-1]); the rest stays"""
    keys = np.array(keys, dtype=np.uint32)
    offsets = np.asarray(offsets, dtype=np.int64)
    lo, hi = int(offsets[0]), int(offsets[-1])
    ids = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    order = np.lexsort((keys[lo:hi], ids)) + lo
    out_k = keys.copy()
    out_k[lo:hi] = keys[order]
    out_v = None
    if values is not None:
        out_v = np.array(values, dtype=np.uint32)
        out_v[lo:hi] = out_v[order]
    return out_k, out_v


def _keys(rng, n, kind):
    if kind == "uniform":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "bits24":
        return rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32)
    if kind == "two_bytes":   # bytes 1 and 3 vary
        return ((rng.integers(0, 256, n, dtype=np.uint64) << 8) | (rng.integers(0, 256, n, dtype=np.uint64) << 24) | 0x00110022).astype(np.uint32)
    if kind == "one_byte":    # byte 2 varies
        return ((rng.integers(0, 256, n, dtype=np.uint64) << 16) | 0x5A0000C3).astype(np.uint32)
    if kind == "equal":
        return np.full(n, 0xDEADBEEF, dtype=np.uint32)
    if kind == "first_tile_one_digit":
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        k[:TILE] = (k[:TILE] & np.uint32(0xFFFFFF00)) | np.uint32(0x7E)
        return k
    if kind == "ones":        # the pads' own value among the keys
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        k[rng.random(n) < 0.5] = 0xFFFFFFFF
        return k
    if kind == "few":
        return rng.choice(np.array([3, 0x80000000, 0x01000000, 0xFFFFFFFF, 0x00010000], dtype=np.uint32), n)
    raise ValueError(kind)


PASS_KINDS = ("uniform", "bits24", "two_bytes", "one_byte", "equal", "first_tile_one_digit", "ones", "few")


def cases(cus, seed=20261021):
    """name -> (keys, values, offsets): values are random, never the index; offsets[0] may be above 0 and offsets[-1] below
    len(keys)"""
    rng = np.random.default_rng(seed)
    out = {}

    def add(name, lengths, kinds=None, lead=0, tail=0):
        lengths = list(lengths)
        kinds = kinds or ["uniform"] * len(lengths)
        offsets = np.concatenate([[lead], lead + np.cumsum(lengths)]).astype(np.int64)
        n = int(offsets[-1]) + tail
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        for b, length, kind in zip(offsets[:-1], lengths, kinds):
            keys[b:b + length] = _keys(rng, length, kind)
        values = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        out[name] = (keys, values, offsets)

    add("n65536", [65536])
    add("n65537", [65537])                          # five pieces, the last of one key
    add("k_quarter", [70001] * (cus // 4))          # 3 shares = 0.75 of a segment: spread
    add("k_half", [70001] * (cus // 2))             # 3 shares = 1.5 segments: not spread
    add("one_among", [50000] * (cus // 2) + [131072] + [50000] * (cus - cus // 2))   # totalLarge sets the share: not spread
    add("one_among_spread", [50000] * (cus // 2) + [262144] + [50000] * (cus - cus // 2))
    add("two_tiles", [2 * cus * 16384 + 257])       # L > 16384, more than one tile per piece
    for r in range(4):                              # the spread segment's begin at every residue mod 4
        add(f"neighbours{r}", [100, 5000, 20000, 65536 + 1000 + r, 17000, 3, 70000, 4097], lead=r, tail=5)
    add("passes", [66000 + 37 * i for i in range(len(PASS_KINDS))], PASS_KINDS, lead=1, tail=3)
    return out
