"""What the tests of the range sorts at every size (vrdxHipCmdRangeSort[KeyValue][Indirect]) share: the cases the GPU tests
run, as functions of the device's CU count; key builders whose bits outside the range are random; and a plain-numpy model of
the chunked form with plantable faults (tests/test_range_sort_cases.py checks the model without a GPU;
tests/test_range_sort_gpu.py runs the device against np.argsort(field, kind="stable") on the same cases).

The chunked form (vrdx_kernels.hip, "range sort"), restated: the array is cut into `grid` contiguous
chunks of chunk_keys keys; for every digit p of the field whose totals show two values at least (an ACTIVE pass) a count
launch counts the digit per chunk IN THE ARRAY THE PASS READS, a scan launch turns the counts into positions
digitStart[d] + the counts of d in the chunks in front, and a scatter launch walks each chunk in tiles of 16384 keys, in
order: stable rank inside the tile, key to base[d] + (its rank among the tile's keys of digit d), then base[d] += the tile's
count of d.  A tile is padded to a multiple of 256 keys with keys of all ones, whose digit is 2^w - 1 in a digit of w bits
and which are taken out of that bin again.  The passes alternate between the caller's arrays and the scratch arrays; an odd
number of ACTIVE passes ends with a copy back.  `fault` plants ONE mistake the kernels could make.
"""
import zlib

import numpy as np

import sort_bits_cases

FAULTS = ("stale-counts",      # 1: per-chunk counts taken from the input in a later pass
          "bases-ignore-chunks",  # 2: a chunk's positions ignore the chunks in front of it
          "base-not-advanced",  # 3: base[] not advanced between the tiles of a chunk
          "copy-back-by-digits",  # 4: the copy back decided by P, not by the number of active passes
          "last-digit-wide",   # 5: the last digit one bit too wide
          "pad-digit-255",     # 6: the pads counted in (and taken out of) bin 255 of a narrow digit
          "scan-by-bound")     # 7: the indirect form's scan chunking by the bound instead of the count

TILE = 16384             # kSegLargeTile
ONE_WORKGROUP_MAX = 16384  # kSmallSortMaxElements
CHUNK_MIN = 8192         # kRangeChunkMinKeys

RANGES = [(0, 1), (31, 32), (0, 8), (5, 14), (8, 24), (4, 28), (1, 32)]
LARGE_RANGES = [(5, 14), (8, 24), (4, 28)]   # one digit and a bit, two digits, three
EMPTY_RANGE = (13, 13)
FULL_RANGE = (0, 32)
INVALID_RANGES = [(9, 8), (0, 33)]
BUILDERS = ["uniform", "few", "const-mid", "const-low", "equal", "ones-mixed"]
LARGE_BUILDERS = ["uniform", "const-mid"]
SMALL_SIZES = [16385, 16385 + 255, 65539]
CROSS_PRODUCT_SIZES = [16385, 65539]
INDIRECT_COUNTS = ("0", "1", "16384", "16385", "bound-1", "bound", "bound+7")

field = sort_bits_cases.field
payload = sort_bits_cases.payload
reference = sort_bits_cases.reference
digits_of = sort_bits_cases.digits_of


def large_sizes(cus):
    """either side of one chunk of 8192 keys per CU, the first two-tile chunks, three tiles per chunk"""
    return [cus * 8192 - 1, cus * 8192 + 1, cus * 16384, cus * 16384 + 1, 2 * cus * 16384 + 257]


def indirect_bound(cus):
    return cus * 16384 + 1


def indirect_count(name, bound):
    return int(name) if name.isdigit() else {"bound-1": bound - 1, "bound": bound, "bound+7": bound + 7}[name]


def gpu_cases(cus):
    """(n, builder, (begin, end)) of every parity case tests/test_range_sort_gpu.py runs on a device of `cus` CUs: the full
    cross product at two small sizes, uniform keys over every range at the third, uniform and constant-digit keys over three
    ranges at the large sizes."""
    out = [(n, builder, r) for n in CROSS_PRODUCT_SIZES for builder in BUILDERS for r in RANGES]
    out += [(16385 + 255, "uniform", r) for r in RANGES]
    out += [(n, builder, r) for n in large_sizes(cus) for builder in LARGE_BUILDERS for r in LARGE_RANGES]
    return out


def sort_grid(n, cus):
    """RangeSortGrid (vrdx_layout.h)"""
    return max(1, min(cus, n // CHUNK_MIN))


def chunk_keys(n, grid):
    """RangeChunkKeys (vrdx_layout.h): the ONE formula of the host and the kernels"""
    g = sort_grid(n, grid)
    return -(-(-(-n // g)) // 256) * 256


def make_keys(builder, n, begin, end, rng):
    """n keys whose field [begin, end) follows `builder` and whose other bits are independent random bits"""
    width = end - begin
    digits = digits_of(begin, end)
    top = 1 << width
    outside = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    f = rng.integers(0, top, size=n, dtype=np.uint64)
    if builder == "uniform":
        pass
    elif builder == "few":            # many ties: three distinct fields (two in a range of one bit)
        distinct = rng.choice(top, size=min(3, top), replace=False).astype(np.uint64)
        f = distinct[rng.integers(0, len(distinct), size=n)]
    elif builder == "const-mid":      # digit 1 the same in every key (three digits: two active passes, no copy back)
        p = min(1, digits - 1)
        f = (f & ~np.uint64(0xFF << (8 * p))) | np.uint64((0x5A << (8 * p)) & (top - 1))
    elif builder == "const-low":      # digit 0 the same in every key (two digits: one active pass, a copy back)
        f = (f & ~np.uint64(0xFF)) | np.uint64(0x5A & (top - 1))
    elif builder == "equal":          # no active pass: nothing may move, nothing may be written
        f = np.full(n, 0x2D5A96C3 & (top - 1), dtype=np.uint64)
    elif builder == "ones-mixed":     # fields of all ones among the others, and real 0xFFFFFFFF keys at the array's end: ties
        f[rng.integers(0, 4, size=n) == 0] = top - 1   # with the pads of the last tile
        f[n - 37:] = top - 1
        outside[n - 37:] = 0xFFFFFFFF
    else:
        raise ValueError(builder)
    mask = np.uint64(((top - 1) << begin) & 0xFFFFFFFF)
    return ((outside & ~mask & np.uint64(0xFFFFFFFF)) | (f << np.uint64(begin))).astype(np.uint32)


def case_inputs(builder, n, begin, end):
    """keys and values of one case: the same arrays wherever the case is run, with or without a GPU"""
    rng = np.random.default_rng(zlib.crc32(f"range_sort/{builder}/{n}/{begin}/{end}".encode()))
    return make_keys(builder, n, begin, end, rng), payload(n)


# ---- the model -----------------------------------------------------------------------------------------------------------

SCRATCH_KEY = 0xA5A5A5A5   # what the model's scratch arrays hold before the sort (the GPU tests' poison)


def sort_range_model(keys, values, begin, end, cus, count=None, bound=None, fault=None, tile=TILE, stale_totals=None,
                     stale_mask=None, stale_counts=None):
    """(keys, values, info) as the call leaves the caller's arrays; info: "form", and for the chunked form "active" (the mask),
    "chunks", "chunk_keys", "copy_back" and "scratch_written", and what the call leaves in the storage: "totals" ([4][256])
    and "counts" (the table of per-chunk counts as the last active pass's scan left it, one row per chunk).  bound:
    maxElementCount (default: all of keys); count: what the device reads (default: the bound).  tile: kSegLargeTile as built; a
    tile that is no multiple of 256 has pads in every tile of a chunk, not only in its last one (fault 6).

    What the storage held before, each for a device that has lost the clear or the store that makes it harmless (the device as
    it stands zeroes the totals with the header, stores the mask in its first scan launch and STORES each row of counts):
      stale_totals  [4][256] (or one word for every bin): the fill does not reach the totals, the count launch adds to them;
      stale_mask    header word 2 as another sort left it, and the first scan launch does not store its own: that launch still
                    decides from the totals whether it has anything to scan, every other launch reads the stale word;
      stale_counts  rows of the table of per-chunk counts: the count launch adds to its row instead of storing it."""
    assert fault is None or fault in FAULTS, fault
    keys = np.asarray(keys, np.uint32)
    bound = len(keys) if bound is None else bound
    n = bound if count is None else min(count, bound)
    width = end - begin
    if not 0 <= begin <= end <= 32 or width == 0 or bound == 0:
        return keys.copy(), None if values is None else np.asarray(values, np.uint32).copy(), {"form": "none"}
    if width == 32:
        order = np.argsort(keys[:n], kind="stable")
        out = np.concatenate([keys[:n][order], keys[n:]])
        vals = None if values is None else np.concatenate([np.asarray(values, np.uint32)[:n][order], values[n:]]).astype(np.uint32)
        return out, vals, {"form": "whole-key"}
    if bound <= ONE_WORKGROUP_MAX:
        k, v = sort_bits_cases.sort_bits_model(keys, values, begin, end, n)
        return k, v, {"form": "one-workgroup"}

    digits = digits_of(begin, end)
    grid = sort_grid(bound, cus)
    per_chunk = chunk_keys(n, grid)
    scan_chunk = chunk_keys(bound, grid) if fault == "scan-by-bound" else per_chunk
    chunks = -(-n // per_chunk) if n else 0
    src_k = keys[:n].copy()
    src_v = None if values is None else np.asarray(values[:n], np.uint32).copy()
    dst_k = np.full(n, SCRATCH_KEY, np.uint32)
    dst_v = None if values is None else np.full(n, SCRATCH_KEY, np.uint32)
    in_caller, scratch_written = True, False

    def digit_of(k, p):
        bits = min(8, width - 8 * p)
        if fault == "last-digit-wide" and p == digits - 1:
            bits += 1
        return ((k.astype(np.uint64) >> np.uint64(begin + 8 * p)) & np.uint64((1 << bits) - 1)).astype(np.int64), bits

    # the first count launch: the totals of every digit, from the input; the first scan launch: the active passes
    bins = 512
    totals = [np.bincount(digit_of(keys[:n], p)[0], minlength=bins) for p in range(digits)]
    if stale_totals is not None:
        before = np.broadcast_to(np.asarray(stale_totals, np.int64), (4, 256))
        for p in range(digits):
            totals[p][:256] += before[p]
    derived = [bool(((t != 0) & (t != n)).any()) for t in totals]   # what the first scan launch finds
    active = derived if stale_mask is None else [bool((stale_mask >> p) & 1) for p in range(digits)]   # ... every other launch
    left_counts = np.zeros((0, 256), np.int64)
    for p in range(digits):
        if not active[p]:
            continue
        counted = keys[:n] if fault == "stale-counts" and p > 0 else src_k
        counts = np.zeros((max(chunks, 1), bins), np.int64)
        for c in range(chunks):
            counts[c] = np.bincount(digit_of(counted[c * per_chunk:(c + 1) * per_chunk], p)[0], minlength=bins)
            if stale_counts is not None and c < len(stale_counts):
                counts[c][:256] += np.asarray(stale_counts[c], np.int64)
        start = np.concatenate([[0], np.cumsum(totals[p])[:-1]])
        table = counts.copy()
        scanned = -(-n // scan_chunk)   # rows the scan launch turns into positions
        if p == 0 and not derived[0]:
            scanned = 0                 # (under a stale mask: the first scan launch returns, the scatter meets raw counts)
        run = start.copy()
        for c in range(min(scanned, chunks)):
            table[c] = start if fault == "bases-ignore-chunks" else run
            run = run + counts[c]
        for c in range(chunks):
            base = table[c].copy()
            lo, hi = c * per_chunk, min(n, (c + 1) * per_chunk)
            for t0 in range(lo, hi, tile):
                k = src_k[t0:min(hi, t0 + tile)]
                m = len(k)
                d, bits = digit_of(k, p)
                pads = -m % 256
                order = np.argsort(d, kind="stable")   # (the pads rank behind every real key: last in memory, the largest digit)
                sorted_d = d[order]
                tile_count = np.bincount(d, minlength=bins)
                tile_start = np.concatenate([[0], np.cumsum(tile_count)[:-1]])
                to = base[sorted_d] + np.arange(m) - tile_start[sorted_d]
                ok = (to >= 0) & (to < n)
                dst_k[to[ok]] = k[order][ok]
                if src_v is not None:
                    dst_v[to[ok]] = src_v[t0:t0 + m][order][ok]
                # the pads were counted with the digit of all ones and are taken out of that bin again
                with_pads = tile_count.copy()
                with_pads[(1 << bits) - 1] += pads
                with_pads[255 if fault == "pad-digit-255" else (1 << bits) - 1] -= pads
                if fault != "base-not-advanced":
                    base = base + with_pads
        scratch_written = scratch_written or in_caller
        left_counts = table[:chunks, :256]
        src_k, dst_k, src_v, dst_v, in_caller = dst_k, src_k, dst_v, src_v, not in_caller
    copy_back = digits % 2 == 1 if fault == "copy-back-by-digits" else not in_caller
    if stale_mask is not None:
        copy_back = bin(stale_mask & 0xF).count("1") % 2 == 1
    caller_k, caller_v = (src_k, src_v) if in_caller else (dst_k, dst_v)
    scratch_k, scratch_v = (dst_k, dst_v) if in_caller else (src_k, src_v)
    if copy_back:
        caller_k, caller_v = scratch_k, scratch_v
    out_keys = np.concatenate([caller_k, keys[n:]]).astype(np.uint32)
    out_values = None if values is None else np.concatenate([caller_v, np.asarray(values[n:], np.uint32)]).astype(np.uint32)
    info = {"form": "chunked", "active": sum(1 << p for p in range(digits) if active[p]), "chunks": chunks,
            "chunk_keys": per_chunk, "copy_back": copy_back, "scratch_written": scratch_written,
            "totals": np.array([totals[p][:256] if p < digits else np.zeros(256, np.int64) for p in range(4)]),
            "counts": left_counts}
    return out_keys, out_values, info
