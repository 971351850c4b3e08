"""What the tests of the segmented sort by a bit range (vrdxHipCmdSortSegmentedBits[KeyValue]) share: the reference, the key
builders, one guarded call, and a plain-numpy model of the three device forms with plantable faults
(tests/test_segmented_bits_cases.py checks the model without a GPU; tests/test_segmented_bits_gpu.py runs the device against
the reference on the same cases).

The order inside every segment is by the field f(k) = (k >> begin) & (2^(end - begin) - 1), stable, keys moved whole.  The
reference is np.lexsort((f(keys), segment id)) over the whole call: what segmented_cases.expected does for whole keys, with
its bad-offset behaviour (a segment with o[i] > o[i+1] or o[i+1] > max_count is left alone).

The model restates the device (vrdx_kernels.hip): segments of up to 16384 elements take P = ceil(width / 8) stable ranking
passes in LDS (SortInWorkgroup with RANGE); a larger one (SegmentLsd with RANGE) reads the segment once for the histograms of
the field's P digits, skips a digit that is the same in every key, walks the segment tile by tile once per remaining digit
from one array to the other -- the caller's range and the same index range of the scratch -- and copies the result back
after an odd number of such walks.  `fault` plants ONE mistake the kernels could make."""
import zlib

import numpy as np

import sort_bits_cases as bits
from segmented_cases import mixed_offsets, run_segmented
from sort_bits_cases import EMPTY_RANGE, FULL_RANGE, RANGES, digits_of, field, non_degenerate, payload  # noqa: F401

SMALL_MAX, MID_MAX, TILE = 4096, 16384, 16384   # kSegSmallMax, kSegMidMax, kSegLargeTile (vrdx_kernels.h)

# "const-middle": digit 1 of the field the same in every key while digits 0 and 2 vary -- over a range of three digits that
# is two active passes of the large form, so no copy back
BUILDERS = list(bits.BUILDERS) + ["const-middle"]
FAULTS = tuple(bits.FAULTS) + ("no-copy-back",              # an odd number of active passes leaves the caller's range one pass behind
                               "bases-from-key-bytes",      # the large form's histogram taken from the key's bytes
                               "boundary-ignored",          # two adjacent segments sorted as one
                               "copy-back-by-digit-count")  # copy back decided by P, not by the active passes

# every size class in one call: both in-LDS kernels at their edges, the large kernel with one tile plus one key, exactly two
# full tiles, three tiles with a ragged last one
SIZES = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 32768, 36865]
PASS_SIZES = [16385, 49153]   # the large form's pass logic: two tiles (the second of one key), four tiles
# (builder, range): what the large form's pass logic has to get right
PASS_CASES = [("uniform", (4, 12)),        # one active pass: the result is copied back
              ("uniform", (5, 21)),        # two
              ("uniform", (7, 24)),        # three
              ("uniform", (1, 32)),        # four
              ("const-middle", (7, 24)),   # three digits, the middle one constant: two active passes, no copy back
              ("const-byte", (7, 24)),     # three digits, the lowest one constant
              ("const-byte", (5, 21)),     # two digits, one active pass
              ("few", (3, 12)),            # two digits, the second one bit wide
              ("equal", (7, 24)),          # the same field in every key: nothing moves
              ("ones", (7, 24))]           # every field ties with the pads


def make_keys(builder, n, begin, end, rng):
    if builder != "const-middle":
        return bits.make_keys(builder, n, begin, end, rng)
    keys = bits.make_keys("uniform", n, begin, end, rng)
    width = end - begin
    if width <= 8:
        return keys   # (the range has no digit 1)
    middle = ((1 << min(8, width - 8)) - 1) << (begin + 8)
    return ((keys & np.uint32(~middle & 0xFFFFFFFF)) | np.uint32(middle & (0xC3 << (begin + 8)))).astype(np.uint32)


def case_inputs(builder, begin, end, sizes=SIZES, tag=""):
    """keys, values and offsets of one case: the same arrays wherever the case is run, with or without a GPU.  Untouched
    elements in front of o[0] and behind the last segment."""
    rng = np.random.default_rng(zlib.crc32(f"segmented_bits/{builder}/{begin}/{end}/{tag}".encode()))
    offsets, n = mixed_offsets(rng, sizes)
    return make_keys(builder, n, begin, end, rng), payload(n), offsets


def expected(keys, values, offsets, max_count, begin, end):
    """Every valid segment (o[i] <= o[i+1] <= max_count) stably sorted by the field on its own, everything else as it was."""
    ek, ev = keys.copy(), (values.copy() if values is not None else None)
    f = field(keys, begin, end)
    o = np.asarray(offsets, dtype=np.int64)
    lengths = np.diff(o)
    if len(o) > 1 and (lengths >= 0).all() and o[-1] <= max_count:
        lo, hi = int(o[0]), int(o[-1])
        seg = np.repeat(np.arange(len(lengths)), lengths)
        order = np.lexsort((f[lo:hi], seg))
        ek[lo:hi] = keys[lo:hi][order]
        if values is not None:
            ev[lo:hi] = values[lo:hi][order]
        return ek, ev
    for b, e in zip(o[:-1], o[1:]):
        if b <= e <= max_count:
            order = np.argsort(f[b:e], kind="stable")
            ek[b:e] = keys[b:e][order]
            if values is not None:
                ev[b:e] = values[b:e][order]
    return ek, ev


def run_segmented_bits(torch, sorter, keys, offsets, begin, end, values=None, **kw):
    """segmented_cases.run_segmented by the bits [begin, end); expect_status=None: the failure word is not read"""
    return run_segmented(torch, sorter, keys, offsets, values, bit_range=(begin, end), **kw)


def check(got_k, got_v, keys, values, offsets, begin, end, want=None):
    ek, ev = want if want is not None else expected(keys, values, offsets, len(keys), begin, end)
    assert np.array_equal(got_k, ek)
    if values is not None:
        assert np.array_equal(got_v, ev)


# ---- the model -----------------------------------------------------------------------------------------------------------

def _passes(begin, end, fault):
    """(first bit, width) of every digit the kernels rank by, in pass order"""
    width = end - begin
    digits = digits_of(begin, end)
    if fault == "whole-key":
        return [(8 * p, 8) for p in range(4)]
    passes = []
    for p in range(digits):
        shift, w = begin + 8 * p, min(8, width - 8 * p)
        if fault == "begin-dropped" and p > 0:
            shift = 8 * p
        if p == digits - 1 and fault == "last-digit-wide":
            w += 1
        if p == digits - 1 and fault == "width-mod-8":
            w = (width - 8 * p) % 8
        passes.append((shift, w))
    return passes


def _digit(k, shift, w):
    return ((k.astype(np.uint64) >> np.uint64(shift)) & np.uint64((1 << w) - 1)).astype(np.int64)


def _in_lds(k, v, begin, end, fault):
    """SortInWorkgroup with RANGE: every digit of the range is ranked, the elements stay in registers"""
    passes = _passes(begin, end, fault)
    for p, (shift, w) in enumerate(passes):
        order = np.argsort(_digit(k, shift, w), kind="stable")
        k = k[order]
        if v is not None and not (fault == "values-stale" and p == len(passes) - 1):
            v = v[order]
    return k, v


def _segment_lsd(k, v, begin, end, fault):
    """SegmentLsd with RANGE on one segment: returns what the caller's range holds afterwards"""
    n = len(k)
    passes = _passes(begin, end, fault)
    # 1. one histogram per digit; a digit with one value only is not a pass
    counted = [(8 * p, 8) for p in range(len(passes))] if fault == "bases-from-key-bytes" else passes
    bins = max(256, max(1 << w for _, w in passes))   # (256 counters per digit; a planted digit of nine bits overruns them)
    hists = [np.bincount(_digit(k, shift, w), minlength=bins) for shift, w in counted]
    active = [p for p, h in enumerate(hists) if ((h != 0) & (h != n)).any()]
    # 2. the walks, between the caller's range (index 0) and the scratch range (index 1)
    ks = [k.copy(), np.zeros(n, np.uint32)]
    vs = [None if v is None else v.copy(), None if v is None else np.zeros(n, np.uint32)]
    src = 0
    for p in active:
        shift, w = passes[p]
        base = np.cumsum(hists[p]) - hists[p]
        stale = fault == "values-stale" and p == active[-1]
        if stale and vs[src] is not None:
            vs[1 - src][:] = vs[src]
        for t0 in range(0, n, TILE):
            tile = ks[src][t0:t0 + TILE]
            d = _digit(tile, shift, w)
            order = np.argsort(d, kind="stable")
            ds = d[order]
            counts = np.bincount(ds, minlength=bins)
            start = np.cumsum(counts) - counts
            to = base[ds] + np.arange(len(tile)) - start[ds]
            ok = to < n
            ks[1 - src][to[ok]] = tile[order][ok]
            if vs[src] is not None and not stale:
                vs[1 - src][to[ok]] = vs[src][t0:t0 + TILE][order][ok]
            base = base + counts
        src = 1 - src
    # 3. the copy back
    if fault == "no-copy-back":
        back = False
    elif fault == "copy-back-by-digit-count":
        back = len(passes) % 2 == 1
    else:
        back = src == 1
    if back:
        ks[0][:] = ks[1]
        if vs[0] is not None:
            vs[0][:] = vs[1]
    return ks[0], vs[0]


def segmented_bits_model(keys, values, offsets, begin, end, fault=None):
    """(keys, values) as the call leaves the caller's arrays, maxElementCount = len(keys)"""
    assert fault is None or fault in FAULTS, fault
    keys = np.asarray(keys, np.uint32)
    out_k = keys.copy()
    out_v = None if values is None else np.asarray(values, np.uint32).copy()
    if end == begin:
        return out_k, out_v
    o = [int(x) for x in offsets]
    segments = [(b, e) for b, e in zip(o[:-1], o[1:]) if b <= e <= len(keys)]
    if fault == "boundary-ignored":
        for i in range(len(segments) - 1):
            (b, m), (m2, e) = segments[i], segments[i + 1]
            if m == m2 and b < m < e:
                segments[i:i + 2] = [(b, e)]
                break
    for b, e in segments:
        n = e - b
        if n < 2:
            continue
        form = _in_lds if n <= MID_MAX else _segment_lsd
        k, v = form(out_k[b:e].copy(), None if out_v is None else out_v[b:e].copy(), begin, end, fault)
        if fault == "masked-keys":
            k = field(k, begin, end)
        out_k[b:e] = k
        if out_v is not None:
            out_v[b:e] = v
    return out_k, out_v
