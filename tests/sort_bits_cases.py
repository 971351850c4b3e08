"""What the tests of the bit-range sorts (vrdxHipCmdSortBits[KeyValue][Indirect]) share: the reference, key builders whose bits
outside the range are random, and a plain-numpy model of the device algorithm with plantable faults
(tests/test_sort_bits_cases.py checks the model without a GPU; tests/test_sort_bits_gpu.py runs the device against the
reference on the same cases).

The order is by the field f(k) = (k >> begin) & (2^(end - begin) - 1), stable, keys moved whole.  Every builder fills the bits
outside the range with independent random bits: a whole-key sort then differs from the range sort, and the stability of a
keys-only sort is visible in the keys themselves.

The model restates what the one-workgroup kernel does (vrdx_kernels.hip, SortInWorkgroup with RANGE): P = ceil(width / 8)
stable ranking passes, pass p by the min(8, width - 8 p) bits of the key from bit begin + 8 p, keys and values moved
together and whole.  `fault` plants ONE mistake the kernel could make.  Range sorts of more than 16384 elements are not
built: the library refuses them (REFUSED_SIZES).
"""
import zlib

import numpy as np

FAULTS = ("last-digit-wide",    # the last digit one bit too wide
          "begin-dropped",      # passes after the first extract from bit 8 p, not begin + 8 p
          "whole-key",          # a whole-key sort in place of the field sort
          "masked-keys",        # the field is stored where the whole key belongs
          "width-mod-8",        # the last digit's width taken modulo 8: nothing where the width is a multiple of 8
          "values-stale")       # the last pass moves the keys and leaves the values in their order

# (begin, end) and what each exercises
RANGES = [(0, 1),     # one bit, bottom
          (31, 32),   # one bit, top
          (0, 8),     # one aligned byte
          (8, 16),    # one aligned byte, not at bit 0
          (4, 12),    # one digit, unaligned
          (3, 12),    # two digits, the second one bit wide
          (0, 16),    # two aligned bytes
          (5, 21),    # two digits, unaligned
          (7, 24),    # three digits plus the copier
          (1, 32),    # four digits, the last of 7 bits
          (0, 31)]
EMPTY_RANGE = (13, 13)
FULL_RANGE = (0, 32)
BUILDERS = ["uniform", "few", "const-byte", "equal", "ones"]
BUILDER_SIZES = [4097, 16383]   # every builder in the 1024-thread kernel: a ragged last chunk, and nearly full

# Sizes of the GPU tests: both one-workgroup kernels (256 threads up to 4096 elements, 1024 threads beyond), their edges,
# and sizes beyond one workgroup, which the library refuses (tests/test_sort_bits_plan.py holds both lists to the planner)
ONE_WORKGROUP_SIZES = [1, 2, 257, 4096, 4097, 16383, 16384]
REFUSED_SIZES = [16385, 65539]
BALLOT_SIZES = [257, 4097, 16384]
BALLOT_RANGES = [(3, 12), (1, 32)]
INDIRECT_BOUNDS = [4096, 4097, 16384]


def digits_of(begin, end):
    return (end - begin + 7) // 8


def field(keys, begin, end):
    keys = np.asarray(keys, dtype=np.uint32)
    width = end - begin
    if width == 0:
        return np.zeros(len(keys), np.uint32)
    return ((keys.astype(np.uint64) >> np.uint64(begin)) & np.uint64((1 << width) - 1)).astype(np.uint32)


def payload(n):
    """values that are not their own index: iota * 2654435761 mod 2^32"""
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def reference(keys, values, begin, end, count=None):
    """np.argsort(f(keys[:count]), kind="stable") applied to keys and values; the tail untouched"""
    n = len(keys) if count is None else min(count, len(keys))
    f = field(keys[:n], begin, end)
    order = np.argsort(f.astype(np.uint16) if end - begin <= 16 else f, kind="stable")   # (the same order, a faster sort)
    out_keys = np.concatenate([np.asarray(keys[:n], np.uint32)[order], keys[n:]]).astype(np.uint32)
    out_values = None if values is None else np.concatenate([np.asarray(values[:n], np.uint32)[order], values[n:]]).astype(np.uint32)
    return out_keys, out_values


def make_keys(builder, n, begin, end, rng):
    """n keys whose field [begin, end) follows `builder` and whose other bits are independent random bits"""
    width = end - begin
    outside = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    top = 1 << width
    if builder == "uniform":
        f = rng.integers(0, top, size=n, dtype=np.uint64)
    elif builder == "few":          # many ties: three distinct fields (two in a range of one bit)
        distinct = rng.choice(top, size=min(3, top), replace=False).astype(np.uint64)
        f = distinct[rng.integers(0, len(distinct), size=n)]
    elif builder == "const-byte":   # byte 0 of the field the same in every key: a pass that must move nothing
        f = (rng.integers(0, top, size=n, dtype=np.uint64) & ~np.uint64(0xFF)) | np.uint64(0x5A & (top - 1))
    elif builder == "equal":
        f = np.full(n, 0x2D5A96C3 & (top - 1), dtype=np.uint64)
    elif builder == "ones":         # ties with the pads behind the last element
        f = np.full(n, top - 1, dtype=np.uint64)
    else:
        raise ValueError(builder)
    mask = np.uint64(((top - 1) << begin) & 0xFFFFFFFF)
    return ((outside & ~mask & np.uint64(0xFFFFFFFF)) | (f << np.uint64(begin))).astype(np.uint32)


def case_inputs(builder, n, begin, end):
    """keys and values of one case: the same arrays wherever the case is run, with or without a GPU"""
    rng = np.random.default_rng(zlib.crc32(f"sort_bits/{builder}/{n}/{begin}/{end}".encode()))
    return make_keys(builder, n, begin, end, rng), payload(n)


def non_degenerate(builder, n, begin, end):
    """Cases on which a whole-key sort must differ from the range sort: random bits ABOVE the range (they lead the whole-key
    order), or random bits below it and fields that tie (they order the ties).  What is left out: the empty and the full
    range, a handful of keys, and ranges that end at bit 32 over fields that are as good as distinct -- there the field
    order IS the whole-key order."""
    if n < 64 or not 0 < end - begin < 32:
        return False
    return end < 32 or (end - begin <= 8 or builder in ("few", "equal", "ones"))


# ---- the model -----------------------------------------------------------------------------------------------------------

def sort_bits_model(keys, values, begin, end, count=None, fault=None):
    """(keys, values) as the one launch leaves the caller's arrays"""
    assert fault is None or fault in FAULTS, fault
    n = len(keys) if count is None else min(count, len(keys))
    width = end - begin
    keys = np.asarray(keys, np.uint32)
    if width == 0 or n == 0:
        return keys.copy(), None if values is None else np.asarray(values, np.uint32).copy()
    digits = digits_of(begin, end)
    k = keys[:n].copy()
    v = None if values is None else np.asarray(values[:n], np.uint32).copy()
    passes = [(begin + 8 * p, min(8, width - 8 * p)) for p in range(digits)]
    if fault == "whole-key":
        passes = [(8 * p, 8) for p in range(4)]
    for p, (shift, bits) in enumerate(passes):
        if fault == "begin-dropped" and p > 0:
            shift = 8 * p
        if p == digits - 1 and fault == "last-digit-wide":
            bits += 1
        if p == digits - 1 and fault == "width-mod-8":
            bits = (width - 8 * p) % 8
        digit = (k.astype(np.uint64) >> np.uint64(shift)) & np.uint64((1 << bits) - 1)
        order = np.argsort(digit, kind="stable")
        k = k[order]
        if v is not None and not (fault == "values-stale" and p == len(passes) - 1):
            v = v[order]
    if fault == "masked-keys":
        k = field(k, begin, end)
    out_keys = np.concatenate([k, keys[n:]]).astype(np.uint32)
    out_values = None if values is None else np.concatenate([v, np.asarray(values[n:], np.uint32)]).astype(np.uint32)
    return out_keys, out_values
