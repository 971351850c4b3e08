"""What the tests of the key orders of the 64-bit sorts share (vrdxHipCmdSort64Ordered[KeyValue][Indirect],
vrdxHipCmdSortSegmented64Ordered[KeyValue]): the order word, the bijection T and its inverse in numpy, the references, the
key builders, and a plain-numpy model of both device forms with plantable faults (tests/test_key_order_cases.py checks
references and model without a GPU; tests/test_sort64_ordered_gpu.py and tests/test_segmented64_ordered_gpu.py run the device
against the references on the same keys).

T(k) = k ^ flip ^ (float64 and bit 63 of k set ? 0x7FFFFFFFFFFFFFFF : 0), flip = 0 for uint64, 1 << 63 for int64 and float64,
complemented for descending.  The sorts leave the elements in ascending unsigned order of T(key), equal keys in input order:
the reference is np.argsort(T(keys), kind="stable") applied to keys and values, and np.lexsort((T(keys), segment id)) for
the segmented calls.

The model restates the device (vrdx_kernels.hip).  The composition keeps the WORDS of T(key) in its word arrays: split, two
stable sorts by a word, merge (keys-only); split with an index, sort, gather of T's high word from the key's high word
alone, sort, permutation that gathers the low word raw and un-transforms only the sorted high word (key+value).  The
segmented kernels turn the real elements into T(key) behind the load and back in front of the store; pads stay all ones; a
byte that is the same in every T(key) of the segment costs no pass; the large form counts the bytes of T(key) once and
walks the segment tile by tile.  `fault` plants ONE mistake the kernels could make."""
import zlib

import numpy as np

from segmented_cases import expected as expected_unsigned_segments
from segmented_cases import mixed_offsets, payload  # noqa: F401

KEY_UINT64, KEY_INT64, KEY_FLOAT64, ORDER_DESCENDING = 0, 1, 2, 0x100   # include/vk_radix_sort.h
ORDERS = ("uint64", "int64", "float64")
DIRECTIONS = (False, True)
SIGN = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
MAGNITUDE = np.uint64(0x7FFFFFFFFFFFFFFF)

SMALL_MAX, MID_MAX, MID_MAX_KEY_VALUE, TILE = 4096, 16384, 8192, 8192   # kSeg64* (vrdx_kernels.h)

FAULTS = ("low-word-flipped-without-the-sign",   # the low word's mask leaves out the float's sign (split and merge alike)
          "merge-sign-from-untransformed-high",  # the merge reads the sign off T's high word as if it were the key's
          "descending-by-reversal",              # ascending sort, output reversed: equal keys come out in reverse input order
          "varying-mask-from-raw-keys",          # the segmented kernels look at the raw keys for what varies (see _segment_lsd)
          "pad-not-largest",                     # the pads go through T with the real elements
          "permute-without-inverse")             # the permutation stores T's high word as the key's


def order_word(order, descending=False):
    return {"uint64": KEY_UINT64, "int64": KEY_INT64, "float64": KEY_FLOAT64}[order] | (ORDER_DESCENDING if descending else 0)


def _flip(order, descending):
    flip = np.uint64(0) if order == "uint64" else SIGN
    return flip ^ ONES if descending else flip


def T(keys, order, descending=False):
    k = np.asarray(keys, np.uint64)
    t = k ^ _flip(order, descending)
    if order == "float64":
        t = t ^ np.where((k & SIGN) != 0, MAGNITUDE, np.uint64(0))
    return t


def T_inverse(t, order, descending=False):
    t = np.asarray(t, np.uint64)
    k = t ^ _flip(order, descending)   # bit 63 is the key's: the float mask never touches it
    if order == "float64":
        k = k ^ np.where((k & SIGN) != 0, MAGNITUDE, np.uint64(0))
    return k


def all_ones_key(order, descending=False):
    """the one key that T maps to all ones, the pad of every segmented kernel: ~0, 0, INT64_MAX, INT64_MIN and the two
    all-ones NaNs"""
    return T_inverse(np.array([ONES]), order, descending)[0]


def expected(keys, values, order, descending=False, count=None):
    """The first `count` (all) elements in ascending order of T(key), equal keys in input order; the rest as they were."""
    n = len(keys) if count is None else count
    perm = np.argsort(T(keys[:n], order, descending), kind="stable")
    ek, ev = keys.copy(), (None if values is None else values.copy())
    ek[:n] = keys[:n][perm]
    if values is not None:
        ev[:n] = values[:n][perm]
    return ek, ev


def expected_segments(keys, values, offsets, max_count, order, descending=False):
    """np.lexsort((T(keys), segment id)) with the bad-offset behaviour of segmented_cases.expected; T is a bijection, so the
    sorted T(keys) are the sorted keys after T_inverse, and what was left alone comes back as it was."""
    tk, ev = expected_unsigned_segments(T(keys, order, descending), values, offsets, max_count)
    return T_inverse(tk, order, descending), ev


def assert_same(got_keys, got_values, want, what=""):
    assert np.array_equal(got_keys, want[0]), f"{what}: keys"
    if got_values is not None:
        assert np.array_equal(got_values, want[1]), f"{what}: values"


# ---- key builders ----------------------------------------------------------------------------------------------------------

INT_EDGES = np.array([1 << 63, (1 << 64) - 1, 0, (1 << 63) - 1, 1, (1 << 63) + 1, (1 << 64) - 2], np.uint64)  # MIN -1 0 MAX ...
FLOAT_EDGES = np.concatenate([
    np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308, 1.5, -1.5,
              1e300, -1e300, 3.0, -3.0]).view(np.uint64),
    # NaNs of both signs: quiet and signalling, several payloads, the two with all payload bits set
    np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FF8000000BEEF00,
              0xFFF8000000BEEF00, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], np.uint64)])
BUILDERS = ("uniform", "mixed-int", "float-specials", "float-values", "low-under-negative-high", "high-only", "duplicates",
            "ones-in-T", "plus-minus-x")


def make_keys(builder, n, rng, order="uint64", descending=False):
    u = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    if builder == "uniform":
        return u
    if builder == "mixed-int":       # both signs, the edges of int64 among them
        return np.where(rng.integers(0, 4, size=n) == 0, INT_EDGES[rng.integers(0, len(INT_EDGES), size=n)], u)
    if builder == "float-specials":  # a third of the keys from +-0, +-inf, denormals, NaNs of both signs, +-x
        return np.where(rng.integers(0, 3, size=n) == 0, FLOAT_EDGES[rng.integers(0, len(FLOAT_EDGES), size=n)], u)
    if builder == "float-values":    # no NaN and no zero, no duplicates to speak of: where torch.sort and totalOrder agree
        return (rng.standard_normal(n) * 1e3 + np.where(rng.integers(0, 2, size=n) == 0, 1e-3, -1e-3)).view(np.uint64)
    if builder == "low-under-negative-high":   # one high word with the sign bit set: the low word alone decides
        return (u & np.uint64(0xFFFFFFFF)) | np.uint64(0xC0123456 << 32)
    if builder == "high-only":
        return (u & np.uint64(0xFFFFFFFF00000000)) | np.uint64(0x89ABCDEF)
    if builder == "duplicates":      # seven keys of both signs: every element has many equals, told apart by their values
        few = np.array([0, 1 << 63, 0xBFF8000000000000, 0x3FF8000000000000, (1 << 64) - 1, 0x7FF8000000000000, 5], np.uint64)
        return few[rng.integers(0, len(few), size=n)]
    if builder == "ones-in-T":       # copies of the key that ties with the pads, at the end of the segment too
        keys = np.where(rng.integers(0, 4, size=n) == 0, all_ones_key(order, descending), u)
        keys[-min(n, 3):] = all_ones_key(order, descending)
        return keys
    if builder == "plus-minus-x":    # +x and -x: ONE raw bit differs, and as float64 up to 63 bits of T
        x = np.array([1234.56789]).view(np.uint64)[0]
        return np.where(rng.integers(0, 2, size=n) == 0, x, x | SIGN)
    raise ValueError(builder)


def case_keys(builder, n, order, descending, tag=""):
    """the same keys and values wherever the case is run, with or without a GPU"""
    rng = np.random.default_rng(zlib.crc32(f"key_order/{builder}/{n}/{order}/{descending}/{tag}".encode()))
    return make_keys(builder, n, rng, order, descending), payload(n)


def segment_case(builder, sizes, order, descending, tag=""):
    """keys, values and offsets of one segmented call: segments of `sizes`, shuffled, untouched elements around them; the
    builder is applied per segment, so "ones-in-T" ends every segment with the pad's twin"""
    rng = np.random.default_rng(zlib.crc32(f"key_order/segments/{builder}/{sizes}/{order}/{descending}/{tag}".encode()))
    offsets, n = mixed_offsets(rng, sizes)
    keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    for b, e in zip(offsets[:-1], offsets[1:]):
        if e > b:
            keys[b:e] = make_keys(builder, int(e - b), rng, order, descending)
    return keys, payload(n), offsets


# ---- the model ---------------------------------------------------------------------------------------------------------------

def _masks(order, descending):
    flip = int(_flip(order, descending))
    return np.uint32(flip >> 32), np.uint32(flip & 0xFFFFFFFF), np.uint32(0xFFFFFFFF if order == "float64" else 0)


def _neg_of_key(hi, float_mask):
    return np.where((hi >> np.uint32(31)) != 0, float_mask, np.uint32(0)).astype(np.uint32)


def _neg_of_t(t_hi, flip_hi, float_mask, fault=None):
    h = t_hi if fault == "merge-sign-from-untransformed-high" else t_hi ^ flip_hi
    return _neg_of_key(h, float_mask)


def _stable(words):
    return np.argsort(words, kind="stable")


def sort64_ordered_model(keys, values, order, descending=False, fault=None):
    """(keys, values) as vrdxHipCmdSort64Ordered[KeyValue] leaves them"""
    assert fault is None or fault in FAULTS, fault
    keys = np.asarray(keys, np.uint64)
    if fault == "descending-by-reversal" and descending:
        k, v = sort64_ordered_model(keys, values, order, False)
        return k[::-1].copy(), (None if v is None else v[::-1].copy())
    flip_hi, flip_lo, float_mask = _masks(order, descending)
    lo, hi = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), (keys >> np.uint64(32)).astype(np.uint32)
    neg = _neg_of_key(hi, float_mask)
    low_neg = np.uint32(0) if fault == "low-word-flipped-without-the-sign" else neg
    t_lo, t_hi = lo ^ flip_lo ^ low_neg, hi ^ flip_hi ^ (neg & np.uint32(0x7FFFFFFF))
    if values is None:
        # split (A = T's low words, B = its high words) | sort (A, B) | sort (B, A) | merge
        p = _stable(t_lo)
        a, b = t_lo[p], t_hi[p]
        p = _stable(b)
        a, b = a[p], b[p]
        neg = _neg_of_t(b, flip_hi, float_mask, fault)
        low_neg = np.uint32(0) if fault == "low-word-flipped-without-the-sign" else neg
        out_lo, out_hi = a ^ flip_lo ^ low_neg, b ^ flip_hi ^ (neg & np.uint32(0x7FFFFFFF))
        return (out_hi.astype(np.uint64) << np.uint64(32)) | out_lo.astype(np.uint64), None
    # split (A = T's low words, I = iota) | sort (A, I) | gather (A = T's high word of keys[I], from the key's high word
    # alone) | sort (A, I) | permute (high word un-transformed, low word raw from keys[I])
    index = _stable(t_lo)
    a = t_hi[index]
    p = _stable(a)
    a, index = a[p], index[p]
    if fault == "permute-without-inverse":
        out_hi = a
    else:
        out_hi = a ^ flip_hi ^ (_neg_of_t(a, flip_hi, float_mask, fault) & np.uint32(0x7FFFFFFF))
    return (out_hi.astype(np.uint64) << np.uint64(32)) | lo[index].astype(np.uint64), np.asarray(values)[index]


def _byte(t, p):
    return ((t >> np.uint64(8 * p)) & np.uint64(0xFF)).astype(np.int64)


def _in_lds(k, v, order, descending, fault):
    """SortInWorkgroup64, ORDERED: T behind the load, pads all ones, a pass per byte that varies over the real elements'
    T(key), the first n slots stored through the inverse.  (Taking the mask over the RAW keys here is harmless, and the model
    shows it: keys of one sign differ in the same bytes before and after T, and keys of two signs are told apart by T's top
    byte, which the raw mask covers with bit 63.)"""
    n = len(k)
    pads = (-n) % 256
    t = T(k, order, descending)
    pad = T(np.array([ONES]), order, descending)[0] if fault == "pad-not-largest" else ONES
    t = np.concatenate([t, np.full(pads, pad, np.uint64)])
    vals = None if v is None else np.concatenate([v, np.zeros(pads, np.uint32)])
    seen = k if fault == "varying-mask-from-raw-keys" else t[:n]
    varying = int(np.bitwise_or.reduce(seen ^ seen[0]))
    for p in range(8):
        if (varying >> (8 * p)) & 0xFF == 0:
            continue
        perm = _stable(_byte(t, p))
        t = t[perm]
        if vals is not None:
            vals = vals[perm]
    return T_inverse(t[:n], order, descending), (None if v is None else vals[:n])


def _segment_lsd(k, v, order, descending, fault):
    """SegmentLsd64, ORDERED: one read counts the eight bytes of T(key); a byte with one value is no pass; every other pass
    walks the segment in tiles from one array to the other, bases from the counts -- the first pass that runs applies T
    behind its loads, the last one the inverse in front of its stores, memory holds T(key) between them; an odd number of
    passes ends with a copy back.  The mask of varying bytes IS the histograms here, so the fault
    "varying-mask-from-raw-keys" takes the counts, and with them the bases, from the raw keys."""
    n = len(k)
    counted = k if fault == "varying-mask-from-raw-keys" else T(k, order, descending)
    hists = [np.bincount(_byte(counted, p), minlength=256) for p in range(8)]
    active = [p for p, h in enumerate(hists) if ((h != 0) & (h != n)).any()]
    ks = [k.copy(), np.zeros(n, np.uint64)]
    vs = [None if v is None else v.copy(), None if v is None else np.zeros(n, np.uint32)]
    src = 0
    for p in active:
        base = np.cumsum(hists[p]) - hists[p]
        for t0 in range(0, n, TILE):
            tile = ks[src][t0:t0 + TILE]
            if p == active[0]:
                tile = T(tile, order, descending)
            d = _byte(tile, p)
            perm = _stable(d)
            ds = d[perm]
            counts = np.bincount(ds, minlength=256)
            start = np.cumsum(counts) - counts
            to = base[ds] + np.arange(len(tile)) - start[ds]
            ok = to < n
            out = tile[perm][ok]
            ks[1 - src][to[ok]] = T_inverse(out, order, descending) if p == active[-1] else out
            if vs[src] is not None:
                vs[1 - src][to[ok]] = vs[src][t0:t0 + TILE][perm][ok]
            base = base + counts
        src = 1 - src
    return ks[src], vs[src]


def segmented64_ordered_model(keys, values, offsets, order, descending=False, fault=None):
    """(keys, values) as vrdxHipCmdSortSegmented64Ordered[KeyValue] leaves the caller's arrays, maxElementCount = len(keys)"""
    assert fault is None or fault in FAULTS, fault
    keys = np.asarray(keys, np.uint64)
    out_k = keys.copy()
    out_v = None if values is None else np.asarray(values, np.uint32).copy()
    mid_max = MID_MAX if values is None else MID_MAX_KEY_VALUE
    o = [int(x) for x in offsets]
    for b, e in zip(o[:-1], o[1:]):
        if not (b <= e <= len(keys)) or e - b < 2:
            continue
        form = _in_lds if e - b <= mid_max else _segment_lsd
        k, v = keys[b:e], (None if values is None else np.asarray(values, np.uint32)[b:e])
        if fault == "descending-by-reversal" and descending:
            k, v = form(k, v, order, False, None)
            k, v = k[::-1], (None if v is None else v[::-1])
        else:
            k, v = form(k, v, order, descending, fault)
        out_k[b:e] = k
        if out_v is not None:
            out_v[b:e] = v
    return out_k, out_v
