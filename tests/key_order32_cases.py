"""What the tests of the key orders of the 32-bit sorts share (vrdxHipCmdOrderedSort[KeyValue][Indirect],
vrdxHipCmdOrderedSortSegmented[KeyValue]): the order word, the bijection T and its inverse in numpy, the references, the key
builders, and a plain-numpy model of the three device forms with plantable faults (tests/test_key_order32_cases.py checks
references and model without a GPU; tests/test_ordered_sort_gpu.py and tests/test_ordered_sort_segmented_gpu.py run the device
against the references on the same keys).

T(k) = k ^ flip ^ (float32 and bit 31 of k set ? 0x7FFFFFFF : 0), flip = 0 for uint32, 1 << 31 for int32 and float32,
complemented for descending.  The sorts leave the elements in ascending unsigned order of T(key), equal keys in input order:
the reference is np.argsort(T(keys), kind="stable") applied to keys and values, and np.lexsort((T(keys), segment id)) for
the segmented calls.

The model restates the device (vrdx_kernels.hip):
  in-LDS      SortInWorkgroup, ORDERED: real elements become T(key) behind the load, pads stay all ones, four stable passes by
              a byte, the first n slots stored through the inverse;
  large       SegmentLsd, ORDERED: one read counts the four bytes of T(key); a byte with one value is no pass; the first pass
              that runs applies T behind its loads, the last one the inverse in front of its stores, memory holds T(key)
              between them; an odd number of passes ends with a copy back;
  flat        beyond 16384 elements: T in place on keys[0, n), n = min(device count, bound), a stable sort of those words,
              the inverse in place on keys[0, n).
`fault` plants ONE mistake the kernels could make."""
import zlib

import numpy as np

from segmented_cases import expected as expected_unsigned_segments
from segmented_cases import mixed_offsets, payload  # noqa: F401

KEY32_UINT32, KEY32_INT32, KEY32_FLOAT32, ORDER_DESCENDING = 0, 1, 2, 0x100   # include/vk_radix_sort.h
ORDERS = ("uint32", "int32", "float32")
DIRECTIONS = (False, True)
SIGN = np.uint32(0x80000000)
ONES = np.uint32(0xFFFFFFFF)
MAGNITUDE = np.uint32(0x7FFFFFFF)

SMALL_MAX, MID_MAX, TILE, ONE_WORKGROUP_MAX = 4096, 16384, 16384, 16384   # kSeg*, kSmallSortMaxElements (vrdx_kernels.h)

FAULTS = ("histogram-from-raw-keys",         # the large class counts the bytes of the raw keys: bases and active passes are not T's
          "no-inverse-before-copy-back",     # the last pass stores T(key) when an odd number of passes ends with the copy back
          "float-mask-flips-sign",           # the float mask is all ones: it also flips bit 31
          "neg-from-untransformed-word",     # the way back reads the sign off T(key) as if it were the key
          "descending-by-reversal",          # ascending sort, output reversed: equal keys come out in reverse input order
          "transform-up-to-the-bound",       # the forward transform runs to the bound, not to the device count: T(key) behind it
          "pads-transformed")                # the pads go through T with the real elements


def order_word(order, descending=False):
    return {"uint32": KEY32_UINT32, "int32": KEY32_INT32, "float32": KEY32_FLOAT32}[order] | (ORDER_DESCENDING if descending else 0)


def _flip(order, descending):
    flip = np.uint32(0) if order == "uint32" else SIGN
    return flip ^ ONES if descending else flip


def T(keys, order, descending=False, fault=None):
    k = np.asarray(keys, np.uint32)
    t = k ^ _flip(order, descending)
    if order == "float32":
        t = t ^ np.where((k & SIGN) != 0, ONES if fault == "float-mask-flips-sign" else MAGNITUDE, np.uint32(0))
    return t


def T_inverse(t, order, descending=False, fault=None):
    t = np.asarray(t, np.uint32)
    k = t ^ _flip(order, descending)   # bit 31 is the key's: the float mask never touches it
    if order == "float32":
        sign_of = t if fault == "neg-from-untransformed-word" else k
        k = k ^ np.where((sign_of & SIGN) != 0, ONES if fault == "float-mask-flips-sign" else MAGNITUDE, np.uint32(0))
    return k


def all_ones_key(order, descending=False):
    """the one key that T maps to all ones, the pad of every in-LDS sort: ~0, 0, INT32_MAX, INT32_MIN and the two all-ones NaNs"""
    return T_inverse(np.array([ONES]), order, descending)[0]


def expected(keys, values, order, descending=False, count=None):
    """The first `count` (all) elements in ascending order of T(key), equal keys in input order; the rest as they were."""
    n = len(keys) if count is None else min(count, len(keys))
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

INT_EDGES = np.array([1 << 31, (1 << 32) - 1, 0, (1 << 31) - 1, 1, (1 << 31) + 1, (1 << 32) - 2], np.uint32)  # MIN -1 0 MAX ...
FLOAT_EDGES = np.concatenate([
    np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38, 1.5, -1.5, 1e30, -1e30, 3.0, -3.0],
             np.float32).view(np.uint32),
    # NaNs of both signs: quiet and signalling, several payloads, the two with all payload bits set
    np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FC0BEEF, 0xFFC0BEEF, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32)])
BUILDERS = ("uniform", "mixed-int", "float-specials", "float-values", "duplicates", "all-equal", "one-byte", "three-bytes",
            "ones-in-T", "plus-minus-x")


def make_keys(builder, n, rng, order="uint32", descending=False):
    u = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if builder == "uniform":
        return u
    if builder == "mixed-int":       # both signs, the edges of int32 among them
        return np.where(rng.integers(0, 4, size=n) == 0, INT_EDGES[rng.integers(0, len(INT_EDGES), size=n)], u)
    if builder == "float-specials":  # a third of the keys from +-0, +-inf, denormals, NaNs of both signs, +-x
        return np.where(rng.integers(0, 3, size=n) == 0, FLOAT_EDGES[rng.integers(0, len(FLOAT_EDGES), size=n)], u)
    if builder == "float-values":    # no NaN and no zero: where torch.sort, np.sort and totalOrder agree
        return (rng.standard_normal(n) * 1e3 + np.where(rng.integers(0, 2, size=n) == 0, 1e-3, -1e-3)).astype(np.float32).view(np.uint32)
    if builder == "duplicates":      # seven keys of both signs: every element has many equals, told apart by their values
        few = np.array([0, 1 << 31, 0xBFC00000, 0x3FC00000, (1 << 32) - 1, 0x7FC00000, 5], np.uint32)
        return few[rng.integers(0, len(few), size=n)]
    if builder == "all-equal":       # no byte of T varies: the large class runs no pass and the keys come back raw
        return np.full(n, 0xC0FFEE11, np.uint32)
    if builder == "one-byte":        # keys that differ in byte 1 only, the sign bit set: exactly one pass, so a copy back
        return (u & np.uint32(0x0000FF00)) | np.uint32(0xC1230045)
    if builder == "three-bytes":     # byte 2 and the sign are constant: exactly three active passes in every order, an odd
        return (u & np.uint32(0x7F00FFFF)) | np.uint32(0x805A0000)   # number, so a copy back
    if builder == "ones-in-T":       # copies of the key that ties with the pads, at the end of the segment too
        keys = np.where(rng.integers(0, 4, size=n) == 0, all_ones_key(order, descending), u)
        keys[-min(n, 3):] = all_ones_key(order, descending)
        return keys
    if builder == "plus-minus-x":    # +x and -x: ONE raw bit differs, and as float32 up to 31 bits of T
        x = np.array([1234.56789], np.float32).view(np.uint32)[0]
        return np.where(rng.integers(0, 2, size=n) == 0, x, x | SIGN)
    raise ValueError(builder)


def case_keys(builder, n, order, descending, tag=""):
    """the same keys and values wherever the case is run, with or without a GPU"""
    rng = np.random.default_rng(zlib.crc32(f"key_order32/{builder}/{n}/{order}/{descending}/{tag}".encode()))
    return make_keys(builder, n, rng, order, descending), payload(n)


def segment_case(builder, sizes, order, descending, tag=""):
    """keys, values and offsets of one segmented call: segments of `sizes`, shuffled, untouched elements around them; the
    builder is applied per segment, so "ones-in-T" ends every segment with the pad's twin"""
    rng = np.random.default_rng(zlib.crc32(f"key_order32/segments/{builder}/{sizes}/{order}/{descending}/{tag}".encode()))
    offsets, n = mixed_offsets(rng, sizes)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    for b, e in zip(offsets[:-1], offsets[1:]):
        if e > b:
            keys[b:e] = make_keys(builder, int(e - b), rng, order, descending)
    return keys, payload(n), offsets


# ---- the model ---------------------------------------------------------------------------------------------------------------

def _stable(words):
    return np.argsort(words, kind="stable")


def _byte(t, p):
    return ((t >> np.uint32(8 * p)) & np.uint32(0xFF)).astype(np.int64)


def _in_lds(k, v, order, descending, fault):
    """SortInWorkgroup, ORDERED: T behind the load, pads all ones behind the real elements, four stable passes, the first n
    slots stored through the inverse."""
    n = len(k)
    pads = (-n) % 256
    t = T(k, order, descending, fault)
    pad = T(np.array([ONES]), order, descending, fault)[0] if fault == "pads-transformed" else ONES
    t = np.concatenate([t, np.full(pads, pad, np.uint32)])
    vals = None if v is None else np.concatenate([v, np.zeros(pads, np.uint32)])
    for p in range(4):
        perm = _stable(_byte(t, p))
        t = t[perm]
        if vals is not None:
            vals = vals[perm]
    return T_inverse(t[:n], order, descending, fault), (None if v is None else vals[:n])


def _segment_lsd(k, v, order, descending, fault):
    """SegmentLsd, ORDERED (the module's docstring).  Every tile is padded with all ones to whole chunks of 256 like the
    device's, the pads are digit 255's last keys and are not written."""
    n = len(k)
    counted = k if fault == "histogram-from-raw-keys" else T(k, order, descending, fault)
    hists = [np.bincount(_byte(counted, p), minlength=256) for p in range(4)]
    active = [p for p, h in enumerate(hists) if ((h != 0) & (h != n)).any()]
    ks = [k.copy(), np.zeros(n, np.uint32)]
    vs = [None if v is None else v.copy(), None if v is None else np.zeros(n, np.uint32)]
    src = 0
    for p in active:
        base = np.cumsum(hists[p]) - hists[p]
        for t0 in range(0, n, TILE):
            tile = ks[src][t0:t0 + TILE]
            m = len(tile)
            if p == active[0]:
                tile = T(tile, order, descending, fault)
            pad = T(np.array([ONES]), order, descending, fault)[0] if fault == "pads-transformed" and p == active[0] else ONES
            padded = np.concatenate([tile, np.full((-m) % 256, pad, np.uint32)])
            d = _byte(padded, p)
            perm = _stable(d)
            ds = d[perm]
            counts = np.bincount(ds, minlength=256)
            start = np.cumsum(counts) - counts
            q = np.arange(len(padded))
            to = base[ds] + q - start[ds]
            ok = (q < m) & (to < n)   # the device stores sorted positions q < m: with pads that are not largest, real keys are lost
            out = padded[perm][ok]
            last = p == active[-1] and not (fault == "no-inverse-before-copy-back" and len(active) % 2 == 1)
            ks[1 - src][to[ok]] = T_inverse(out, order, descending, fault) if last else out
            if vs[src] is not None:
                pv = np.concatenate([vs[src][t0:t0 + TILE], np.zeros((-m) % 256, np.uint32)])
                vs[1 - src][to[ok]] = pv[perm][ok]
            real = np.bincount(_byte(tile, p), minlength=256)   # tileCount: the pads are taken off digit 255
            base = base + real
        src = 1 - src
    return ks[src], vs[src]


def _reversed(form, k, v, order):
    k, v = form(k, v, order, False, None)
    return k[::-1].copy(), (None if v is None else v[::-1].copy())


def ordered_sort_model(keys, values, order, descending=False, count=None, fault=None):
    """(keys, values) as vrdxHipCmdOrderedSort[KeyValue][Indirect] leaves the caller's arrays: the bound is len(keys), `count`
    the device-side count (None: the direct forms)."""
    assert fault is None or fault in FAULTS, fault
    keys = np.asarray(keys, np.uint32)
    bound = len(keys)
    n = bound if count is None else min(count, bound)
    out_k = keys.copy()
    out_v = None if values is None else np.asarray(values, np.uint32).copy()
    k, v = keys[:n], (None if values is None else out_v[:n].copy())
    if fault == "descending-by-reversal" and descending:
        k, v = ordered_sort_model(k, v, order, False)
        out_k[:n], v = k[::-1], (None if v is None else v[::-1])
    elif bound <= ONE_WORKGROUP_MAX:
        if n != 0:
            out_k[:n], v = _in_lds(k, v, order, descending, fault)
    else:
        # order32_kernel | the unordered plan on the words | order32_kernel<INVERSE>
        forward = bound if fault == "transform-up-to-the-bound" else n
        out_k[:forward] = T(out_k[:forward], order, descending, fault)
        perm = _stable(out_k[:n])
        out_k[:n] = out_k[:n][perm]
        v = None if v is None else v[perm]
        out_k[:n] = T_inverse(out_k[:n], order, descending, fault)
    if out_v is not None:
        out_v[:n] = v
    return out_k, out_v


def segmented_ordered_model(keys, values, offsets, order, descending=False, fault=None):
    """(keys, values) as vrdxHipCmdOrderedSortSegmented[KeyValue] leaves the caller's arrays, maxElementCount = len(keys)"""
    assert fault is None or fault in FAULTS, fault
    keys = np.asarray(keys, np.uint32)
    out_k = keys.copy()
    out_v = None if values is None else np.asarray(values, np.uint32).copy()
    o = [int(x) for x in offsets]
    for b, e in zip(o[:-1], o[1:]):
        if not (b <= e <= len(keys)) or e - b < 2:
            continue
        form = _in_lds if e - b <= MID_MAX else _segment_lsd
        k, v = keys[b:e], (None if values is None else np.asarray(values, np.uint32)[b:e])
        if fault == "descending-by-reversal" and descending:
            k, v = _reversed(form, k, v, order)
        else:
            k, v = form(k, v, order, descending, fault)
        out_k[b:e] = k
        if out_v is not None:
            out_v[b:e] = v
    return out_k, out_v
