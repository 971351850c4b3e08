"""What the tests of the sorts of 32-bit keys with 64-bit values share (vrdxHipCmdWideValueSort[Indirect]): the reference, the
key builders, the values, and a plain-numpy model of the three device forms with plantable faults
(tests/test_wide_value_cases.py checks reference and model without a GPU; tests/test_wide_value_gpu.py holds the device to the
same reference on the same kinds of keys).

The reference: order = np.argsort(keys[:n], kind="stable"); keys[order] and values[order]; elements from n on as they were.

The model restates the device (vrdx_kernels.hip, vrdx_plan.h):
  one workgroup  small_sort_wide_kernel: n <= 8192.  The elements are padded to whole chunks of 256 with key 0xFFFFFFFF, LAST
                 in memory order; the OR of key ^ key[0] over the REAL elements says which bytes vary; one stable pass per
                 varying byte moves key, value low and value high together; the first n slots are stored.
  gather         A[i] = i; stable sort of (keys, A); T[j] = values[A[j]]; values[j] = T[j].
  two sorts      A = keys, B = value low, C = value high; stable sort of (A, B); stable sort of (keys, C);
                 values[i] = C[i] << 32 | B[i].
The streaming steps take four elements per thread and the last n mod 4 one by one.
`fault` plants ONE mistake the kernels or the recorder could make."""
import numpy as np

ONE_WORKGROUP_MAX = 8192   # kWideSmallMaxElements (vrdx_kernels.h)
ONES = np.uint32(0xFFFFFFFF)
LOW = np.uint64(0xFFFFFFFF)
SHIFT = np.uint64(32)

FAULTS = ("value-words-swapped",           # the merge / the store puts the low word on top
          "high-word-from-unsorted",       # the high word is taken from the element's position before the sort
          "gather-by-position",            # T[j] = values[j] instead of values[A[j]]
          "second-sort-on-sorted-copy",    # the second inner sort runs on the key copy the first one has already sorted
          "scalar-tail-dropped",           # the streaming steps leave the last n mod 4 elements out
          "pad-stored",                    # the one-workgroup form stores its pads too: it writes behind element n
          "constant-byte-from-all-slots")  # the mask of varying bytes is taken over first ^ last key only: a byte that varies
#                                            in between is skipped as "constant"

BUILDERS = ("uniform", "three", "equal", "all_ones", "descending", "byte2")


def make_keys(builder, n, rng):
    if builder == "uniform":
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if builder == "three":       # stability shows in the values
        return rng.choice(np.array([7, 0x80000001, 0xFFFFFFFE], np.uint32), size=n)
    if builder == "equal":
        return np.full(n, 0x12345678, np.uint32)
    if builder == "all_ones":    # ties with the pads
        return np.full(n, ONES, np.uint32)
    if builder == "descending":
        return np.uint32(0xFFFFFFF0) - np.arange(n, dtype=np.uint32) * np.uint32(3)
    if builder == "byte2":       # only byte 2 varies
        return (rng.integers(0, 256, size=n, dtype=np.uint64).astype(np.uint32) << np.uint32(16)) | np.uint32(0x5A00A55A)
    raise ValueError(builder)


def make_values(n, rng):
    """never the index: random 64-bit words whose halves differ, a few with a half of 0 or 0xFFFFFFFF"""
    v = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    v[(v >> SHIFT) == (v & LOW)] ^= np.uint64(1)
    edges = (0x00000000DEADBEEF, 0xFFFFFFFF12345678, 0x87654321FFFFFFFF, 0xCAFEF00D00000000)
    for at, word in zip(range(0, n, max(1, n // 7)), edges):
        v[at] = word
    return v


def expected(keys, values, count=None):
    keys, values = np.asarray(keys, np.uint32).copy(), np.asarray(values, np.uint64).copy()
    n = len(keys) if count is None else min(count, len(keys))
    order = np.argsort(keys[:n], kind="stable")
    keys[:n], values[:n] = keys[:n][order], values[:n][order]
    return keys, values


def form_of(bound, two_sorts_from, small_sort=True):
    if bound == 0:
        return "none"
    if bound <= ONE_WORKGROUP_MAX and small_sort:
        return "one-workgroup"
    return "gather" if bound < two_sorts_from else "two-sorts"


def _streamed(n, fault):
    """the elements a streaming step touches"""
    return n - n % 4 if fault == "scalar-tail-dropped" else n


def _stable_pass(words, shift, *arrays):
    order = np.argsort((words >> np.uint32(shift)) & np.uint32(0xFF), kind="stable")
    return [a[order] for a in arrays]


def _one_workgroup(keys, values, n, fault):
    if n == 0:
        return
    slots = -(-n // 256) * 256
    k = np.full(slots, ONES, np.uint32)
    lo, hi = np.full(slots, ONES, np.uint32), np.full(slots, ONES, np.uint32)   # (a pad's value is never looked at)
    k[:n] = keys[:n]
    lo[:n], hi[:n] = (values[:n] & LOW).astype(np.uint32), (values[:n] >> SHIFT).astype(np.uint32)
    hi_in = hi.copy()
    if fault == "constant-byte-from-all-slots":
        varying = int(k[0] ^ k[n - 1])
    else:
        varying = int(np.bitwise_or.reduce(k[:n] ^ k[0]))
    for shift in (0, 8, 16, 24):
        if (varying >> shift) & 0xFF:
            k, lo, hi = _stable_pass(k, shift, k, lo, hi)
    if fault == "high-word-from-unsorted":
        hi = hi_in
    if fault == "value-words-swapped":
        lo, hi = hi, lo
    stored = min(slots, len(keys)) if fault == "pad-stored" else n
    keys[:stored] = k[:stored]
    values[:stored] = (hi[:stored].astype(np.uint64) << SHIFT) | lo[:stored].astype(np.uint64)


def _gather(keys, values, n, fault):
    m = _streamed(n, fault)
    a = np.full(n, 0, np.uint32)          # (what the storage held: the model's scratch starts as zeros)
    a[:m] = np.arange(m, dtype=np.uint32)
    order = np.argsort(keys[:n], kind="stable")
    keys[:n], a = keys[:n][order], a[order]
    t = np.zeros(n, np.uint64)
    t[:m] = values[:m] if fault == "gather-by-position" else values[a[:m]]
    if fault == "high-word-from-unsorted":
        t[:m] = (values[:m] & ~LOW) | (t[:m] & LOW)
    if fault == "value-words-swapped":
        t = (t << SHIFT) | (t >> SHIFT)
    values[:m] = t[:m]


def _two_sorts(keys, values, n, fault):
    m = _streamed(n, fault)
    a, b, c = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    a[:m] = keys[:m]
    b[:m], c[:m] = (values[:m] & LOW).astype(np.uint32), (values[:m] >> SHIFT).astype(np.uint32)
    c_in = c.copy()
    first = np.argsort(a, kind="stable")
    a, b = a[first], b[first]
    if fault == "second-sort-on-sorted-copy":
        second = np.argsort(a, kind="stable")   # the identity: C stays where it was, and the caller's keys stay unsorted
        c = c[second]
    else:
        second = np.argsort(keys[:n], kind="stable")
        keys[:n], c = keys[:n][second], c[second]
    if fault == "high-word-from-unsorted":
        c = c_in
    if fault == "value-words-swapped":
        b, c = c, b
    values[:m] = (c[:m].astype(np.uint64) << SHIFT) | b[:m].astype(np.uint64)


def wide_value_model(keys, values, bound=None, count=None, two_sorts_from=1 << 22, small_sort=True, fault=None):
    """The call on the FULL arrays: bound = elementCount / maxElementCount (default: all of keys), count = the device's word
    (default: the bound), clamped to the bound.  Returns (keys, values) as the model leaves them."""
    keys, values = np.asarray(keys, np.uint32).copy(), np.asarray(values, np.uint64).copy()
    bound = len(keys) if bound is None else bound
    n = bound if count is None else min(count, bound)
    form = form_of(bound, two_sorts_from, small_sort)
    if form == "one-workgroup":
        _one_workgroup(keys, values, n, fault)
    elif form == "gather":
        _gather(keys, values, n, fault)
    elif form == "two-sorts":
        _two_sorts(keys, values, n, fault)
    return keys, values
