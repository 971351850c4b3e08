"""A plain-numpy model of the 64-bit sorts (vrdxHipCmdSort64[KeyValue]) and what their GPU tests share
(tests/test_sort64_gpu.py, tests/test_sort64_edges_gpu.py; tests/test_sort64_model.py checks the model without a GPU).

The model restates the composition of RecordSort64 (vrdx_api.cpp) step by step on host arrays, each 32-bit sort an
np.argsort(kind="stable"):

  keys-only   split (A = lo, B = hi) | sort (A, B) | sort (B, A) | merge (keys = B << 32 | A)
  key+value   split (A = lo, I = iota) | sort (A, I) | gather (A = hi of keys[I]) | sort (A, I) |
              permute (T = A << 32 | lo of keys[I], A = values[I]) | copy back (keys = T, values = A)

`fault` plants ONE in-bounds mistake in a step -- the mistakes the streaming kernels around the inner sorts could make
(every thread owns four consecutive elements, the last n mod 4 go one by one) -- so that the tests can show which inputs
tell a faulty sort from a right one, and which do not.
"""
import zlib

import numpy as np

import plan_model

FAULTS = ("value-is-index",        # permute writes I[j] instead of values[I[j]]
          "low-from-high",         # permute takes the high word of keys[I[j]] where it wants the low
          "merge-swaps-lanes",     # merge: elements 4t + 1 and 4t + 2 of every whole group of four exchange low words
          "tail-index",            # key+value split: the last n mod 4 elements all get the index of the first of them
          "tail-values-stale",     # copy back leaves the last n mod 4 values as they were
          "second-sort-unstable")  # the second sort reverses every run of equal high words


# ---- inputs --------------------------------------------------------------------------------------------------------------

PATTERNS = ["uniform", "high-constant", "low-constant", "identical", "descending", "8-distinct", "bit63-mixed", "tile-depth",
            "dup-high"]


def make_keys64(pattern, n, rng):
    if pattern == "uniform":
        return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    low = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    if pattern == "high-constant":
        return np.uint64(0xDEADBEEF << 32) | low
    if pattern == "low-constant":
        return (low << np.uint64(32)) | np.uint64(0x12345678)
    if pattern == "identical":
        return np.full(n, 0x8000000100000002, dtype=np.uint64)
    if pattern == "descending":  # strictly decreasing in both words
        return np.uint64(0xFFFFFFFFFFFFFFFF) - np.arange(n, dtype=np.uint64) * np.uint64(0x100000001)
    if pattern == "8-distinct":
        return rng.integers(0, 1 << 64, size=8, dtype=np.uint64)[rng.integers(0, 8, size=n)]
    if pattern == "bit63-mixed":  # the unsigned order: keys with bit 63 come last, whatever int64 makes of them
        small = rng.integers(0, 1 << 20, size=n, dtype=np.uint64)
        return small | (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63))
    if pattern == "tile-depth":  # a 16-bit tile id over the bits of a positive float depth
        tile = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
        depth = (rng.random(n, dtype=np.float32) * np.float32(100.0) + np.float32(0.1)).view(np.uint32).astype(np.uint64)
        return (tile << np.uint64(32)) | depth
    if pattern == "dup-high":
        # 37 high words (long runs for the second sort, whose order only the low words and the stability decide) over
        # uniform low words, and every fifth key an exact 64-bit copy of a key drawn at random (ties that only the
        # values tell apart)
        high = rng.integers(0, 1 << 32, size=37, dtype=np.uint64)[rng.integers(0, 37, size=n)]
        keys = (high << np.uint64(32)) | low
        source = rng.integers(0, max(n, 1), size=len(keys[::5]))
        keys[::5] = keys.copy()[source]
        return keys
    raise ValueError(pattern)


def payload64(n):
    """Values that are not their own index anywhere: one cycle through 0 ... n - 1 in a random order (a permutation without
    fixed points for n >= 2) with the top bit set, and a 0xFFFFFFFF and a 0 among them, planted as segmented_cases.payload
    does.  A sort that hands out the index for the value, or reads the values at another base, cannot pass with them."""
    v = np.zeros(n, dtype=np.uint32)
    if n > 0:
        order = np.random.default_rng(n).permutation(n).astype(np.uint32)
        v[order] = np.roll(order, -1)  # order[k] -> order[k + 1]
    v ^= np.uint32(0x80000000)
    if n > 1:
        v[n // 3] = 0xFFFFFFFF
        v[(2 * n) // 3 + (n // 3 == (2 * n) // 3)] = 0
    return v


def case_inputs(pattern, n):
    """The keys and values of one case of the GPU tests: the same arrays wherever the case is run, with or without a GPU."""
    rng = np.random.default_rng(zlib.crc32(f"sort64/{pattern}/{n}".encode()))
    return make_keys64(pattern, n, rng), payload64(n)


def with_tail(keys, values, extra=3):
    """the arrays with `extra` elements behind them that a sort of len(keys) elements must leave alone: keys that would
    come first if they were sorted along, in descending order"""
    tail = np.arange(extra, 0, -1, dtype=np.uint64)
    return (np.concatenate([keys, tail]),
            None if values is None else np.concatenate([values, (tail + np.uint64(0x70000000)).astype(np.uint32)]))


# The cases of tests/test_sort64_edges_gpu.py (the alignments are the device's business: the host arrays are the same)
VALUE_PATTERNS = ["dup-high", "identical", "8-distinct", "tile-depth"]
VALUE_SIZES = [5, 1027, 16385, (1 << 18) + 3, 8_200_001]
MATRIX_BLOCKS = [1, 37]               # n = 1024 k + r, r = 0 ... 3: one workgroup of the streaming kernels, and several
TINY_SIZES = [1, 2, 3, 4, 5, 7, 8]
EDGE_SIZES = list(range(1020, 1029)) + [2047, 2048, 2049]   # the thread with the scalar tail: last of a workgroup, first of the next


def small_cases(limit=2049):
    """(pattern, n) of every input the edge tests run at n <= limit"""
    cases = [(p, n) for p in VALUE_PATTERNS for n in VALUE_SIZES if n <= limit]
    sizes = [1024 * k + r for k in MATRIX_BLOCKS for r in range(4)] + TINY_SIZES + EDGE_SIZES
    cases += [("dup-high", n) for n in sorted(set(sizes)) if n <= limit and ("dup-high", n) not in cases]
    return cases


# ---- the reference and the check -----------------------------------------------------------------------------------------

def expected64(keys, values):
    if values is None:
        return np.sort(keys), None
    order = np.argsort(keys, kind="stable")
    return keys[order], values[order]


def check64(got_keys, got_values, keys, values, count=None, want=None):
    """`want`: expected64 of the first `count` elements where the caller has it already"""
    n = len(keys) if count is None else count
    want_keys, want_values = want if want is not None else expected64(keys[:n], None if values is None else values[:n])
    assert np.array_equal(got_keys[:n], want_keys)
    assert np.array_equal(got_keys[n:], keys[n:]), "keys behind elementCount changed"
    if values is not None:
        assert np.array_equal(got_values[:n], want_values)
        assert np.array_equal(got_values[n:], values[n:]), "values behind elementCount changed"


# ---- the model -----------------------------------------------------------------------------------------------------------

def _stable(words):
    return np.argsort(words, kind="stable")


def _runs_reversed(words):
    """a sort that is right about the keys and wrong about ties: every run of equal keys comes out back to front"""
    order = np.argsort(words, kind="stable")
    n = len(order)
    if n == 0:
        return order
    s = words[order]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    run = np.cumsum(np.concatenate([[True], s[1:] != s[:-1]])) - 1
    begin, end = starts[run], np.concatenate([starts[1:], [n]])[run]
    return order[begin + end - 1 - np.arange(n)]


def words_of(keys):
    keys = np.asarray(keys, dtype=np.uint64)
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), (keys >> np.uint64(32)).astype(np.uint32)


def join(high, low):
    return (high.astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)


def sort64_model(keys, values=None, fault=None):
    """(keys, values) as the recorded steps leave the caller's arrays; values None = vrdxHipCmdSort64."""
    assert fault is None or fault in FAULTS, fault
    n = len(keys)
    whole = n - n % 4  # the elements that move four to a thread
    second = _runs_reversed if fault == "second-sort-unstable" else _stable
    lo, hi = words_of(keys)
    if values is None:
        a, b = lo, hi                                       # split
        p = _stable(a); a, b = a[p], b[p]                   # sort (A, B)
        q = second(b); b, a = b[q], a[q]                    # sort (B, A)
        low = a.copy()                                      # merge
        if fault == "merge-swaps-lanes":
            low[1:whole:4], low[2:whole:4] = a[2:whole:4], a[1:whole:4]
        return join(b, low), None
    values = np.asarray(values, dtype=np.uint32)
    a, index = lo, np.arange(n, dtype=np.uint32)            # split with iota
    if fault == "tail-index":
        index[whole:] = whole
    p = _stable(a); a, index = a[p], index[p]               # sort (A, I)
    a = hi[index]                                           # gather
    q = second(a); a, index = a[q], index[q]                # sort (A, I)
    temp = join(a, hi[index] if fault == "low-from-high" else lo[index])   # permute
    a = index.copy() if fault == "value-is-index" else values[index]
    out = a.copy()                                          # copy back
    if fault == "tail-values-stale":
        out[whole:] = values[whole:]
    return temp, out


# ---- what the device decides about the second inner sort -----------------------------------------------------------------

def second_sort_keys(keys):
    """The keys of the second inner sort in the order it meets them: the high words as the stable sort by the low words
    left them (the MSD plan's sample reads 64 of them BY POSITION, so the order is part of the verdict)."""
    lo, hi = words_of(keys)
    return hi[_stable(lo)]


def second_sort_verdict(keys, plan, bits=0, msd_cap=0):
    """The VERDICT_* that vrdxHipReadPlanVerdict reports after a 64-bit sort of `keys`: that of the inner key+value sort over
    the high words, by plan_model's rules.  plan: the name vrdxHipDescribePlan gives for (len(keys), key+value); bits and
    msd_cap: the MSD plan's window width and bucket capacity."""
    n = len(keys)
    words = second_sort_keys(keys)
    if plan == "msd":
        return plan_model.msd_verdict(words, n, bits, msd_cap)[0]
    if plan == "hybrid-8":
        return plan_model.hybrid_verdict(words, n, plan_model.hybrid_capacity(n))[0]
    return plan_model.VERDICT_NONE
