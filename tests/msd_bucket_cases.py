"""Inputs that reach the MSD plan's bucket kernels (BucketSort2Bucket in vrdx_kernels.hip) bucket by bucket, and a numpy
restatement of that function -- what tests/test_msd_buckets_gpu.py runs and tests/test_msd_bucket_cases.py checks without a
GPU.  A plain module next to plan_model.py, imported the same way.

The plan, its grids and its kernel forms depend on the BOUND of an indirect sort, the window and the buckets on the keys the
DEVICE count covers: under a bound of 8.6 M ... 37 M keys a count of 90 K ... 170 K keys runs the real kernels on buckets
whose sizes and contents are chosen here.  build() lays the keys out so that the sample (plan_model.sample_indices) sees 64
distinct window digits -- the window lies where the case wants it and the skew rule cannot fire -- and every other position
holds a designed key: a bucket is given as the bits BELOW the window of its keys in arrival order, which is the order the
bucket kernel loads them in (the scatter is stable).

What the kernel does with a bucket of n keys, restated (bucket_model):
  chunks = ceil(n / 256) chunks of four 64-key slots, dealt chunks / WAVES (+ 1 for w < chunks % WAVES) to the waves, in
  memory order; positions from n on hold the pad: key 0xFFFFFFFF, value 0.  Two stable passes by W0 = (below + 1) / 2 and
  W1 = below / 2 bits; between them the keys lie in pass-0 order.  Positions below n are stored.
  RankPacked16, per chunk: `watch` = at most 48 lanes of the first slot differ from lane 0; per slot of a watched chunk:
  `uniform` = no lane differs from lane 0 (one lane adds 64).
"""
import collections

import numpy as np

import plan_model as model
from segmented_cases import payload  # noqa: F401 (values: all different, top bit set, a 0 and a 0xFFFFFFFF among them)

GUARD = 0x5A5A5A5A
PAD_KEY = 0xFFFFFFFF

# name, the indirect sort's bound, the window's bits, bucket capacity, waves of the bucket kernel, recorded launches
Form = collections.namedtuple("Form", "name bound bits cap waves launches")
FORMS = {f.name: f for f in (Form("half", 8_600_003, 10, 18432, 8, 7),
                             Form("full10", 19_000_001, 10, 36864, 16, 6),
                             Form("full10-streamed", 1 << 25, 10, 36864, 16, 6),
                             Form("eleven", 37_000_003, 11, 36864, 16, 6))}


def widths(below):
    """(W0, W1): the bits of the bucket kernel's two passes"""
    return (below + 1) // 2, below // 2


# ---- bucket contents: the `below` low bits of a bucket's keys, in arrival order ------------------------------------------

def _rand(rng, bits, size, exclude_ones=False):
    """uniform values of `bits` bits (exclude_ones: never all ones; bits >= 1)"""
    if bits == 0:
        return np.zeros(size, np.uint32)
    return rng.integers(0, (1 << bits) - (1 if exclude_ones else 0), size=size, dtype=np.uint64).astype(np.uint32)


def _distinct_neighbours(rng, bits, count):
    """`count` values of `bits` >= 1 bits, no two neighbours equal"""
    steps = rng.integers(1, 1 << bits, size=count, dtype=np.uint64)
    return (np.cumsum(steps) & np.uint64((1 << bits) - 1)).astype(np.uint32)


def _runs(size, below, rng, length, lead):
    """runs of `length` arrivals with one pass-0 digit each (neighbouring runs differ), the first run `lead` long"""
    w0, w1 = widths(below)
    run = (np.arange(size) + (length - lead)) // length
    return _distinct_neighbours(rng, w0, int(run[-1]) + 1 if size else 0)[run] | (_rand(rng, w1, size) << np.uint32(w0))


def _first_slot(size, below, rng, uniform_first):
    """in every chunk of 256 arrivals either the first slot of 64 has one pass-0 digit and the other three are random, or
    the other three have one digit each and the first is random"""
    w0, w1 = widths(below)
    pos = np.arange(size)
    first = pos % 256 < 64
    per_slot = _distinct_neighbours(rng, w0, size // 64 + 1)[pos // 64]
    digit = np.where(first == uniform_first, per_slot, _rand(rng, w0, size))
    return digit.astype(np.uint32) | (_rand(rng, w1, size) << np.uint32(w0))


def _probe(size, below, rng, differ):
    """the first slot of every chunk: exactly `differ` of lanes 1 ... 63 hold another pass-0 digit than lane 0"""
    w0, w1 = widths(below)
    digit = _rand(rng, w0, size)
    for start in range(0, size, 256):
        slot = digit[start:start + 64]   # (a view)
        mine = _rand(rng, w0, 1)[0]
        other = mine ^ (_rand(rng, w0, 64, exclude_ones=True) + np.uint32(1))
        lanes = 1 + rng.permutation(63)[:differ]
        full = np.full(64, mine, np.uint32)
        full[lanes] = other[lanes]
        slot[:] = full[:len(slot)]
    return digit | (_rand(rng, w1, size) << np.uint32(w0))


def _thirds(size, below, rng):
    """a third of the keys all ones below the window, the first and the last arrival among them; the rest random"""
    low = _rand(rng, below, size)
    low[::3] = (1 << below) - 1
    low[size - 1:] = (1 << below) - 1
    return low


def content(name, size, below, rng):
    """The bits below the window of a bucket of `size` keys, in arrival order (uint32, < 2^below)."""
    w0, w1 = widths(below)
    ones = np.uint32((1 << below) - 1)
    pos = np.arange(size, dtype=np.uint64)
    if name == "random":
        return _rand(rng, below, size)
    if name == "all-equal":
        return np.full(size, _rand(rng, below, 1)[0], np.uint32)
    if name == "zeros":
        return np.zeros(size, np.uint32)
    if name == "two-values":   # (they differ in both passes' digits)
        a = _rand(rng, below, 1)[0]
        return np.where(pos % 2 == 0, a, a ^ np.uint32((1 << w0) | 1)).astype(np.uint32)
    if name in ("ascending", "descending"):
        up = ((pos << np.uint64(below)) // np.uint64(max(size, 1))).astype(np.uint32)
        return up if name == "ascending" else up[::-1].copy()
    if name in ("pad-twins", "top-sentinels"):
        return _thirds(size, below, rng)
    if name == "all-pad-twins":
        return np.full(size, ones, np.uint32)
    if name == "pass0-ones":   # the pad's digit in pass 0 only
        return np.uint32((1 << w0) - 1) | (_rand(rng, w1, size, exclude_ones=True) << np.uint32(w0))
    if name == "pass1-ones":   # ... in pass 1 only
        return _rand(rng, w0, size, exclude_ones=True) | np.uint32(((1 << w1) - 1) << w0)
    if name == "runs64":
        return _runs(size, below, rng, 64, 64)
    if name == "runs256":
        return _runs(size, below, rng, 256, 256)
    if name == "runs64+1":     # every slot: 63 arrivals of one run, then the first of the next
        return _runs(size, below, rng, 64, 63)
    if name == "first-slot-only-uniform":
        return _first_slot(size, below, rng, True)
    if name == "first-slot-only-mixed":
        return _first_slot(size, below, rng, False)
    if name == "probe-48":
        return _probe(size, below, rng, 48)
    if name == "probe-49":
        return _probe(size, below, rng, 49)
    if name == "pass1-uniform":
        return _rand(rng, w0, size) | (_rand(rng, w1, 1)[0] << np.uint32(w0))
    if name == "pass0-uniform":
        return _rand(rng, w0, 1)[0] | (_rand(rng, w1, size) << np.uint32(w0))
    raise ValueError(name)


# the contents that take turns in the ladder's buckets (top-sentinels and zeros are placed by the cases that need them)
ROTATION = ("random", "all-equal", "two-values", "ascending", "descending", "pad-twins", "all-pad-twins", "pass0-ones",
            "pass1-ones", "runs64", "runs256", "runs64+1", "first-slot-only-uniform", "first-slot-only-mixed", "probe-48",
            "probe-49", "pass1-uniform", "pass0-uniform")


# ---- the builder -----------------------------------------------------------------------------------------------------

def build(bits, shift, prefix, buckets, order, seed):
    """The keys of one call.  buckets: {window digit: its keys' `shift` low bits in arrival order} (an empty array keeps a
    digit empty).  The 64 positions the sample reads hold 64 keys of 64 different digits -- digit 0 at index 0, digit
    2^bits - 1 at the end -- taken from the digits `buckets` does not name; a designed bucket 0 gives its first arrival to
    index 0 and a designed top bucket its last arrival to the last index.  Every other position holds a designed key:
    order "merged" interleaves the buckets at random (seeded) and keeps each bucket's arrival order, "grouped" places bucket
    after bucket.  A key is prefix's bits above shift + bits | digit << shift | low."""
    rng = np.random.default_rng(seed)
    nb = 1 << bits
    top = nb - 1
    assert 2 <= shift <= 32 - bits and all(0 <= b < nb for b in buckets)
    buckets = {b: np.asarray(v, dtype=np.uint32) for b, v in buckets.items()}
    assert all(int(v.max(initial=0)) < (1 << shift) for v in buckets.values())
    free = [b for b in range(1, top) if b not in buckets]
    ends = {b: buckets[b] for b in (0, top) if len(buckets.get(b, ()))}   # designed buckets that own a sample position
    assert all(b in ends or b not in buckets for b in (0, top)), "an EMPTY bucket 0 or top bucket cannot be designed"
    sample_digits = np.concatenate([[0], rng.choice(free, model.SAMPLE_KEYS - 2, replace=False), [top]]).astype(np.uint32)
    sample_low = _rand(rng, shift, model.SAMPLE_KEYS)
    body = dict(buckets)
    if 0 in ends:
        sample_low[0], body[0] = ends[0][0], ends[0][1:]
    if top in ends:
        sample_low[-1], body[top] = ends[top][-1], ends[top][:-1]
    ids = np.concatenate([np.full(len(v), b, np.uint32) for b, v in body.items()] + [np.zeros(0, np.uint32)])
    if order == "merged":
        ids = ids[rng.permutation(len(ids))]
    else:
        assert order == "grouped"
    low = np.empty(len(ids), np.uint32)
    for b, v in body.items():
        low[ids == b] = v   # (in arrival order: boolean assignment fills ascending positions)
    n = len(ids) + model.SAMPLE_KEYS
    sample = np.array(model.sample_indices(n))
    assert len(set(sample.tolist())) == model.SAMPLE_KEYS
    high = np.uint32(model.prefix_of(shift + bits, prefix) if shift + bits < 32 else 0)
    keys = np.empty(n, np.uint32)
    rest = np.ones(n, bool)
    rest[sample] = False
    keys[rest] = high | (ids << np.uint32(shift)) | low
    keys[sample] = high | (sample_digits << np.uint32(shift)) | sample_low
    return keys


def window_histogram(keys, bits, shift):
    return np.bincount((keys >> np.uint32(shift)) & np.uint32((1 << bits) - 1), minlength=1 << bits)


# ---- the cases -------------------------------------------------------------------------------------------------------

def ladder_sizes(form):
    """one bucket size either side of every edge of the kernel's chunk dealing (W = its waves) and of its capacity"""
    w, cap = form.waves, form.cap
    return (1, 2, 63, 64, 65, 255, 256, 257, 256 * w - 1, 256 * w, 256 * w + 1, 256 * (2 * w - 1), 256 * (2 * w - 1) + 1,
            cap - 256, cap - 255, cap - 1, cap)


# window digit -> index into ladder_sizes: digit 1 and the last but one; (b, b + 2^bits / 2) are the two buckets of one
# workgroup of the 1024-thread kernels: cap - 255 then 2, 1 then cap, 257 then cap - 1, 256 W - 1 then 256 (2W - 1) + 1;
# ten bits: 767 is the last bucket whose output the streamed form streams (a full one), 768 the first it does not.
LADDER_DIGITS = {10: {1: 14, 513: 1, 255: 0, 767: 16, 256: 7, 768: 15, 100: 8, 612: 12, 37: 2, 300: 3, 400: 4, 500: 5,
                      650: 6, 700: 9, 900: 10, 1000: 11, 1022: 13},
                 11: {1: 14, 1025: 1, 255: 0, 1279: 16, 256: 7, 1280: 15, 100: 8, 1124: 12, 37: 2, 300: 3, 400: 4, 500: 5,
                      1650: 6, 1700: 9, 1900: 10, 2000: 11, 2046: 13}}

# name; form; shift = the bits below the window; order; buckets = ((digit, content, size), ...); the model's verdict
Case = collections.namedtuple("Case", "name form shift order buckets verdict")


def _case(name, form, shift, order, buckets, verdict=model.VERDICT_MSD_RUNS):
    return Case(f"{name}-{form.name}-shift{shift}-{order}", form, shift, order, tuple(buckets), verdict)


def shifts_of(form):
    return range(2, 32 - form.bits + 1)


def ladder_content(index, shift, key_value):
    """The contents rotate over the ladder's buckets with the shift, and the key+value sweep is one step ahead of the
    keys-only one: over any 18 consecutive shifts x both modes every bucket holds every content under an odd and under an
    even `below`."""
    return ROTATION[(index + shift + (1 if key_value else 0)) % len(ROTATION)]


def ladder_case(form, key_value, shift, order="merged"):
    """the whole ladder in one call"""
    sizes = ladder_sizes(form)
    buckets = [(digit, ladder_content(i, shift, key_value), sizes[i]) for digit, i in LADDER_DIGITS[form.bits].items()]
    return _case("ladder" + ("-kv" if key_value else ""), form, shift, order, buckets)


def grouped_shifts(form):
    return (2, 11, 32 - form.bits)


def top_case(form, size):
    """the top window with real 0xFFFFFFFF keys in the top bucket and real zeros in bucket 0"""
    return _case(f"top{size}", form, 32 - form.bits, "merged",
                 [(0, "zeros", 4097), ((1 << form.bits) - 1, "top-sentinels", size)])


def top_sizes(form):
    return (257, form.cap - 1, form.cap)


def pair_case(form, shift):
    """the two buckets b and b + 2^bits / 2 that one workgroup of the 1024-thread kernel sorts one after the other"""
    assert form.waves == 16
    half, cap = (1 << form.bits) // 2, form.cap
    buckets = []
    for b, (first, second) in ((10, (("all-pad-twins", cap), ("random", 1))),
                               (255, (("random", 1), ("two-values", cap))),      # (767: the last streamed bucket)
                               (256, (("random", 0), ("pad-twins", 257))),       # (768: the first plain one)
                               (100, (("runs64+1", 4097), ("random", 0))),
                               (400, (("descending", cap), ("zeros", cap)))):
        buckets += [(b, *first), (b + half, *second)]
    return _case("pairs", form, shift, "merged", buckets)


def pair_shifts(form):
    return (3, 32 - form.bits)


def overflow_case(form):
    """one bucket one key beyond the capacity: the spine turns the plan down and the four passes sort"""
    return _case("overflow", form, 11, "merged", [(1, "pad-twins", 257), (333, "random", form.cap + 1), (700, "runs64", 4097)],
                 verdict=model.VERDICT_NONE)


def gpu_cases(form, key_value):
    """every case tests/test_msd_buckets_gpu.py runs for one form and mode"""
    cases = [ladder_case(form, key_value, s) for s in shifts_of(form)]
    cases += [ladder_case(form, key_value, s, order="grouped") for s in grouped_shifts(form)]
    cases += [top_case(form, size) for size in top_sizes(form)]
    if form.waves == 16:
        cases += [pair_case(form, s) for s in pair_shifts(form)]
    cases.append(overflow_case(form))
    return cases


def case_seed(case):
    return sum(ord(c) * (i + 1) for i, c in enumerate(case.name))   # (no hash(): the same keys in every process)


def bucket_lows(case):
    """{digit: low bits in arrival order} of a case"""
    rng = np.random.default_rng(case_seed(case) + 1)
    return {digit: content(name, size, case.shift, rng) for digit, name, size in case.buckets}


def case_keys(case):
    return build(case.form.bits, case.shift, model.PREFIX, bucket_lows(case), case.order, case_seed(case))


def reference(keys, values):
    order = np.argsort(keys, kind="stable")
    return keys[order], values[order]


# ---- the slot layout, for the tests of the contents ------------------------------------------------------------------

def pass_digits(low, below, which):
    """[slots][64]: the digits RankPacked16 sees in pass `which` of a bucket -- slot = 64 consecutive positions, in arrival
    order in pass 0 and in pass-0 order in pass 1, the pads (all ones) behind position n up to a whole chunk"""
    w0, w1 = widths(below)
    n = len(low)
    padded = np.full(-(-n // 256) * 256, (1 << below) - 1, np.uint32)
    padded[:n] = low
    d0 = padded & np.uint32((1 << w0) - 1)
    if which == 0:
        return d0.reshape(-1, 64)
    return (padded[np.argsort(d0, kind="stable")] >> np.uint32(w0)).reshape(-1, 64)


def slot_census(digits):
    """dict(uniform = slots with one digit, lone = slots where lane 0's digit is that of exactly 63 lanes, probe = per chunk
    the lanes of its first slot that differ from lane 0)"""
    same = (digits == digits[:, :1]).sum(axis=1)
    return dict(uniform=int((same == 64).sum()), lone=int((same == 63).sum()), probe=64 - same[::4])


# ---- BucketSort2Bucket in numpy, with plantable faults ---------------------------------------------------------------

FAULTS = ("pads-first", "pass1-unstable", "lone-lane-uniform", "dropped-chunk", "stale-value-ranks")


def bucket_model(keys, values, below, waves, fault=None):
    """One bucket: pad to whole chunks, two stable passes by W0 then W1 bits, the positions below n.  Faults:
      pads-first          (a) pads rank in front of the real keys of their digit;
      pass1-unstable      (b) pass 1 ranks equal digits in reverse order;
      lone-lane-uniform   (c) a slot of a watched chunk in which lane 0's digit is that of 63 lanes is ranked as uniform:
                          the 64th key is placed as if it had that digit too;
      dropped-chunk       (d) the last wave that is dealt a chunk more than the others (w = chunks % WAVES - 1) leaves it
                          out: its keys are neither ranked nor stored, the others close up;
      stale-value-ranks   (e) pass 1 moves the values by the positions of pass 0."""
    n = len(keys)
    chunks = -(-n // 256)
    total = 256 * chunks
    k = np.full(total, PAD_KEY, np.uint32)
    v = np.zeros(total, np.uint32)
    k[:n], v[:n] = keys, values
    pad = np.arange(total) >= n
    w0, w1 = widths(below)
    index = np.arange(total)
    dead = np.zeros(total, bool)
    if fault == "dropped-chunk" and chunks % waves:
        base, extra = divmod(chunks, waves)
        last = (extra - 1) * (base + 1) + base   # wave extra - 1 starts at chunk w (base + 1) and takes base + 1
        dead[256 * last:256 * (last + 1)] = True
    dropped = dead.copy()
    first_order = None
    for which, (shift, width) in enumerate(((0, w0), (w0, w1))):
        d = ((k >> np.uint32(shift)) & np.uint32((1 << width) - 1)).astype(np.int64)
        if fault == "lone-lane-uniform":
            slots = d.reshape(-1, 64)
            same = (slots == slots[:, :1]).sum(axis=1)
            watch = np.repeat(64 - same[::4] <= 48, 4)
            slots[watch & (same == 63)] = slots[watch & (same == 63), :1]   # (d is a view of slots)
        if fault == "pads-first":
            order = np.lexsort((index, ~pad, d))
        elif fault == "pass1-unstable" and which == 1:
            order = np.lexsort((-index, d))
        else:
            order = np.argsort(d, kind="stable")
        if fault == "dropped-chunk":
            order = np.concatenate([order[~dead[order]], np.flatnonzero(dead)])   # (the survivors close up)
        if which == 0:
            first_order = order
        k, pad, dead = k[order], pad[order], dead[order]
        v = v[first_order] if fault == "stale-value-ranks" else v[order]
    if dropped.any():   # nothing is stored for the positions of the chunk left out, nothing sorted arrives behind the survivors
        lost = dropped | dead
        k[lost], v[lost] = GUARD, GUARD
    return k[:n], v[:n]


def call_model(keys, values, form, shift, fault=None):
    """A whole call the plan takes: the stable scatter by the window, then every bucket by bucket_model."""
    digit = (keys >> np.uint32(shift)) & np.uint32((1 << form.bits) - 1)
    order = np.argsort(digit, kind="stable")
    k, v = keys[order], values[order]
    ends = np.cumsum(np.bincount(digit, minlength=1 << form.bits))
    start = 0
    for end in ends.tolist():
        if end > start:
            k[start:end], v[start:end] = bucket_model(k[start:end], v[start:end], shift, form.waves, fault)
        start = end
    return k, v
