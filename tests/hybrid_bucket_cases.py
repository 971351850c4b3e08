"""Inputs that reach the hybrid plan's kernels (launch 0 in its scatter role, bucket_sort_kernel and
SortInWorkgroup with bytes = t, in vrdx_kernels.hip) bucket by bucket, and a numpy restatement of the bucket kernel -- what
tests/test_hybrid_buckets_gpu.py runs and tests/test_hybrid_bucket_cases.py checks without a GPU.  A plain module next to
plan_model.py and msd_bucket_cases.py, imported the same way; no GPU, no torch.

The plan, the grids and the kernel forms depend on the BOUND of an indirect sort; the byte t the scatter ranks by, the verdict
and the 256 buckets follow on the DEVICE from the histogram of the keys the count covers.  So a bound that selects a kernel
form (FORMS) with a device count of at most 262 K keys runs the real kernels on buckets whose sizes and contents are chosen
here: build() gives every key the same bytes above t (plan_model.prefix_of), a designed digit in byte t and, below it, the
8 t bits its bucket lists in ARRIVAL order -- the order the bucket kernel loads them in, the scatter being stable.

What the kernel does with a bucket of n keys, restated (bucket_model):
  chunks = ceil(n / 256) chunks of four 64-key slots; wave w of 16 takes chunks / 16 (+ 1 for w < chunks % 16) of them,
  consecutive in memory (KPT >= 8, "DYN"; the 4096-key form gives wave w chunk w); positions from n on hold the pad: key
  0xFFFFFFFF, value 0.  t stable passes by the bytes 0 ... t - 1; in pass p the keys lie in the order pass p - 1 left.
  Positions below n are stored.  t = 0: a copy.
  RankAtomic, per chunk: `watch` = at most 48 lanes of the first slot differ from lane 0; per slot of a watched chunk:
  `uniform` = no lane differs from lane 0 (one lane adds 64); otherwise, if at most 48 lanes differ from lane 0 and they all
  hold ONE other digit, both groups are ranked by ballots (old0 / old1).
"""
import collections
import functools
import re

import numpy as np

import plan_model as model
from msd_bucket_cases import GUARD, PAD_KEY, payload, reference  # noqa: F401 (shared with the MSD plan's cases)

WAVES = 16   # bucket_sort_kernel<1024, ...>

# name; the indirect sort's bound; bucket capacity; keys per thread of the bucket kernel (DYN from 8); launch 0's tile
# geometry keys-only / key+value (vrdx_plan.h, ConfigIndex); the size of the form's filled direct sort (or None) and ITS
# launch-0 geometries; whether the ballot ranking has the form (its largest capacity is 16384)
Form = collections.namedtuple("Form", "name bound cap kpt config_keys config_kv filled filled_keys filled_kv ballot")
FORMS = {f.name: f for f in (
    Form("b4", 524_287, 4096, 4, "1024x8", "1024x8", 300_007, "1024x8", "1024x8", True),
    Form("b8", 1_048_575, 8192, 8, "1024x8", "1024x8", 1_048_575, "1024x8", "1024x8", True),
    Form("b16", 2_097_151, 16384, 16, "1024x16", "1024x8", 2_097_151, "1024x16", "1024x8", True),
    Form("b32-a", 2_097_155, 32768, 32, "1024x16", "1024x8", 2_500_003, "1024x16", "1024x16", False),
    Form("b32-b", 4_300_003, 32768, 32, "1024x32", "1024x16", None, None, None, False),     # (keys-only: even split)
    Form("b32-c", 8_144_383, 32768, 32, "1024x32", "1024x32", None, None, None, False))}


# ---- bucket contents: the 8 t low bits of a bucket's keys, in arrival order ----------------------------------------------

def _rand(rng, bits, size, exclude_ones=False):
    """uniform values of `bits` bits (exclude_ones: no BYTE of them is 0xFF)"""
    if bits == 0:
        return np.zeros(size, np.uint32)
    if not exclude_ones:
        return rng.integers(0, 1 << bits, size=size, dtype=np.uint64).astype(np.uint32)
    out = np.zeros(size, np.uint32)
    for byte in range(bits // 8):
        out |= rng.integers(0, 255, size=size, dtype=np.uint64).astype(np.uint32) << np.uint32(8 * byte)
    return out


def _distinct_neighbours(rng, count):
    """`count` byte values, no two neighbours equal"""
    steps = rng.integers(1, 256, size=count, dtype=np.uint64)
    return (np.cumsum(steps) & np.uint64(0xFF)).astype(np.uint32)


def _pick(rng, rows, counts):
    """[rows][64] booleans: in row r exactly counts[r] of lanes 1 ... 63 (never lane 0), chosen at random"""
    chosen = np.argsort(rng.random((rows, 63)), axis=1) < np.asarray(counts).reshape(-1, 1)
    return np.concatenate([np.zeros((rows, 1), bool), chosen], axis=1)


def _other(rng, mine, shape):
    """byte values that differ from `mine` (broadcast)"""
    return mine ^ rng.integers(1, 256, size=shape, dtype=np.uint64).astype(np.uint32)


# the digits ONE pass sees, position by position of that pass (slot = 64 consecutive positions, chunk = four slots)

def _d_runs(size, rng, length, lead):
    """runs of `length` positions with one digit each (neighbouring runs differ), the first run `lead` long"""
    run = (np.arange(size) + (length - lead)) // length
    return _distinct_neighbours(rng, int(run[-1]) + 1)[run]


def _d_first_slot(size, rng, uniform_first):
    """in every chunk either the first slot has one digit and the other three are random, or the other three have one
    digit each and the first is random"""
    pos = np.arange(size)
    per_slot = _distinct_neighbours(rng, size // 64 + 1)[pos // 64]
    return np.where((pos % 256 < 64) == uniform_first, per_slot, _rand(rng, 8, size)).astype(np.uint32)


def _d_probe(size, rng, differ):
    """the first slot of every chunk: exactly `differ` of lanes 1 ... 63 hold another digit than lane 0 (not ONE other
    digit: the slot is not two-valued); the other three slots are random"""
    chunks = -(-size // 256)
    d = _rand(rng, 8, 256 * chunks).reshape(chunks, 256)
    mine = _rand(rng, 8, chunks).reshape(chunks, 1)
    other = _other(rng, mine, (chunks, 64))
    other[:, 1::2] = mine ^ np.uint32(0x80)          # (at least two other digits among any three lanes: 0x80 and, on the
    other[:, 2::4] = mine ^ np.uint32(0x01)          # lanes 2, 6, 10, ..., 0x01)
    d[:, :64] = np.where(_pick(rng, chunks, np.full(chunks, differ)), other, mine)
    return d.ravel()[:size].copy()


def _d_pair(size, rng, second):
    """every slot holds two digits, `second` lanes (never lane 0) on the one lane 0 does not have -- in WATCHED chunks: with
    second > 48 the first slot of every chunk holds one digit only"""
    slots = -(-size // 64)
    mine = _distinct_neighbours(rng, slots).reshape(slots, 1)
    counts = np.full(slots, second)
    if second > 48:
        counts[::4] = 0
    d = np.where(_pick(rng, slots, counts), _other(rng, mine, (slots, 1)), mine)
    return d.ravel()[:size].astype(np.uint32)


def _d_lone(size, rng):
    """every slot: 63 lanes agree and one does not -- any lane, but never lane 0 in the first slot of a chunk, so that
    every chunk is watched, and lane 0 in the second"""
    slots = -(-size // 64)
    mine = _distinct_neighbours(rng, slots).reshape(slots, 1)
    lane = rng.integers(0, 64, size=slots)
    lane[::4] = rng.integers(1, 64, size=len(lane[::4]))
    lane[1::4] = 0   # (lane 0 alone: 63 lanes differ from it, the slot takes the plain path of a watched chunk)
    d = np.where(np.arange(64).reshape(1, 64) == lane.reshape(slots, 1), _other(rng, mine, (slots, 1)), mine)
    return d.ravel()[:size].astype(np.uint32)


def _in_pass(size, t, p, rng, digits):
    """8 t bits in arrival order whose byte p, read in the order pass p finds the keys in (arrival order for p = 0, else the
    stable order by the bytes below p, which are random), is `digits`; the bytes above p are random"""
    lower = _rand(rng, 8 * p, size)
    rank = np.empty(size, np.int64)
    rank[np.argsort(lower, kind="stable")] = np.arange(size)
    upper = _rand(rng, 8 * (t - p - 1), size)
    return lower | (digits[rank].astype(np.uint32) << np.uint32(8 * p)) | (upper << np.uint32(8 * (p + 1)))


def _thirds(size, bits, rng):
    """a third of the keys all ones, the first and the last arrival among them; the rest random"""
    low = _rand(rng, bits, size)
    low[::3] = (1 << bits) - 1
    low[size - 1:] = (1 << bits) - 1
    return low


_NAME = re.compile(r"^(?:pass(\d)-)?([a-z0-9+-]+?)(?:@(\d))?$")


def split_name(name, t):
    """(what, pass) of a content's name under t >= 1 bytes: "pass2-ones" and "lone-lane@2" name pass 2, a name without a
    pass names pass 0; a pass the bucket kernel does not run under this t is taken modulo t"""
    front, what, back = _NAME.match(name).groups()
    return what, int(front or back or 0) % t


def content(name, size, t, rng):
    """The 8 t bits below byte t of a bucket of `size` keys, in arrival order (uint32, < 2^(8 t)).  t = 0: nothing to choose."""
    if t == 0:
        return np.zeros(size, np.uint32)
    bits = 8 * t
    what, p = split_name(name, t)
    pos = np.arange(size, dtype=np.uint64)
    if what == "random":
        return _rand(rng, bits, size)
    if what == "all-equal":
        return np.full(size, _rand(rng, bits, 1)[0], np.uint32)
    if what == "zeros":
        return np.zeros(size, np.uint32)
    if what == "two-values":   # (they differ in every byte below t)
        a = _rand(rng, bits, 1)[0]
        return np.where(pos % 2 == 0, a, a ^ np.uint32(0x010101 & ((1 << bits) - 1))).astype(np.uint32)
    if what in ("ascending", "descending"):
        up = ((pos << np.uint64(bits)) // np.uint64(max(size, 1))).astype(np.uint32)
        return up if what == "ascending" else up[::-1].copy()
    if what == "pad-twins":
        return _thirds(size, bits, rng)
    if what == "all-pad-twins":
        return np.full(size, (1 << bits) - 1, np.uint32)
    if what == "ones":         # the pad's digit in pass p only: no other byte is 0xFF
        others = _rand(rng, bits, size, exclude_ones=True) & np.uint32(~(0xFF << (8 * p)) & 0xFFFFFFFF)
        return others | np.uint32(0xFF << (8 * p))
    if what == "uniform":      # byte p constant in the bucket, the others random
        return (_rand(rng, bits, size) & np.uint32(~(0xFF << (8 * p)) & 0xFFFFFFFF)) | (_rand(rng, 8, 1)[0] << np.uint32(8 * p))
    if what == "runs64":
        digits = _d_runs(size, rng, 64, 64)
    elif what == "runs256":
        digits = _d_runs(size, rng, 256, 256)
    elif what == "runs64+1":   # every slot: 63 positions of one run, then the first of the next
        digits = _d_runs(size, rng, 64, 63)
    elif what == "first-slot-only-uniform":
        digits = _d_first_slot(size, rng, True)
    elif what == "first-slot-only-mixed":
        digits = _d_first_slot(size, rng, False)
    elif what in ("probe-48", "probe-49"):
        digits = _d_probe(size, rng, int(what[-2:]))
    elif what in ("pair-48", "pair-49"):
        digits = _d_pair(size, rng, int(what[-2:]))
    elif what == "lone-lane":
        digits = _d_lone(size, rng)
    else:
        raise ValueError(name)
    return _in_pass(size, t, p, rng, digits)


# the contents that take turns in the ladder's buckets; "@p" and "pass{p}-": the pass the content is laid out for
ROTATION = ("random", "all-equal", "zeros", "ascending", "descending", "two-values", "pad-twins", "all-pad-twins",
            "pass0-ones", "pass1-ones", "pass2-ones", "runs64", "runs256", "runs64+1", "first-slot-only-uniform",
            "first-slot-only-mixed", "probe-48", "probe-49", "pair-48", "pair-49", "lone-lane", "pass0-uniform",
            "pass1-uniform", "pass2-uniform", "probe-48@1", "probe-49@2", "pair-48@2", "pair-49@1", "lone-lane@1",
            "lone-lane@2", "runs64+1@1", "first-slot-only-uniform@2", "probe-48@2", "probe-49@1", "pair-48@1", "pair-49@2")


# ---- the builder -----------------------------------------------------------------------------------------------------

def build(t, buckets, order, seed):
    """The keys of one call.  buckets: {digit of byte t: the 8 t low bits of its keys in arrival order}, at least two of them
    non-empty (byte t must vary).  key = plan_model.prefix_of(8 (t + 1)) | digit << 8 t | low; t = 3 has no prefix.  order
    "merged" interleaves the buckets at random (seeded) and keeps each bucket's arrival order; "grouped" places bucket after
    bucket, in the order `buckets` lists them: whole scatter tiles of one digit."""
    rng = np.random.default_rng(seed)
    assert 0 <= t <= 3 and all(0 <= b < 256 for b in buckets)
    buckets = {b: np.asarray(v, dtype=np.uint32) for b, v in buckets.items()}
    assert all(int(v.max(initial=0)) < (1 << (8 * t)) for v in buckets.values())
    assert sum(1 for v in buckets.values() if len(v)) >= 2
    ids = np.concatenate([np.full(len(v), b, np.uint32) for b, v in buckets.items()])
    if order == "merged":
        ids = ids[rng.permutation(len(ids))]
    else:
        assert order == "grouped"
    # bucket b's keys take the positions that hold b, ascending: the stable order of the positions by digit, filled with
    # the buckets' lists in ascending order of the digit
    low = np.empty(len(ids), np.uint32)
    low[np.argsort(ids.astype(np.uint8), kind="stable")] = np.concatenate([buckets[b] for b in sorted(buckets)])
    high = np.uint32(model.prefix_of(8 * (t + 1)) if t < 3 else 0)
    return high | (ids << np.uint32(8 * t)) | low


def byte_histogram(keys, t):
    return np.bincount((keys >> np.uint32(8 * t)) & np.uint32(0xFF), minlength=256)


# ---- the cases -------------------------------------------------------------------------------------------------------

def ladder_sizes(form):
    """one bucket size either side of every edge of SortInWorkgroup's chunk dealing (W = 16 waves) and of the capacity; for
    32768 also either side of one interior multiple of 256 W"""
    w, cap = WAVES, form.cap
    sizes = [1, 2, 63, 64, 65, 255, 256, 257,
             256 * (w - 1) + 1, 256 * w - 1, 256 * w, 256 * w + 1, 256 * (w + 1), 256 * (w + 1) + 1, 256 * (2 * w - 1),
             256 * (2 * w - 1) + 1, 512 * w, 512 * w + 1]
    if cap == 32768:
        sizes += [256 * 5 * w, 256 * 5 * w + 1]
    sizes += [cap - 256, cap - 255, cap - 1, cap]
    return tuple(sorted(set(s for s in sizes if s <= cap)))


# The digits of the ladder's buckets, the same for every form: 0, 1, 254 and 255, the rest spread out.  They take, in this
# order, cap - 255, 1, cap and 257 keys, then the other sizes ascending.
LADDER_DIGITS = (0, 1, 254, 255, 17, 128, 64, 200, 33, 99, 150, 230, 7, 77, 111, 180, 222, 45, 141, 166, 91, 240, 58, 127)
OVERFLOW_DIGIT = 0x5A          # not a ladder digit
TWO_DIGITS = (0xC3, 0x3C)      # (listed high digit first: "grouped" would place them against the sorted order)


def ladder(form):
    """{digit: size}"""
    sizes = ladder_sizes(form)
    ends = [form.cap - 255, 1, form.cap, 257]
    return dict(zip(LADDER_DIGITS, ends + [s for s in sizes if s not in ends]))


# name; form; t; order; buckets = ((digit, content, size), ...); the model's verdict; direct = the size of a direct sort
# (no count word) or None
Case = collections.namedtuple("Case", "name form t order buckets verdict direct")


def _case(name, form, t, order, buckets, verdict=model.VERDICT_HYBRID_RUNS, direct=None):
    return Case(f"{name}-{form.name}-t{t}-{order}", form, t, order, tuple(buckets), verdict, direct)


def ladder_content(index, turn, key_value):
    """The contents rotate over the ladder's buckets with the turn, and the key+value sweep is one step ahead of the
    keys-only one: over len(ROTATION) turns every bucket holds every content, in either mode."""
    return ROTATION[(index + turn + (1 if key_value else 0)) % len(ROTATION)]


def _ladder_buckets(form, turn, key_value):
    return [(digit, ladder_content(i, turn, key_value), size) for i, (digit, size) in enumerate(ladder(form).items())]


def ladder_case(form, key_value, t, turn, order="merged"):
    """the whole ladder in one call (key+value at turn k holds the keys of keys-only at turn k + 1)"""
    step = (turn + (1 if key_value else 0)) % len(ROTATION)
    return _case(f"ladder{step}", form, t, order, _ladder_buckets(form, turn, key_value))


def top_sizes(form):
    return (257, form.cap - 1, form.cap)


def top_case(form, size):
    """t = 3 with real 0xFFFFFFFF keys -- the pad itself -- in bucket 255 and real zeros in bucket 0"""
    return _case(f"top{size}", form, 3, "merged", [(0, "zeros", 1025), (255, "pad-twins", size)])


def two_bucket_case(form, t, second):
    """only two digits occur -- launch 0 ranks a two-valued byte -- with cap keys and `second` (1 or cap) keys"""
    return _case(f"two{second}", form, t, "merged",
                 [(TWO_DIGITS[0], "pad-twins", form.cap), (TWO_DIGITS[1], "descending", second)])


def overflow_case(form, t):
    """one bucket one key beyond the capacity among the ladder's: the plan is turned down and the four passes sort"""
    buckets = _ladder_buckets(form, 5, False) + [(OVERFLOW_DIGIT, "random", form.cap + 1)]
    return _case("overflow", form, t, "merged", buckets, verdict=model.VERDICT_HYBRID_DECLINED)


def filled_case(form, key_value, t):
    """a direct sort of form.filled elements: the ladder's buckets, every other digit filled evenly with random keys"""
    n = form.filled
    mine = _ladder_buckets(form, 11, key_value)
    others = [d for d in range(256) if d not in dict(ladder(form))]
    rest = n - sum(size for _, _, size in mine)
    share, more = divmod(rest, len(others))
    assert 0 < share and share + 1 <= form.cap, (form.name, share)
    mine += [(d, "random", share + (1 if i < more else 0)) for i, d in enumerate(others)]
    step = (11 + (1 if key_value else 0)) % len(ROTATION)
    return _case(f"filled{step}", form, t, "merged", mine, direct=n)


LADDER_TS = (3, 2, 1, 0)
GROUPED = ((3, 0), (3, 16), (1, 7), (1, 19))   # (t, turn)
BALLOT = [(t, turn) for t in (3, 1) for turn in (0, 9, 17, 26)]
OVERFLOW_TS = (3, 1, 0)
FILLED_TS = (3, 2, 0)


def gpu_cases(form, key_value):
    """every case tests/test_hybrid_buckets_gpu.py runs on the one-atomic sorter for one form and mode"""
    cases = [ladder_case(form, key_value, t, turn) for t in LADDER_TS for turn in range(len(ROTATION))]
    cases += [ladder_case(form, key_value, t, turn, order="grouped") for t, turn in GROUPED]
    cases += [top_case(form, size) for size in top_sizes(form)]
    cases += [two_bucket_case(form, t, second) for t in LADDER_TS for second in (1, form.cap)]
    cases += [overflow_case(form, t) for t in OVERFLOW_TS]
    if form.filled is not None:
        cases += [filled_case(form, key_value, t) for t in FILLED_TS]
    return cases


def ballot_cases(form, key_value):
    return [ladder_case(form, key_value, t, turn) for t, turn in BALLOT]


def case_seed(case):
    """(no hash(): the same keys in every process; forms of one capacity share their keys)"""
    text = case.name.replace(case.form.name, str(case.form.cap))
    return sum(ord(c) * (i + 1) for i, c in enumerate(text))


def bucket_lows(case):
    """{digit: low bits in arrival order} of a case"""
    rng = np.random.default_rng(case_seed(case) + 1)
    return {digit: content(name, size, case.t, rng) for digit, name, size in case.buckets}


@functools.lru_cache(maxsize=4)
def _keys(cap, t, order, buckets, seed):
    rng = np.random.default_rng(seed + 1)
    keys = build(t, {digit: content(name, size, t, rng) for digit, name, size in buckets}, order, seed)
    keys.setflags(write=False)
    return keys


def case_keys(case):
    """(read-only: shared between the callers of one process)"""
    return _keys(case.form.cap, case.t, case.order, case.buckets, case_seed(case))


# ---- the slot layout, for the tests of the contents ------------------------------------------------------------------

def pass_digits(low, t, p):
    """[slots][64]: the digits the ranking sees in pass p < t of a bucket -- slot = 64 consecutive positions, in arrival order
    in pass 0 and in the order pass p - 1 left in pass p, the pads (all ones) behind position n up to a whole chunk"""
    n = len(low)
    padded = np.full(-(-n // 256) * 256, (1 << (8 * t)) - 1, np.uint32)
    padded[:n] = low
    if p:
        padded = padded[np.argsort(padded & np.uint32((1 << (8 * p)) - 1), kind="stable")]
    return ((padded >> np.uint32(8 * p)) & np.uint32(0xFF)).reshape(-1, 64)


def slot_census(digits):
    """dict(uniform = slots with one digit; lone = slots in which all lanes but one hold one digit; lone0 = those of them
    where lane 0 is among the 63; probe = per chunk, the lanes of its first slot that differ from lane 0; pair = per slot the
    lanes that differ from lane 0 if they all hold ONE other digit, else -1; watched = per slot, whether its chunk is)"""
    same = (digits == digits[:, :1]).sum(axis=1)
    ordered = np.sort(digits, axis=1)
    distinct = 1 + (ordered[:, 1:] != ordered[:, :-1]).sum(axis=1)
    most = np.maximum(same, 64 - same)
    probe = 64 - same[::4]
    return dict(uniform=int((same == 64).sum()), lone=int(((distinct == 2) & (most == 63)).sum()),
                lone0=int(((distinct == 2) & (same == 63)).sum()), probe=probe,
                pair=np.where(distinct == 2, 64 - same, -1), watched=np.repeat(probe <= 48, 4))


# ---- bucket_sort_kernel + SortInWorkgroup in numpy, with plantable faults ---------------------------------------------

FAULTS = ("pads-first", "later-pass-unstable", "lone-lane-uniform", "pair-second-from-first", "dropped-chunk",
          "stale-value-ranks", "one-pass-short")


def wave_of_chunk(chunks, waves, dyn):
    """the wave that takes each chunk: dealt out evenly, consecutive (DYN); else wave w takes chunk w"""
    if not dyn:
        return np.arange(chunks)
    base, extra = divmod(chunks, waves)
    return np.repeat(np.arange(waves), base + (np.arange(waves) < extra))


def bucket_model(keys, values, t, waves, fault=None, dyn=True):
    """One bucket: pad to whole chunks, t stable passes by the bytes 0 ... t - 1, the positions below n.  Faults:
      pads-first              (1) pads rank in front of the real keys of digit 0xFF;
      later-pass-unstable     (2) a pass p >= 1 ranks equal digits in reverse order;
      lone-lane-uniform       (3) a slot of a watched chunk in which lane 0's digit is that of 63 lanes is ranked as uniform:
                              the 64th key is placed as if it had that digit too;
      pair-second-from-first  (4) in a two-valued slot of a watched chunk (at most 48 lanes on the digit lane 0 does not
                              have) the second group takes the first group's counter: old0 where old1 belongs -- its keys
                              land on other keys' places, and the places they leave keep what the pass before left there;
      dropped-chunk           (5) the last wave that is dealt a chunk more than the others (w = chunks % waves - 1) leaves it
                              out: its keys are neither ranked nor stored, the others close up (dyn only);
      stale-value-ranks       (6) a pass p >= 1 moves the values by the positions of pass p - 1;
      one-pass-short          (7) byte t - 1 is not ranked."""
    n = len(keys)
    chunks = -(-n // 256)
    total = 256 * chunks
    k = np.full(total, PAD_KEY, np.uint32)
    v = np.zeros(total, np.uint32)
    k[:n], v[:n] = keys, values
    pad = np.arange(total) >= n
    index = np.arange(total)
    dead = np.zeros(total, bool)
    if fault == "dropped-chunk" and dyn and chunks % waves:
        base, extra = divmod(chunks, waves)
        last = (extra - 1) * (base + 1) + base   # wave extra - 1 starts at chunk w (base + 1) and takes base + 1
        dead[256 * last:256 * (last + 1)] = True
    dropped = dead.copy()
    wave = np.repeat(wave_of_chunk(chunks, waves, dyn), 256)
    before = None
    for p in range(t - 1 if fault == "one-pass-short" else t):
        d = ((k >> np.uint32(8 * p)) & np.uint32(0xFF)).astype(np.uint8)   # (numpy sorts bytes by radix: stable and fast)
        slots = d.reshape(-1, 64)   # (a view)
        census = slot_census(slots) if fault in ("lone-lane-uniform", "pair-second-from-first") else None
        moved = {}
        if fault == "lone-lane-uniform":
            same = (slots == slots[:, :1]).sum(axis=1)
            hit = census["watched"] & (same == 63)
            slots[hit] = slots[hit, :1]
        if fault == "pair-second-from-first":
            for s in np.flatnonzero(census["watched"] & (census["pair"] >= 1) & (census["pair"] <= 48)).tolist():
                row = slots[s]
                second = np.flatnonzero(row != row[0])
                start = int(np.flatnonzero(wave == wave[64 * s])[0])     # the wave's counters count from its first slot
                seen = d[start:64 * s]
                old0, old1 = int((seen == row[0]).sum()), int((seen == row[second[0]]).sum())
                if old0 != old1:
                    moved[s] = (second + 64 * s, old0 - old1)
        if fault == "pads-first":
            order = np.lexsort((index, ~pad, d))
        elif fault == "later-pass-unstable" and p >= 1:
            order = np.lexsort((-index, d))
        else:
            order = np.argsort(d, kind="stable")
        if fault == "dropped-chunk":
            order = np.concatenate([order[~dead[order]], np.flatnonzero(dead)])   # (the survivors close up)
        if not moved and fault != "stale-value-ranks":   # every key to the place its rank names: a permutation
            k, v, pad, dead = k[order], v[order], pad[order], dead[order]
            continue
        to = np.empty(total, np.int64)
        to[order] = index
        for where, shift in moved.values():
            to[where] = np.clip(to[where] + shift, 0, total - 1)
        stale_k, stale_v = (k, v) if p else (np.full(total, GUARD, np.uint32), np.full(total, GUARD, np.uint32))
        new_k, new_v, new_pad, new_dead = stale_k.copy(), stale_v.copy(), pad.copy(), dead.copy()
        new_k[to], new_pad[to], new_dead[to] = k, pad, dead
        new_v[before if fault == "stale-value-ranks" and p >= 1 else to] = v
        k, v, pad, dead, before = new_k, new_v, new_pad, new_dead, to
    if dropped.any():   # nothing is stored for the positions of the chunk left out, nothing sorted arrives behind the survivors
        lost = dropped | dead
        k[lost], v[lost] = GUARD, GUARD
    return k[:n], v[:n]


def call_model(keys, values, form, t, fault=None):
    """A whole call: the stable scatter by byte t, then every bucket by bucket_model -- or, with a bucket beyond the
    capacity, four stable passes by the four bytes."""
    digit = ((keys >> np.uint32(8 * t)) & np.uint32(0xFF)).astype(np.uint8)
    counts = np.bincount(digit, minlength=256)
    if int(counts.max()) > form.cap:
        k, v = keys, values
        for p in range(4):
            order = np.argsort(((k >> np.uint32(8 * p)) & np.uint32(0xFF)).astype(np.uint8), kind="stable")
            k, v = k[order], v[order]
        return k, v
    order = np.argsort(digit, kind="stable")
    k, v = keys[order], values[order]
    start = 0
    for end in np.cumsum(counts).tolist():
        if end > start:
            k[start:end], v[start:end] = bucket_model(k[start:end], v[start:end], t, WAVES, fault, dyn=form.kpt >= 8)
        start = end
    return k, v
