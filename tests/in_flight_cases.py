"""What tests/test_in_flight_gpu.py (on the GPU) and tests/test_in_flight_cases.py (without one) share: the LANES -- one
recorded call each, run beside another one on a second stream or from a second host thread -- and the pure arithmetic of the
battery.  A plain module next to storage_reuse_cases.py, imported the same way; it needs numpy only.

A lane is one row of storage_reuse_cases.CALLS (all of them), or one of three HEAVY rows added here: the full-size forms of
the MSD plan that CALLS does not reach, because its M is the half-size bucket kernel, whose workgroups keep fixed buckets.
Each heavy row runs at the bound tests/msd_bucket_cases.py uses for that form, with a real count:

  full10-pairs           vrdxCmdSortKeyValue   19 000 001   ten bits, buckets of 36864: the bucket role draws its buckets by ticket
  full10-streamed-keys   vrdxCmdSort           1 << 25      ten bits, the keys-only form that streams its early buckets out
  eleven-pairs           vrdxCmdSortKeyValue   37 000 003   eleven bits

Their keys are 24 uniform bits under plan_model.PREFIX: the plan runs with its window (bits 14-23, eleven bits: 13-23) below
the prefix, and with 16.8 M values for 19 M ... 37 M keys most keys have a tie.  Values are random words, never the index:
among equal keys only they can show an order violation.  References, bit for bit: np.argsort(kind="stable") once per input.

input_set, expected_of and verdict_of answer for every lane -- the heavy rows here, the rows of CALLS through
storage_reuse_cases -- so that tests/recorded_call.py builds either kind from this module.
"""
import functools
import itertools

import numpy as np

import msd_bucket_cases
import plan_model as model
import storage_reuse_cases as cases
from storage_reuse_cases import Call, INHERITED, MSD_RUNS, NONE

KEY_BITS = 24          # the heavy rows' keys: plan_model.narrow_keys(uniform, 24)
HEAVY_REPETITIONS = 2
MOST_REPETITIONS = 16  # bounds what one pair enqueues: 2 lanes x 16 repetitions x some twenty stream-ordered operations

# the heavy rows, and the form of msd_bucket_cases.FORMS each of them is (bound, bits, capacity, recorded launches)
HEAVY = [
    Call("full10-pairs", "atomic", "vrdxCmdSortKeyValue", "key-value", 19_000_001, None, "msd", "heavy-full10", MSD_RUNS, 0),
    Call("full10-streamed-keys", "atomic", "vrdxCmdSort", "keys", 1 << 25, None, "msd", "heavy-streamed", MSD_RUNS, 0),
    Call("eleven-pairs", "atomic", "vrdxCmdSortKeyValue", "key-value", 37_000_003, None, "msd", "heavy-eleven", MSD_RUNS, 0),
]
HEAVY_FORMS = {"full10-pairs": msd_bucket_cases.FORMS["full10"], "full10-streamed-keys": msd_bucket_cases.FORMS["full10-streamed"],
               "eleven-pairs": msd_bucket_cases.FORMS["eleven"]}
HEAVY_SEEDS = {"heavy-full10": 301, "heavy-streamed": 311, "heavy-eleven": 321}
HEAVY_NAMES = [c.name for c in HEAVY]

LANES = cases.CALLS + HEAVY
NAMES = [c.name for c in LANES]
BY_NAME = {c.name: c for c in LANES}
assert len(BY_NAME) == len(LANES) and all(HEAVY_FORMS[c.name].bound == c.bound for c in HEAVY)


def is_heavy(call):
    return call.name in HEAVY_FORMS


# ---- inputs, references and verdicts of every lane ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def input_set(name):
    """(keys, values, offsets), read-only, as storage_reuse_cases.input_set: the heavy sets here, every other one there"""
    if name not in HEAVY_SEEDS:
        return cases.input_set(name)
    n = next(c.bound for c in HEAVY if c.inputs == name)
    seed = HEAVY_SEEDS[name]
    keys = model.narrow_keys(cases._words(n, seed), KEY_BITS)
    values = cases._words(n, seed + 1)
    for a in (keys, values):
        a.setflags(write=False)
    return keys, values, None


@functools.lru_cache(maxsize=None)
def _heavy_expected(name):
    call = BY_NAME[name]
    keys, values, _ = input_set(call.inputs)
    if not cases.is_key_value(call):
        return np.sort(keys), None
    order = np.argsort(keys, kind="stable")
    return keys[order], values[order]


def expected_of(call):
    """(keys, values) of the whole arrays after the call"""
    return _heavy_expected(call.name) if is_heavy(call) else cases.expected_of(call)


def heavy_constants(call):
    """(bits, bucket capacity) of a heavy row: its form's, which are the table's of plan edges at that bound"""
    form = HEAVY_FORMS[call.name]
    assert cases.msd_constants(call) == (form.bits, form.cap), (call.name, cases.msd_constants(call))
    return form.bits, form.cap


def verdict_of(call):
    """(verdict, shift | byte | None) by plan_model's rules, as storage_reuse_cases.verdict_of"""
    if not is_heavy(call):
        return cases.verdict_of(call)
    keys, _, _ = input_set(call.inputs)
    return model.msd_verdict(keys, call.bound, *heavy_constants(call))


def heavy_window(call):
    """the lowest bit of the window a heavy row is built for: the window's bits end where the keys' varying bits end"""
    return KEY_BITS - HEAVY_FORMS[call.name].bits


# ---- the battery's arithmetic --------------------------------------------------------------------------------------------

def pairs(names=None):
    """every unordered pair of lanes once, each lane with itself included, the first lane never behind the second in the list"""
    return list(itertools.combinations_with_replacement(NAMES if names is None else list(names), 2))


def partners(first):
    """the lanes at or after `first` in the list: what the test of that first lane runs it beside"""
    return NAMES[NAMES.index(first):]


def repetitions(solo_us, target_us, most=MOST_REPETITIONS):
    """How often a lane whose one repetition takes solo_us records, to last target_us: rounded up, at least 2 (so that a
    fault in one repetition must be seen although another one follows), at most `most`.  A lane that takes no measurable time
    gets the most."""
    if solo_us <= 0:
        return most
    return int(max(2, min(most, -(-target_us // solo_us))))


def pair_repetitions(a, b, solo_us):
    """(R of lane a, R of lane b) beside each other: both last about twice the longer of the two solo times (its lane then
    has the two repetitions every lane has at least); the heavy rows always take HEAVY_REPETITIONS"""
    target = 2 * max(solo_us[a], solo_us[b])
    return tuple(HEAVY_REPETITIONS if name in HEAVY_FORMS else repetitions(solo_us[name], target) for name in (a, b))


def intersect(a0, a1, b0, b1):
    """the length of the intersection of [a0, a1) and [b0, b1): 0 for intervals that only touch, that lie apart, or when one
    of them is empty"""
    return max(0, min(a1, b1) - max(a0, b0))


def msd_sorts(call):
    """[verdict, ...] of every 32-bit sort the call records with the MSD plan in front: the call itself, or the inner sorts of
    a composition.  The two-sorts form of the wide-value sorts records two inner sorts of the SAME keys -- their copy with the
    values' low words, then the caller's keys with the high words -- so both leave the call's verdict; its gather form
    records one.  A 64-bit composition records two inner sorts, of which its row tells the second one's verdict only: none of
    the lanes plans those with the MSD plan, and one that did would need the first verdict stated too."""
    if call.plan != "msd":
        return []
    assert call.sorter == "atomic", call.name   # (the ballot ranking never records the plan: MsdBits)
    assert not cases.is_wide(call), f"{call.name}: state the verdict of the first inner sort"
    assert cases.records_msd_plan(call) and call.verdict != INHERITED
    inner = 2 if cases.has_wide_values(call) and call.form == "two-sorts" else 1
    return [call.verdict] * inner


def expected_counters(lanes_and_repetitions, sorter="atomic"):
    """By how much (recorded, declined) of that sorter's vrdxHipReadPlanCounters move for [(call, repetitions), ...]: every
    sort recorded with the MSD plan in front counts as recorded, and as declined when the device turns the plan down -- it
    leaves VERDICT_NONE; all keys equal (VERDICT_MSD_SORTED) is the plan's own answer."""
    recorded = declined = 0
    for call, reps in lanes_and_repetitions:
        if call.sorter != sorter:
            continue
        verdicts = msd_sorts(call)
        recorded += reps * len(verdicts)
        declined += reps * sum(1 for v in verdicts if v == NONE)
    return recorded, declined


def expected_sticky(calls, sorter):
    """the OR of the failure words the calls of that sorter must leave"""
    word = 0
    for call in calls:
        if call.sorter == sorter and call.failure != INHERITED:
            word |= call.failure
    return word


def deal(names=None):
    """the lanes dealt round-robin to two hands (every second one each): both sorters and every family sit on both sides"""
    names = NAMES if names is None else list(names)
    return names[0::2], names[1::2]
