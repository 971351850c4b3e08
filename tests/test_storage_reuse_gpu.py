"""Every kind of sort on the storage every other kind of sort left behind.

INTEGRATION.md promises that the storage "may hold anything on entry", and the callers this library is built for lean on
it: one storage per shard (batched.py), twenty arrays through one (bench.py), two inner sorts on one header (the 64-bit
sorts).  Nothing clears the state between two sorts in one step; the table below says, region by region, who zeroes or
fully overwrites it before its first reader, and which pair of calls or which fill word of this file would show a clear
that went missing.  The calls are CALLS of tests/storage_reuse_cases.py (one per entry point and per path through it; the
verdicts they must leave are checked against tests/plan_model.py without a GPU by tests/test_storage_reuse_cases.py).

  region of the storage (vrdx_layout.h)     zeroed or fully written before its first reader by          exposed here by
  ----------------------------------------  ----------------------------------------------------------  ---------------------------------------------
  word 0, the count                         the fill (hipMemsetAsync of clearBytes); indirect: the      no kernel reads it (they read the caller's
                                            copy of the caller's count; segmented_clear_kernel          word); the `empty` call pins that it stays
  word 1, the plan's verdict                the fill; segmented_clear_kernel; small_sort_kernel         (msd-runs-keys | hybrid-runs, one-workgroup |
                                            (words 1-3 of the header)                                    sort64-small): the stale verdict; fill 0x00000001
  word 2, the MSD plan's word               the same three                                               (msd-declined-keys, msd-runs-keys): a stale
                                                                                                         "turned down" makes the plan return; fill 0xFFFFFFFF
  word 3, the failure word                  the same three                                               (segmented-invalid, every call but `empty`)
  global histogram [4][256]                 the fill (its kernel adds with atomics)                      every pair of general sorts, e.g. (hybrid-runs,
                                                                                                         hybrid-declined): doubled counts; fill 0x00000001
  MSD bucketCount[2^bits]                   the fill (clearBytes reaches behind it under the MSD plan)   (msd-runs-keys, msd-runs-pairs): doubled buckets
                                                                                                         exceed the capacity, verdict NONE; fill 0x00000001
  MSD bucketBase[2^bits]                    spine_msd_kernel writes every bucket's base                  (msd-declined-keys, msd-runs-keys); random fill
  MSD per-tile counts uint16[tiles][2^bits] histogram_msd_kernel writes every tile's row, also of tiles  (msd-runs-keys, msd-indirect-small): 20001 keys
                                            behind an indirect count                                     under rows a sort of M left; fill 0xFFFFFFFF
  status region 0 (tile rows + block rows)  histogram_kernel; under the MSD plan spine_msd_kernel        (tail-split, msd-declined-keys): the rows lie in
                                                                                                         what was key scratch; (block-sums, block-sums);
                                                                                                         fills 0x40000001, 0x80000001, 0x04000001
  status region 1                           every pass zeroes its own row (and block row) of the other   (msd-runs-pairs, msd-declined-pairs-skips): two
                                            region -- also a pass that moves nothing and a tile behind   passes move nothing; (msd-runs-keys,
                                            an indirect count                                            msd-indirect-declined); the same fills
  tickets[2]                                histogram_kernel / histogram_msd_kernel zero both; every     (msd-runs-pairs, hybrid-declined): the ticket line
                                            pass zeroes the next pass's                                  of H lies in the leaver's per-tile counts; fill
                                                                                                         0x00000001 (tile 0 would be skipped)
  key and value scratch                     every pass writes all n elements before the next reads them  (tail-split, msd-runs-pairs); random fill
  segmented: the two list counters          segmented_clear_kernel                                       (msd-runs-keys | hybrid-runs, segmented |
                                                                                                         segmented64): they lie in the global histogram
  segmented: mid and large list             segmented_small_kernel writes slot [0, count) before the     (segmented-invalid, segmented): other ids in the
                                            mid and the large kernel read them                           same slots; random fill
  segmented: key and value scratch          a large segment's pass writes its range before the next one  (msd-runs-pairs, segmented | segmented64)
  64-bit: A, B | I, T behind the inner      split64 / gather_hi64 / permute64 write [0, n) of each       (sort64-pairs, sort64-indirect): half the count
  storage                                   before the inner sorts, merge64 and copy_back64 read it      over the leaver's arrays; (msd-runs-pairs,
                                                                                                         sort64-pairs): they lie in 32-bit key scratch
  words 1-3 behind the newer one-workgroup  small_sort_bits_kernel, small_sort_ordered_kernel and       (msd-runs-keys | hybrid-runs | segmented-invalid,
  sorts                                     small_sort_wide_kernel, each on its own (as                  bits-one-workgroup | ordered-small |
                                            small_sort_kernel does)                                      wide-one-workgroup): stale verdict, stale
                                                                                                         "turned down", stale failure word; fills
                                                                                                         0x00000001 and 0xFFFFFFFF
  range sort: word 2, the mask of active    the range sort's fill zeroes it with the header;             (msd-declined-keys, range-chunked-keys): a "turned
  passes (the MSD plan's word elsewhere)    range_scan_kernel's first launch stores it before any        down" read as passes; (range-chunked-pairs-copy-
                                            other launch reads it                                        back, msd-runs-keys): a mask read as "turned
                                                                                                         down", verdict NONE; (range-chunked-pairs-copy-
                                                                                                         back, range-equal-field); fill 0xFFFFFFFF
  range sort: totals[4][256]                the range sort's fill (the first count launch adds with      (hybrid-runs | segmented, range-chunked-keys): the
                                            atomics)                                                     global histogram and the two list counters lie
                                                                                                         there; (range-chunked-pairs-copy-back, range-gap-
                                                                                                         in-mask): a constant digit becomes a pass; and
                                                                                                         back: (range-chunked-keys, hybrid-declined |
                                                                                                         segmented); fill 0x00000001
  range sort: counts[chunks][256]           range_count_kernel STORES the row of every chunk that        (msd-runs-keys, range-chunked-keys): bucketCount
                                            holds keys; range_scan_kernel and the scatter read those     and bucketBase lie there; (range-chunked-pairs-
                                            rows only (rows behind an indirect count keep what they      copy-back, range-indirect-small): two rows under
                                            held)                                                        eight of a longer sort; back: (range-chunked-keys,
                                                                                                         msd-runs-pairs): doubled buckets; random fill
  range sort: key and value scratch         every active pass's scatter writes all n elements before     (msd-runs-pairs, range-chunked-pairs-copy-back);
                                            the next pass or the copy back reads them; no active pass:   (range-chunked-keys, range-equal-field): the
                                            not a byte                                                   scratch stays byte for byte the leaver's; random
                                                                                                         fill
  wide values: A, B, C | A, T behind the    iota_wide_kernel writes A[0, n), gather_wide_kernel T[0, n)  (wide-gather, wide-two-sorts-indirect) and back: T
  inner storage                             before copy_back_wide_kernel reads it; split_wide_kernel     lies over B and C; (sort64-pairs, wide-gather),
                                            writes A, B, C [0, n) before the inner sorts and             (wide-gather, sort64-ordered-pairs): the 64-bit
                                            merge_wide_kernel read them                                  sorts' A, B | I, T lie in the same bytes;
                                                                                                         (msd-runs-pairs, wide-gather): 32-bit scratch
  wide values, segmented: counters, lists   segmented_clear_kernel; segmented_small_wide_kernel writes   (wide-gather | hybrid-runs, wide-segmented): the
  and scratch                               slot [0, count) before the mid and the large kernel read     counters lie in the global histogram; (segmented-
                                            them; a large segment's pass writes its range of the         invalid, wide-segmented): other ids in the slots;
                                            scratch (over A and T) before the next one reads it          (wide-two-sorts-indirect, wide-segmented)
  by a bit range, in a key order            no region of their own: the segmented forms use the          (segmented, segmented-bits | ordered-segmented),
                                            segmented regions above, the 64-bit ones those of the        (segmented64, segmented64-ordered), (sort64-pairs,
                                            64-bit sorts; order32_kernel works on the caller's keys,     sort64-ordered-pairs), (msd-declined-keys,
                                            in place, around the plan's own steps                        ordered-msd) and each of them back

No region is left without a pair.  The one-workgroup path is the one that touched too little: small_sort_kernel cleared the
failure word alone, so a sort of up to 16384 elements behind an MSD or hybrid sort reported that sort's verdict
(vrdxHipReadPlanVerdict, Sorter.plan_taken()); the kernel now zeroes words 1-3.  The families added since -- by a bit range,
in a key order, with 8-byte values, range sorts at every size -- joined the matrix later, every writer above named from the
recorder and the kernels; the battery found nothing in them.

Every wait in the kernels is bounded by their spin limit, so a clear that went missing shows up as STATUS_LOOKBACK_GAVE_UP or
as a mismatch, never as a hang.  Only booleans and header words cross to the host per run: the inputs and the expected
outputs are made once and kept on the device.
"""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import storage_reuse_cases as cases
from guarded_call import ballot_sorter, sorter, to_device, torch_mod  # noqa: F401 (fixtures)
from storage_reuse_cases import CALLS, INHERITED, NAMES
from test_plan_choice_gpu import expected_word, plan_storage_word
from test_range_sort_gpu import scratch_from
from vulkan_radix_sort_amd import api

pytestmark = pytest.mark.gpu

OFFSETS = (0, 48)     # storageOffset: the layout moves with the low seven bits of the storage's address
FRONT = max(OFFSETS)
BAND = 256            # 0x5A behind the largest requirement
BEHIND = 4096         # bytes right behind a call's own requirement that it must leave alone
POISON, FRONT_BYTE, BAND_BYTE = 0xA5, 0x3C, 0x5A
FILLS = [("zero", 0x00000000), ("ones", 0xFFFFFFFF), ("one", 0x00000001), ("aggregate-1", 0x40000001),
         ("inclusive-1", 0x80000001), ("block-arrival-1", 0x04000001), ("random", None)]

RAN = set()           # (leaver, follower, storage_off) of every pair the matrix has run


@pytest.fixture(scope="module")
def world(torch_mod, sorter, ballot_sorter):
    """Once: every call's inputs and expected outputs, on the device (calls that share an input set share its pristine copy
    and its working buffers), the requirement of every call and ONE storage tensor for the largest of them."""
    torch = torch_mod
    started = time.perf_counter()
    w = SimpleNamespace(torch=torch, sorters={"atomic": sorter, "ballot": ballot_sorter}, device={})
    shared = {}
    for call in CALLS:
        s = w.sorters[call.sorter]
        key_value, wide = cases.is_key_value(call), cases.is_wide(call)
        # what the host records is what the table of CALLS assumes
        if call.plan is not None:
            info = s.describe_plan(call.bound, True if wide else key_value)
            assert info.name == call.plan, (call.name, info.name)
            assert call.plan != "msd" or int(info.bits) == cases.MSD_BITS, (call.name, int(info.bits))
            assert call.plan != "msd" or int(info.bits) == cases.msd_constants(call)[0], (call.name, int(info.bits))
        chunks = _family_plan(s, call, key_value)
        if call.inputs not in shared:
            keys, values, offsets = cases.input_set(call.inputs)
            pristine = SimpleNamespace(keys=to_device(torch, cases.padded(keys)),
                                       values=to_device(torch, cases.padded(values)) if values is not None else None,
                                       offsets=to_device(torch, offsets) if offsets is not None else None)
            shared[call.inputs] = SimpleNamespace(
                pristine=pristine, keys=pristine.keys.clone(),
                values=pristine.values.clone() if values is not None else None,
                offsets=pristine.offsets.clone() if offsets is not None else None, expected={})
        d = shared[call.inputs]
        which = (key_value, cases.sorted_count(call), call.bits, call.order, cases.is_segmented(call))
        if which not in d.expected:
            want_keys, want_values = cases.expected_of(call)
            d.expected[which] = (to_device(torch, cases.padded(want_keys)),
                                 to_device(torch, cases.padded(want_values)) if key_value else None)
        required = {"keys": lambda: s.storage_requirements(call.bound),
                    "key-value": lambda: s.key_value_storage_requirements(call.bound),
                    "keys64": lambda: s.storage_requirements64(call.bound, False),
                    "key-value64": lambda: s.storage_requirements64(call.bound, True),
                    "wide-value": lambda: s.wide_value_storage_requirements(call.bound)}[call.requirement]().size
        # (the wide-value requirement is the inner one plus 12 bytes per element plus 112 + 2 x 124: a multiple of 4 only)
        assert required % (4 if call.requirement == "wide-value" else 16) == 0
        verdict, shift = cases.verdict_of(call) if call.verdict != INHERITED else (INHERITED, None)
        assert verdict == call.verdict, (call.name, verdict)
        count = None
        if call.count is not None:
            count = to_device(torch, np.array([call.count, 0, 0, 0], np.uint32))
        w.device[call.name] = SimpleNamespace(
            buffers=d, key_value=key_value, expected_keys=d.expected[which][0], expected_values=d.expected[which][1],
            required=required, count=count, count_pristine=count.clone() if count is not None else None,
            bits=call.bits if call.bits is not None else (None, None), order=cases.order_word(call),
            scratch_from=scratch_from(chunks) if call.name == "range-equal-field" else None,
            plan_word=expected_word(verdict, shift) if cases.records_msd_plan(call) else None)
    w.largest = max(d.required for d in w.device.values())
    w.storage = torch.empty(FRONT + w.largest + BAND, dtype=torch.uint8, device="cuda")
    assert w.storage.data_ptr() % 128 == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(20261018)
    w.random_words = torch.randint(-(1 << 31), 1 << 31, (w.largest // 4,), generator=g, device="cuda",
                                   dtype=torch.int64).to(torch.int32)
    torch.cuda.synchronize()
    print(f"storage-reuse fixture: {time.perf_counter() - started:.1f} s, storage of {w.largest} bytes")
    yield w
    del w.storage, w.device, shared


def _family_plan(s, call, key_value):
    """The plan of a call of the newer families against the family's own describe call, before anything runs; returns the
    chunks of a chunked range sort (else None)."""
    if cases.is_segmented(call):
        return None
    if cases.is_range_sort(call):
        info = s.describe_range_sort_plan(call.bound, key_value, *call.bits)
        cus = int(s.describe_range_sort_plan(0x3FFFFFFC, False, 0, 8).chunks)   # (the device's CU count)
        assert (info.name, int(info.digits)) == (call.form, -(-(call.bits[1] - call.bits[0]) // 8)), (call.name, info.name)
        assert int(info.chunks) == min(cus, call.bound // 8192), (call.name, int(info.chunks))
        assert cus >= cases.RANGE_FACTS[call.name].most_chunks, cus   # (every chunk RANGE_FACTS counts on holds keys here)
        return int(info.chunks)
    if call.bits is not None:
        info = s.describe_sort_bits_plan(call.bound, key_value, *call.bits)
        assert info.name == call.form and int(info.launches) == 1, (call.name, info.name)
    elif cases.is_ordered32(call):
        info = s.describe_ordered_sort_plan(call.bound, key_value, cases.order_word(call))
        assert info.name == call.plan, (call.name, info.name)
        assert call.plan != "msd" or int(info.bits) == cases.msd_constants(call)[0], (call.name, int(info.bits))
    elif cases.has_wide_values(call):
        info = s.describe_wide_value_sort_plan(call.bound)
        assert info.name == call.form, (call.name, info.name)
        assert (int(info.oneWorkgroupMax), int(info.twoSortsFrom)) == (cases.WIDE_ONE_WORKGROUP_N, cases.WIDE_TWO_SORTS_N)
        assert call.form == "one-workgroup" or api.PLAN_NAMES[int(info.innerPlan)] == call.plan, (call.name, int(info.innerPlan))
    return None


def _prepare_storage(w, off, word=None, random=False):
    """[0, off) front bytes | [off, off + largest) the storage: 0xA5 bytes, or `word` in every uint32, or the seeded random
    words | the band (and whatever lies behind it)"""
    torch = w.torch
    w.storage[:off] = FRONT_BYTE
    region = w.storage[off:off + w.largest]
    if random:
        region.view(torch.int32).copy_(w.random_words)
    elif word is not None:
        region.view(torch.int32).fill_(word - (1 << 32) if word >= 1 << 31 else word)
    else:
        region.fill_(POISON)
    w.storage[off + w.largest:] = BAND_BYTE


ROWS = {row.c_name: row for row in api.RECORDING_CALLS + api.ORDERED_SORT_CALLS + api.WIDE_VALUE_CALLS
        + api.WIDE_VALUE_SEGMENTED_CALLS + api.RANGE_SORT_CALLS}


def _record(s, stream, call, d, storage, off):
    """the row of RECORDING_CALLS, ORDERED_SORT_CALLS, WIDE_VALUE_CALLS, WIDE_VALUE_SEGMENTED_CALLS or RANGE_SORT_CALLS that
    `call.entry` names, on the world's buffers at byte offset 0"""
    b = d.buffers
    row = ROWS[call.entry]
    given = {"command_buffer": stream, "element_count": call.bound, "max_element_count": call.bound,
             "segment_count": len(b.offsets) - 1 if b.offsets is not None else None, "offsets": b.offsets, "indirect": d.count,
             "keys": b.keys, "values": b.values if d.key_value else None, "begin_bit": d.bits[0], "end_bit": d.bits[1],
             "order": d.order}
    given = {name: t.data_ptr() if hasattr(t, "data_ptr") else t for name, t in given.items()}
    given.update(storage=storage, storage_offset=off, offsets_offset=0, indirect_offset=0, keys_offset=0, values_offset=0)
    getattr(s, row.method)(*(given[name] for name, _ in row.parameters[:-2]))   # (no query pool)


def run(w, call, off):
    """One call on the storage as it is: fresh copies of the inputs, the call, and every check of the module's docstring.
    Returns (problems, failure word the call must leave): the problems as a list of short strings, empty when all is well."""
    torch = w.torch
    s, d = w.sorters[call.sorter], w.device[call.name]
    b = d.buffers
    stream = torch.cuda.current_stream().cuda_stream
    b.keys.copy_(b.pristine.keys)
    if b.values is not None:
        b.values.copy_(b.pristine.values)
    end = off + d.required
    header = w.storage[off:off + 16].clone()
    behind = w.storage[end:end + BEHIND].clone()   # (up to the end of the band for the largest call)
    scratch = w.storage[off + d.scratch_from:end].clone() if d.scratch_from is not None else None
    _record(s, stream, call, d, w.storage.data_ptr(), off)
    torch.cuda.synchronize()
    problems = []
    # 0. a range sort over a field that is the same in every key writes neither of its scratch arrays
    if scratch is not None:
        assert scratch.numel() > 4 * call.bound
        if not torch.equal(w.storage[off + d.scratch_from:end], scratch):
            problems.append("an equal field wrote the scratch arrays")
    # 1. keys and values bit for bit, the elements from the count on and the guard behind the arrays included
    if not torch.equal(b.keys, d.expected_keys):
        problems.append("keys differ")
    if d.key_value and not torch.equal(b.values, d.expected_values):
        problems.append("values differ")
    if b.values is not None and not d.key_value and not torch.equal(b.values, b.pristine.values):
        problems.append("a keys-only call wrote the values")
    if d.count is not None and not torch.equal(d.count, d.count_pristine):
        problems.append("the count word changed")
    if b.offsets is not None and not torch.equal(b.offsets, b.pristine.offsets):
        problems.append("the offsets changed")
    # 2. and 3. the failure word, the verdict, and word 1 as a whole where the MSD plan is recorded
    want_status, want_verdict = call.failure, call.verdict
    if call.verdict == INHERITED:   # an empty sort records nothing: the header is the call before's
        words = header.cpu().numpy().view(np.uint32)
        want_status, want_verdict = int(words[3]), int(words[1]) & 0xFF
        if not torch.equal(w.storage[off:off + 16], header):
            problems.append("an empty sort wrote the header")
    status = s.read_status(stream, w.storage.data_ptr(), off)
    if status != want_status:
        problems.append(f"failure word {status:#x}, not {want_status:#x}")
    verdict = s.read_plan_verdict(stream, w.storage.data_ptr(), off)
    if verdict != want_verdict:
        problems.append(f"verdict {verdict}, not {want_verdict}")
    if d.plan_word is not None:
        word = plan_storage_word(w.storage[off:])
        if word != d.plan_word:
            problems.append(f"plan word {word:#x}, not {d.plan_word:#x}")
    # 4. nothing outside the call's own requirement
    if not bool((w.storage[off + w.largest:] == BAND_BYTE).all()):
        problems.append("wrote the band behind the storage")
    if not bool((w.storage[:off] == FRONT_BYTE).all()):
        problems.append("wrote in front of the storage offset")
    if not torch.equal(w.storage[end:end + BEHIND], behind):
        problems.append("wrote behind its own storage requirement")
    return problems, (0 if call.failure == INHERITED else call.failure)


def _sticky_problems(w, left):
    """5. every sorter's sticky word is the OR of the failure words its runs must leave (reading clears it)"""
    stream = w.torch.cuda.current_stream().cuda_stream
    problems = []
    for kind, s in w.sorters.items():
        want = 0
        for call, failure in left:
            if call.sorter == kind:
                want |= failure
        got = s.read_sorter_status(stream)
        if got != want:
            problems.append(f"sticky word of the {kind} sorter {got:#x}, not {want:#x}")
    return problems


@pytest.mark.parametrize("storage_off", OFFSETS)
@pytest.mark.parametrize("leaver", NAMES)
def test_follower_after_leaver(world, leaver, storage_off):
    """For every follower: the leaver, then the follower on the storage the leaver left, nothing reinitialised in between --
    nor between one follower and the next leaver.  Both runs are checked."""
    w = world
    _prepare_storage(w, storage_off)
    _sticky_problems(w, [])   # (clears both words)
    first = cases.BY_NAME[leaver]
    failures = []
    for follower in CALLS:
        where = f"({leaver}, {follower.name}, {storage_off})"
        left = []
        for role, call in (("leaver", first), ("follower", follower)):
            problems, failure = run(w, call, storage_off)
            left.append((call, failure))
            failures += [f"{where} {role} {call.name}: {p}" for p in problems]
        failures += [f"{where}: {p}" for p in _sticky_problems(w, left)]
        RAN.add((leaver, follower.name, storage_off))
    assert not failures, f"{len(failures)} problems:\n" + "\n".join(failures)


@pytest.mark.parametrize("fill", [name for name, _ in FILLS])
@pytest.mark.parametrize("name", NAMES)
def test_call_on_prefilled_storage(world, name, fill):
    """One call on storage filled with a word a missed clear would take for real: a ticket or a count of one, AGGREGATE and
    INCLUSIVE with the value 1, one arrival in a block-sum word, zeros, all ones, seeded random words."""
    w = world
    word = dict(FILLS)[fill]
    _prepare_storage(w, 0, word=word, random=word is None)
    _sticky_problems(w, [])
    call = cases.BY_NAME[name]
    problems, failure = run(w, call, 0)
    problems += _sticky_problems(w, [(call, failure)])
    assert not problems, f"({name}, fill {fill}): " + "; ".join(problems)


def test_the_matrix_ran_every_ordered_pair():
    """len(CALLS)^2 ordered pairs at both storage offsets (counts what test_follower_after_leaver ran in this session: it
    wants the whole matrix in front of it)"""
    assert len(RAN) == len(OFFSETS) * len(CALLS) ** 2, len(RAN)
    assert RAN == {(a, b, off) for a in NAMES for b in NAMES for off in OFFSETS}
