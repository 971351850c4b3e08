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
outputs are made once and kept on the device.  What one call needs -- its plan, its device buffers, the recording, the
checks of its arrays and header words -- is tests/recorded_call.py, which tests/test_in_flight_gpu.py runs two at a time.
"""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import recorded_call
import storage_reuse_cases as cases
from guarded_call import ballot_sorter, sorter, torch_mod  # noqa: F401 (fixtures)
from recorded_call import BAND, BAND_BYTE, BEHIND, FRONT, FRONT_BYTE, OFFSETS, POISON
from storage_reuse_cases import CALLS, INHERITED, NAMES
from test_plan_choice_gpu import plan_storage_word

pytestmark = pytest.mark.gpu

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
        # what the host records is what the table of CALLS assumes
        required, chunks = recorded_call.planned(w.sorters[call.sorter], call)
        w.device[call.name] = recorded_call.device_call(torch, call, shared, required, chunks)
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


def run(w, call, off):
    """One call on the storage as it is: fresh copies of the inputs, the call, and every check of the module's docstring.
    Returns (problems, failure word the call must leave): the problems as a list of short strings, empty when all is well."""
    torch = w.torch
    s, d = w.sorters[call.sorter], w.device[call.name]
    stream = torch.cuda.current_stream().cuda_stream
    recorded_call.restore_inputs(d)
    end = off + d.required
    header = w.storage[off:off + 16].clone()
    behind = w.storage[end:end + BEHIND].clone()   # (up to the end of the band for the largest call)
    scratch = w.storage[off + d.scratch_from:end].clone() if d.scratch_from is not None else None
    recorded_call.record(s, stream, call, d, w.storage.data_ptr(), off)
    torch.cuda.synchronize()
    problems = []
    # 0. a range sort over a field that is the same in every key writes neither of its scratch arrays
    if scratch is not None:
        assert scratch.numel() > 4 * call.bound
        if not torch.equal(w.storage[off + d.scratch_from:end], scratch):
            problems.append("an equal field wrote the scratch arrays")
    # 1. keys and values bit for bit, the elements from the count on and the guard behind the arrays included
    problems += [message for message, left, wanted in recorded_call.array_checks(d) if not torch.equal(left, wanted)]
    # 2. and 3. the failure word, the verdict, and word 1 as a whole where the MSD plan is recorded
    before = after = None
    if call.verdict == INHERITED:   # an empty sort records nothing: the header is the call before's
        before = header.cpu().numpy().view(np.uint32)
        after = w.storage[off:off + 16].cpu().numpy().view(np.uint32)
    problems += recorded_call.header_problems(
        call, d, s.read_status(stream, w.storage.data_ptr(), off), s.read_plan_verdict(stream, w.storage.data_ptr(), off),
        lambda: plan_storage_word(w.storage[off:]), before, after)
    # 4. nothing outside the call's own requirement
    if not bool((w.storage[off + w.largest:] == BAND_BYTE).all()):
        problems.append("wrote the band behind the storage")
    if not bool((w.storage[:off] == FRONT_BYTE).all()):
        problems.append("wrote in front of the storage offset")
    if not torch.equal(w.storage[end:end + BEHIND], behind):
        problems.append("wrote behind its own storage requirement")
    return problems, recorded_call.failure_left(call)


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
