"""Lanes of recorded calls in flight beside each other, and the checks of what they left: what tests/test_in_flight_gpu.py
runs on two streams of a GPU and tests/test_in_flight_cases.py on host tensors, against a fake that misbehaves.  A plain
module next to recorded_call.py, imported the same way; torch and everything that touches a device come in through a RIG:

  rig.torch                      the module
  rig.stream(i)                  a context: what follows is enqueued on lane i's stream
  rig.fill(copies)               enqueues the filler on the gate stream, returns the event `gate` recorded behind it
  rig.wait(i, gate)              lane i's stream waits for the gate
  rig.mark(i)                    an event recorded on lane i's stream; rig.since(gate, event): microseconds between the two
  rig.record(w, call, d, rep)    records the call on the current stream, on world w's buffers and storage
  rig.synchronize()
  rig.sticky(kind)               reads and clears a sorter's sticky word; rig.counters(kind): its plan counters

A WORLD holds the working arrays of every lane and one storage tensor for the largest of them; the pristine inputs and the
expected outputs may be another world's, they are only read.

A lane records R times: restore the inputs, record the call, add to a device counter per check whether what the call left
differs from what it must leave -- keys, values, the guard elements behind them, the count word, the offsets (the checks of
recorded_call.array_checks, the guards split off).  Everything is a stream-ordered torch operation; nothing synchronises and
nothing crosses to the host until the caller's ONE synchronise, after which lanes_problems() reads the counters (every
repetition counts, not the last alone), the header words each lane's storage held in front of and behind it, the bytes around
the storage, the two sorters' sticky words, their plan counters and, for two lanes behind a gate, the lanes' intervals."""
import math
import time
from types import SimpleNamespace

import numpy as np

import in_flight_cases as flight
import recorded_call
from recorded_call import BAND, BAND_BYTE, BEHIND, FRONT, FRONT_BYTE, POISON
from storage_reuse_cases import GUARD_ELEMENTS
from vulkan_radix_sort_amd import api

SCRATCH_WRITTEN = "an equal field wrote the scratch arrays"
AROUND = ("wrote in front of the storage offset", "wrote behind its own storage requirement", "wrote the band behind the storage")
NOT_OWNED = api.STATUS_ENQUEUE_REFUSED | api.STATUS_COUNT_CLAMPED | api.STATUS_RANK_ORDER | api.STATUS_LOOKBACK_GAVE_UP
KINDS = ("atomic", "ballot")


# ---- worlds --------------------------------------------------------------------------------------------------------------

def new_world(torch, devices, off, device="cuda"):
    """devices: {lane name: what recorded_call.device_call returned}.  The storage: FRONT_BYTE x off | POISON x the largest
    requirement | BAND_BYTE x BAND, as tests/test_storage_reuse_gpu.py lays it out."""
    w = SimpleNamespace(torch=torch, device=devices, off=off)
    w.largest = max(d.required for d in devices.values())
    w.storage = torch.full((FRONT + w.largest + BAND,), BAND_BYTE, dtype=torch.uint8, device=device)
    w.storage[:off] = FRONT_BYTE
    w.storage[off:off + w.largest] = POISON
    return w


def second_world(torch, first, off, device="cuda"):
    """working arrays and count words of its own for every lane of `first`; the pristine inputs and the expected outputs are
    `first`'s (lanes that share an input set share the new working arrays too, as there)"""
    buffers, devices = {}, {}
    for name, d in first.device.items():
        b = d.buffers
        if id(b) not in buffers:
            buffers[id(b)] = SimpleNamespace(
                pristine=b.pristine, keys=b.pristine.keys.clone(),
                values=b.pristine.values.clone() if b.values is not None else None,
                offsets=b.pristine.offsets.clone() if b.offsets is not None else None, expected=b.expected)
        mine = SimpleNamespace(**vars(d))
        mine.buffers = buffers[id(b)]
        mine.count = d.count_pristine.clone() if d.count is not None else None
        devices[name] = mine
    return new_world(torch, devices, off, device)


# ---- one lane ------------------------------------------------------------------------------------------------------------

def lane_checks(d):
    """recorded_call.array_checks with the guard elements behind the keys and the values as checks of their own"""
    checks = []
    for message, left, wanted in recorded_call.array_checks(d):
        if left is d.buffers.keys or left is d.buffers.values:
            what = "keys" if left is d.buffers.keys else "values"
            checks.append((message, left[:-GUARD_ELEMENTS], wanted[:-GUARD_ELEMENTS]))
            checks.append((f"the guard behind the {what} changed", left[-GUARD_ELEMENTS:], wanted[-GUARD_ELEMENTS:]))
        else:
            checks.append((message, left, wanted))
    return checks


def enqueue_lane(rig, w, call, reps):
    """`reps` repetitions of the call on world w, on the current stream, nothing but stream-ordered operations.  Returns what
    lanes_problems() reads after the synchronise: the checks' names and ONE int32 tensor -- a counter per check, then the four
    header words in front of the lane and the four behind it."""
    torch = w.torch
    d = w.device[call.name]
    off, end = w.off, w.off + d.required
    checks = lane_checks(d)
    names = [message for message, _, _ in checks] + ([SCRATCH_WRITTEN] if d.scratch_from is not None else []) + list(AROUND)
    result = torch.zeros(len(names) + 8, dtype=torch.int32, device=w.storage.device)
    slot = {name: result[i:i + 1] for i, name in enumerate(names)}
    header = w.storage[off:off + 16].view(torch.int32)
    result[-8:-4].copy_(header)
    behind = w.storage[end:end + BEHIND].clone()   # (up to the end of the band for the largest call)
    for rep in range(reps):
        recorded_call.restore_inputs(d)
        scratch = w.storage[off + d.scratch_from:end].clone() if d.scratch_from is not None else None
        rig.record(w, call, d, rep)
        for message, left, wanted in checks:
            slot[message].add_(torch.ne(left, wanted).any())
        if scratch is not None:
            assert scratch.numel() > 4 * call.bound
            slot[SCRATCH_WRITTEN].add_(torch.ne(w.storage[off + d.scratch_from:end], scratch).any())
    result[-4:].copy_(header)
    slot[AROUND[0]].add_(torch.ne(w.storage[:off], FRONT_BYTE).any())
    slot[AROUND[1]].add_(torch.ne(w.storage[end:end + BEHIND], behind).any())
    slot[AROUND[2]].add_(torch.ne(w.storage[off + w.largest:], BAND_BYTE).any())
    return SimpleNamespace(call=call, d=d, reps=reps, names=names, result=result)


def lane_problems(lane):
    """what one lane left, read from its result tensor (after the synchronise)"""
    words = lane.result.cpu().numpy()
    counts, before, after = words[:-8], words[-8:-4].view(np.uint32), words[-4:].view(np.uint32)
    problems = []
    for name, count in zip(lane.names, counts.tolist()):
        if count != 0:
            problems.append(name if name in AROUND else f"{name} in {count} of {lane.reps} repetitions")
    problems += recorded_call.header_problems(lane.call, lane.d, int(after[3]), int(after[1]) & 0xFF, lambda: int(after[1]),
                                              before, after)
    return problems


# ---- lanes in flight -----------------------------------------------------------------------------------------------------

def run_lanes(rig, lanes, copies, while_in_flight=None):
    """lanes: [(world, call, repetitions)], lane i on stream i, all of them behind one gate: a filler of `copies` copies runs
    on the gate stream, every lane's stream waits for the event behind it.  Returns (problems, facts); facts.queued says whether
    the gate was still closed after the last enqueue -- if not, the lanes may have run one after the other and the caller
    runs them again behind a longer filler.  while_in_flight: called with the lanes in flight (their start and end events
    among what enqueue_lane returned) between the last enqueue and the synchronise."""
    before = {kind: rig.counters(kind) for kind in KINDS}
    for kind in KINDS:
        rig.sticky(kind)   # (clears both words)
    gate = rig.fill(copies)
    flights = []
    for i, (w, call, reps) in enumerate(lanes):
        with rig.stream(i):
            rig.wait(i, gate)
            start = rig.mark(i)
            lane = enqueue_lane(rig, w, call, reps)
            lane.start, lane.end = start, rig.mark(i)
        flights.append(lane)
    queued = not gate.query()
    if while_in_flight is not None:
        while_in_flight(flights)
    rig.synchronize()
    facts = SimpleNamespace(queued=queued, copies=copies, sticky={}, moved={},
                            intervals=[(rig.since(gate, lane.start), rig.since(gate, lane.end)) for lane in flights])
    return lanes_problems(rig, flights, before, facts.intervals, facts), facts


def calls_beside(lane, call, times, patience_s=5.0):
    """Polls (no sleep) until the lane's start event has passed -- the gate has opened and the lane's stream is running -- then
    calls `call` `times` times from this thread.  Returns [(began inside, returned inside)] per call: whether the lane had
    started and not yet ended right before the call, and whether it had still not ended right after it.  A call that did not
    begin inside the lane's interval ran beside nothing; the caller decides what that means.  patience_s only bounds the
    polling should the start event never pass."""
    deadline = time.perf_counter() + patience_s
    while not lane.start.query() and time.perf_counter() < deadline:
        pass
    stood = []
    for _ in range(times):
        began = lane.start.query() and not lane.end.query()
        call()
        stood.append((began, not lane.end.query()))
    return stood


def lanes_problems(rig, flights, counters_before, intervals=None, facts=None):
    """Every check behind the one synchronise, as a list of strings that name what went wrong (empty: all is well).  facts:
    takes the sticky words read (reading clears them) and by how much the plan counters moved, by sorter."""
    problems = []
    for i, lane in enumerate(flights):
        problems += [f"lane {i} {lane.call.name}: {p}" for p in lane_problems(lane)]
    calls = [lane.call for lane in flights]
    for kind in KINDS:
        got, want = rig.sticky(kind), flight.expected_sticky(calls, kind)
        if got != want:
            nobody = got & ~want & NOT_OWNED
            problems.append(f"sticky word of the {kind} sorter {got:#x}, not {want:#x}"
                            + (f": nobody owns {nobody:#x}" if nobody else ""))
        moved = tuple(now - then for now, then in zip(rig.counters(kind), counters_before[kind]))
        want = flight.expected_counters([(lane.call, lane.reps) for lane in flights], kind)
        if facts is not None:
            facts.sticky[kind], facts.moved[kind] = got, moved
        if moved != want:
            problems.append(f"plan counters of the {kind} sorter moved by {moved}, not {want}"
                            + (": an update was lost" if moved[0] < want[0] or moved[1] < want[1] else ""))
    if intervals is not None and len(intervals) == 2:
        (a0, a1), (b0, b1) = intervals
        if not flight.intersect(a0, a1, b0, b1) > 0:
            problems.append(f"the lanes did not intersect: {calls[0].name} ran [{a0:.0f}, {a1:.0f}) us behind the gate, "
                            f"{calls[1].name} [{b0:.0f}, {b1:.0f})")
    return problems


def intersection_share(intervals):
    """the intersection of two lanes' intervals divided by the shorter lane"""
    (a0, a1), (b0, b1) = intervals
    shorter = min(a1 - a0, b1 - b0)
    return flight.intersect(a0, a1, b0, b1) / shorter if shorter > 0 else 0.0


def run_pair(rig, lanes, filler):
    """Two lanes behind the gate; filler.copies_per_repetition x their repetitions is the filler's length, doubled (for good:
    it settles) and the pair run again, at most three times, while the gate opens before the last enqueue.  That tunes the
    harness; a failing pair is not run again."""
    problems, facts = [], None
    for attempt in range(4):
        copies = math.ceil(filler.copies_per_repetition * sum(reps for _, _, reps in lanes))
        problems, facts = run_lanes(rig, lanes, copies)
        if facts.queued or any("did not intersect" not in p for p in problems):
            break
        if attempt < 3:
            filler.copies_per_repetition *= 2
            filler.doubled += 1
    if not facts.queued:
        problems.append(f"the gate opened before the last enqueue behind a filler of {facts.copies} copies")
    return problems, facts
