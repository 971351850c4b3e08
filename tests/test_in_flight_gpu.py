"""Every kind of sort in flight beside every other kind: two streams on one sorter, two host threads on one sorter, and the
lane-order check begun while a sort runs.

INTEGRATION.md promises that "the sorter is immutable, so different streams with different storage may sort concurrently".
What IS shared between two sorts in flight is little: the sorter's two device words -- the sticky status and
the count of plans the device turned down -- which every sort of every stream updates with atomics, and its host atomics
(plans recorded, sorts recorded, the two host-side status bits).  Everything else a sort touches lies in its own storage and
in the caller's arrays.  What two sorts in flight share beyond that is the DEVICE: which workgroups are resident and when --
the bucket role of the full-size MSD plan draws its buckets by ticket, every look-back is a bounded spin, and the stability of
every fast plan rests on LDS returning atomics being served in lane order, whoever's workgroups own the other half of the CUs.

The lanes are those of tests/in_flight_cases.py: the 38 calls of tests/storage_reuse_cases.py and three heavy rows, the
full-size MSD forms at real counts with 24-bit keys (ties) and random values (only they can show an order violation).
tests/in_flight_battery.py holds the runner and its checks, tests/recorded_call.py what it shares with
tests/test_storage_reuse_gpu.py; tests/test_in_flight_cases.py runs the checks without a GPU against a fake that commits each
fault a concurrency bug would show.

  test_lane_beside_every_partner   per first lane: that lane on stream 0 and every lane at or after it in the list on stream
                                   1 -- 861 unordered pairs.  World 0 (storageOffset 0) and world 1 (48) have working arrays
                                   and a storage of their own.  Both lanes wait behind one gate, so that all work is queued
                                   before either starts; each records R times and checks every repetition on the device.
                                   A pair whose lanes' intervals (events, relative to the gate) do not intersect FAILS.
  test_two_host_threads            two threads, released by a barrier, each with a world and a stream, record every lane of
                                   their hand eight times; then the hands swapped.  A lost update on the plan counters or a
                                   stray bit in a sticky word shows here.
  test_recheck_while_a_sort_runs   vrdxHipRecheck sixteen times from the recording thread, the first of them begun while the
                                   lane is demonstrably in flight (its start event has passed, its end event has not).

R and the filler's length are harness parameters, not pass criteria: the fixture runs every lane alone (checked like any
other run) and takes its time from events; beside a partner both lanes last about twice the longer solo time, the heavy rows
take R = 2.  Every wait in the kernels is bounded by their spin limit, so cross-talk shows up as a mismatch, as
STATUS_LOOKBACK_GAVE_UP or as a wrong word, never as a hang.
"""
import statistics
import threading
import time
from types import SimpleNamespace

import pytest

import in_flight_battery as battery
import in_flight_cases as flight
import recorded_call
from guarded_call import ballot_sorter, sorter, torch_mod  # noqa: F401 (fixtures)
from test_sort_gpu import msd_capacity
from vulkan_radix_sort_amd import api

pytestmark = pytest.mark.gpu

STORAGE_OFFSETS = recorded_call.OFFSETS   # world 0 | world 1: the two layouts differ
FILLER_BYTES = 256 << 20                  # one copy of the filler moves this many bytes
FILLER_US_PER_REPETITION = 300            # where the filler's length starts: per repetition the pair enqueues
THREAD_REPETITIONS = 8
RECHECKS, RECHECK_REPETITIONS = 16, 4

RAN = {}              # (first, second) -> facts of every pair the battery has run
THREAD_ROUNDS = []
RECHECKED = []


class GpuRig:
    """in_flight_battery's rig on torch streams: two lane streams and the gate stream, no others"""

    def __init__(self, torch, sorters):
        self.torch, self.sorters = torch, sorters
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.gate_stream = torch.cuda.Stream()
        self.source = torch.zeros(FILLER_BYTES, dtype=torch.uint8, device="cuda")
        self.target = torch.empty_like(self.source)

    def stream(self, i):
        return self.torch.cuda.stream(self.streams[i])

    def fill(self, copies):
        with self.torch.cuda.stream(self.gate_stream):
            for _ in range(copies):
                self.target.copy_(self.source)
            gate = self.torch.cuda.Event(enable_timing=True)
            gate.record()
        return gate

    def wait(self, i, gate):
        self.streams[i].wait_event(gate)

    def mark(self, i):
        event = self.torch.cuda.Event(enable_timing=True)
        event.record(self.streams[i])
        return event

    def since(self, gate, event):
        return 1000.0 * gate.elapsed_time(event)

    def record(self, w, call, d, rep):
        stream = self.torch.cuda.current_stream().cuda_stream
        recorded_call.record(self.sorters[call.sorter], stream, call, d, w.storage.data_ptr(), w.off)

    def synchronize(self):
        self.torch.cuda.synchronize()

    def sticky(self, kind):
        return self.sorters[kind].read_sorter_status(self.torch.cuda.current_stream().cuda_stream)

    def counters(self, kind):
        return self.sorters[kind].read_plan_counters(self.torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def rigged(torch_mod, sorter, ballot_sorter):
    """Once: every lane's inputs and expected outputs on the device (the three heavy references are built here), the two
    worlds, the filler's unit, and every lane alone on world 0 -- checked, and timed by its events."""
    torch = torch_mod
    started = time.perf_counter()
    sorters = {"atomic": sorter, "ballot": ballot_sorter}
    shared, devices = {}, {}
    for call in flight.LANES:
        s, bits = sorters[call.sorter], None
        if flight.is_heavy(call):   # the bound records the form that is meant, keys-only and key+value (as Rig.arena)
            form = flight.HEAVY_FORMS[call.name]
            for key_value in (False, True):
                info = s.describe_plan(form.bound, key_value)
                assert (info.name, int(info.bits), int(info.launches)) == ("msd", form.bits, form.launches), (form.name, key_value)
            assert msd_capacity(form.bound, form.bits) == form.cap
            bits = form.bits
        required, chunks = recorded_call.planned(s, call, msd_bits=bits)
        devices[call.name] = recorded_call.device_call(torch, call, shared, required, chunks, source=flight)
    first = battery.new_world(torch, devices, STORAGE_OFFSETS[0])
    worlds = [first, battery.second_world(torch, first, STORAGE_OFFSETS[1])]
    assert all(w.storage.data_ptr() % 128 == 0 for w in worlds)
    rig = GpuRig(torch, sorters)
    torch.cuda.synchronize()
    built = time.perf_counter() - started

    # the filler's unit: what one copy takes
    rig.fill(4)
    torch.cuda.synchronize()
    with torch.cuda.stream(rig.gate_stream):
        begin = rig.torch.cuda.Event(enable_timing=True)
        begin.record()
    end = rig.fill(16)
    torch.cuda.synchronize()
    copy_us = 1000.0 * begin.elapsed_time(end) / 16
    filler = SimpleNamespace(copy_us=copy_us, copies_per_repetition=max(1.0, FILLER_US_PER_REPETITION / copy_us), doubled=0)
    filler.started_at = filler.copies_per_repetition

    # every lane alone: once to have its kernels loaded, once for its time; both runs checked
    solo_us, failures = {}, []
    for call in flight.LANES:
        for _ in range(2):
            problems, facts = battery.run_lanes(rig, [(worlds[0], call, 1)], max(1, round(filler.copies_per_repetition)))
            failures += [f"{call.name} alone: {p}" for p in problems]
        solo_us[call.name] = facts.intervals[0][1] - facts.intervals[0][0]
    assert not failures, f"{len(failures)} problems:\n" + "\n".join(failures)
    r = SimpleNamespace(torch=torch, rig=rig, worlds=worlds, sorters=sorters, filler=filler, solo_us=solo_us, built_s=built)
    r.fixture_s = time.perf_counter() - started
    print(f"in-flight fixture: {r.fixture_s:.1f} s ({built:.1f} s to build the lanes), storages of {first.largest} bytes, "
          f"one filler copy {copy_us:.0f} us")
    print("solo times, us: " + ", ".join(f"{name} {solo_us[name]:.0f}" for name in flight.NAMES))
    yield r
    del r.worlds, worlds, first, devices, shared


@pytest.mark.parametrize("first", flight.NAMES)
def test_lane_beside_every_partner(rigged, first):
    """`first` on stream 0 beside every lane at or after it in the list on stream 1, each pair behind one gate; every check
    of in_flight_battery.lanes_problems after the pair's one synchronise."""
    r = rigged
    failures = []
    for second in flight.partners(first):
        reps = flight.pair_repetitions(first, second, r.solo_us)
        lanes = [(r.worlds[i], flight.BY_NAME[name], reps[i]) for i, name in enumerate((first, second))]
        problems, facts = battery.run_pair(r.rig, lanes, r.filler)
        failures += [f"({first} x {reps[0]}, {second} x {reps[1]}): {p}" for p in problems]
        facts.reps = reps
        RAN[(first, second)] = facts
    assert not failures, f"{len(failures)} problems:\n" + "\n".join(failures)


def test_the_battery_ran_every_unordered_pair(rigged):
    """41 x 42 / 2 = 861 pairs, and every one of them intersected (counts what test_lane_beside_every_partner ran in this
    session: it wants the whole battery in front of it).  Prints the harness parameters the session settled on."""
    want = flight.pairs()
    assert len(want) == len(flight.NAMES) * (len(flight.NAMES) + 1) // 2 == 861
    assert set(RAN) == set(want), (len(RAN), sorted(set(want) - set(RAN))[:8])
    shares = sorted(battery.intersection_share(facts.intervals) for facts in RAN.values())
    assert shares[0] > 0, "a pair's lanes did not intersect"
    f = rigged.filler
    print(f"\nfiller: {f.copy_us:.0f} us a copy, started at {f.started_at:.2f} copies per repetition, doubled {f.doubled} "
          f"times, settled on {f.copies_per_repetition:.2f}")
    cut = statistics.quantiles(shares, n=20)
    print(f"intersection / shorter lane over {len(shares)} pairs: min {shares[0]:.3f}, 5 % {cut[0]:.3f}, 25 % {cut[4]:.3f}, "
          f"median {cut[9]:.3f}, 75 % {cut[14]:.3f}, max {shares[-1]:.3f}; {sum(s >= 0.999 for s in shares)} pairs at 1.0")
    # The intervals intersect whenever both lanes start at the gate, whatever the device does then; how long the pair took
    # says more.  alone = each lane's solo time x R: a pair the device ran one lane after the other ends after the SUM of the
    # two, one that ran them side by side at no cost to either after the LONGER of the two.
    def spread(values):
        cut = statistics.quantiles(values, n=20)
        return f"min {min(values):.2f}, 5 % {cut[0]:.2f}, median {cut[9]:.2f}, 95 % {cut[18]:.2f}, max {max(values):.2f}"
    of_sum, of_longer, stretch = [], [], []
    for pair, facts in RAN.items():
        alone = [rigged.solo_us[name] * reps for name, reps in zip(pair, facts.reps)]
        took = max(end for _, end in facts.intervals) - min(start for start, _ in facts.intervals)
        of_sum.append(took / sum(alone))
        of_longer.append(took / max(alone))
        stretch += [(end - start) / a for (start, end), a in zip(facts.intervals, alone)]
    print(f"pair's time / sum of its lanes alone:        {spread(of_sum)}")
    print(f"pair's time / the longer of its lanes alone: {spread(of_longer)}")
    print(f"a lane's time beside its partner / alone:    {spread(stretch)}")
    for pair in (("eleven-pairs", "eleven-pairs"), ("full10-pairs", "eleven-pairs"), ("msd-runs-keys", "msd-runs-keys"),
                 ("msd-runs-keys", "full10-pairs"), ("hybrid-runs", "eleven-pairs"), ("segmented", "sort64-pairs")):
        facts = RAN[pair]
        print("  " + ", ".join(f"{name} x {reps} [{start:.0f}, {end:.0f}) us, alone {rigged.solo_us[name] * reps:.0f}"
                               for name, reps, (start, end) in zip(pair, facts.reps, facts.intervals)))
    for name in flight.NAMES:
        took =[facts.reps[pair.index(name)] for pair, facts in RAN.items() if name in pair]
        print(f"  {name:32s} solo {rigged.solo_us[name]:8.0f} us   R {min(took)} ... {max(took)}")


def _hand(rig, i, world, names, barrier, flights, errors):
    try:
        with rig.stream(i):
            barrier.wait()
            for name in names:
                flights.append(battery.enqueue_lane(rig, world, flight.BY_NAME[name], THREAD_REPETITIONS))
    except BaseException as e:   # (reported by the test: a thread's exception is lost otherwise)
        errors.append(e)
        barrier.abort()


@pytest.mark.parametrize("swapped", [False, True])
def test_two_host_threads(rigged, swapped):
    """Two threads record on ONE sorter of each kind at once (api.py calls through ctypes.CDLL, which releases the GIL): each
    owns a world and a stream and records every lane of its hand THREAD_REPETITIONS times, checked per repetition on the
    device.  After the join and one synchronise: every lane's checks, the sticky words exactly the OR of what the lanes
    leave -- no STATUS_ENQUEUE_REFUSED, no STATUS_COUNT_CLAMPED -- and the plan counters moved by exactly the sum."""
    r, rig = rigged, rigged.rig
    hands = flight.deal()
    if swapped:
        hands = hands[::-1]
    before = {kind: rig.counters(kind) for kind in battery.KINDS}
    for kind in battery.KINDS:
        rig.sticky(kind)
    barrier, errors, flights = threading.Barrier(2), [], ([], [])
    threads = [threading.Thread(target=_hand, args=(rig, i, r.worlds[i], hands[i], barrier, flights[i], errors)) for i in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    rig.synchronize()
    assert not errors, errors
    assert [len(f) for f in flights] == [len(h) for h in hands]
    facts = SimpleNamespace(sticky={}, moved={})
    problems = battery.lanes_problems(rig, flights[0] + flights[1], before, None, facts)
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems)
    for kind in battery.KINDS:
        assert facts.sticky[kind] & (api.STATUS_ENQUEUE_REFUSED | api.STATUS_COUNT_CLAMPED) == 0, (kind, hex(facts.sticky[kind]))
    everything = [(flight.BY_NAME[name], THREAD_REPETITIONS) for name in flight.NAMES]
    assert facts.moved["atomic"] == flight.expected_counters(everything) and facts.moved["ballot"] == (0, 0), facts.moved
    THREAD_ROUNDS.append(swapped)


@pytest.mark.parametrize("name", ["full10-pairs", "hybrid-runs"])
def test_recheck_while_a_sort_runs(rigged, name):
    """One lane behind the gate, and while it is in flight the recording thread calls vrdxHipRecheck (not thread-safe against
    recording, so nothing else records meanwhile): every call returns, the sorter still ranks with one atomic, no
    STATUS_RANK_ORDER, the lane bit-exact in every repetition.

    So that this cannot pass with every check on an idle device, the thread polls the lane's start event and the FIRST call
    must begin after the lane has started and before it has ended (in_flight_battery.calls_beside); if the lane was over too
    soon the lane runs again behind a filler twice as long, at most three times -- that tunes the harness -- and a round in
    which no first call began inside the lane fails and says so.  The call is synchronous: it allocates a word, runs its two
    check kernels on the null stream, copies the word back and frees it.  In the runs on record the first call
    returned only when the lane was over (as freeing would if it waits for the whole device), so the calls behind it found an
    idle device: ONE call per lane begins beside the sort.  How many of the sixteen began and returned inside the lane is
    printed, not asserted (profiles/r22_sorts_in_flight.txt)."""
    r = rigged
    s = r.sorters["atomic"]
    stood = []

    def rechecks(flights):
        stood[:] = battery.calls_beside(flights[0], s.recheck, RECHECKS)

    copies = max(1, round(r.filler.copies_per_repetition * RECHECK_REPETITIONS))
    for attempt in range(4):
        problems, facts = battery.run_lanes(r.rig, [(r.worlds[0], flight.BY_NAME[name], RECHECK_REPETITIONS)], copies,
                                            while_in_flight=rechecks)
        assert len(stood) == RECHECKS   # every call returned
        assert s.describe_plan(9_000_017, True).name == "msd"
        assert facts.sticky["atomic"] & api.STATUS_RANK_ORDER == 0, hex(facts.sticky["atomic"])
        assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems)
        if facts.queued and stood[0][0]:
            break
        copies *= 2
    began, returned = sum(b for b, _ in stood), sum(e for _, e in stood)
    print(f"\nrecheck beside {name}: lane [{facts.intervals[0][0]:.0f}, {facts.intervals[0][1]:.0f}) us behind the gate, filler "
          f"of {facts.copies} copies, attempt {attempt + 1}: {began} of {RECHECKS} calls began inside the lane, {returned} returned "
          f"inside it")
    assert facts.queued, f"the gate opened before the last enqueue behind a filler of {facts.copies} copies"
    assert stood[0][0], f"no call of vrdxHipRecheck began while {name} was in flight: the lane was over before the first one"
    RECHECKED.append(name)


def test_both_thread_rounds_and_both_recheck_lanes_ran():
    assert THREAD_ROUNDS == [False, True] and RECHECKED == ["full10-pairs", "hybrid-runs"]
