"""tests/in_flight_cases.py and the checks of tests/in_flight_battery.py without a GPU.

The lanes: the pair list holds every unordered pair once; the battery's arithmetic at its edges; what the plan counters must
move by, lane by lane, against a table written down here (the verdicts behind it by tests/plan_model.py); the heavy inputs
against the model (the plan takes each with the window it is built for) and their ties.

The battery: run_lanes / run_pair on host tensors with a rig whose `record` is a fake that writes what the call must leave --
and can be told to misbehave in each way a concurrency bug would show.  Every planted fault must fail with a message that
names it; the correct fake passes."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import in_flight_battery as battery
import in_flight_cases as flight
import plan_model as model
import recorded_call
import storage_reuse_cases as cases
from storage_reuse_cases import Call, INHERITED, NONE
from vulkan_radix_sort_amd import api


# ---- the lanes -----------------------------------------------------------------------------------------------------------

def test_the_pair_list_holds_every_unordered_pair_once():
    pairs = flight.pairs()
    n = len(flight.NAMES)
    assert n == 41 and len(pairs) == n * (n + 1) // 2 == 861 and len(set(pairs)) == len(pairs)
    assert {frozenset(p) for p in pairs} == {frozenset((a, b)) for a in flight.NAMES for b in flight.NAMES}
    assert len({frozenset(p) for p in pairs}) == len(pairs)
    assert all(flight.NAMES.index(a) <= flight.NAMES.index(b) for a, b in pairs)
    assert sum(a == b for a, b in pairs) == n
    # what the GPU test of one first lane runs is that lane's share of the list
    assert [(a, b) for a in flight.NAMES for b in flight.partners(a)] == pairs
    assert flight.NAMES[:len(cases.CALLS)] == cases.NAMES and flight.NAMES[len(cases.CALLS):] == flight.HEAVY_NAMES


def test_repetitions_at_their_edges():
    r = flight.repetitions
    assert r(100, 200) == 2 and r(100, 201) == 3 and r(100, 100) == 2 and r(100, 1) == 2   # never fewer than 2
    assert r(10, 159) == 16 and r(10, 160) == 16 and r(10, 161) == 16 and r(10, 10 ** 9) == flight.MOST_REPETITIONS
    assert r(0, 500) == flight.MOST_REPETITIONS and r(-1.0, 500) == flight.MOST_REPETITIONS   # a lane too short to time
    assert r(33.3, 100.0) == 4 and isinstance(r(33.3, 100.0), int)
    solo = {"one-workgroup": 50.0, "msd-runs-keys": 400.0, "eleven-pairs": 3000.0, "full10-pairs": 1500.0}
    assert flight.pair_repetitions("msd-runs-keys", "msd-runs-keys", solo) == (2, 2)
    assert flight.pair_repetitions("one-workgroup", "msd-runs-keys", solo) == (16, 2)
    assert flight.pair_repetitions("msd-runs-keys", "eleven-pairs", solo) == (15, 2)
    assert flight.pair_repetitions("full10-pairs", "eleven-pairs", solo) == (2, 2)     # the heavy rows take 2, whatever
    assert flight.pair_repetitions("one-workgroup", "one-workgroup", solo) == (2, 2)


def test_intersect_at_its_edges():
    i = flight.intersect
    assert i(0, 10, 10, 20) == 0 and i(10, 20, 0, 10) == 0          # touching intervals do not intersect
    assert i(0, 10, 11, 20) == 0 and i(0, 10, 9, 20) == 1 and i(9, 20, 0, 10) == 1
    assert i(0, 100, 40, 50) == 10 and i(40, 50, 0, 100) == 10      # one inside the other
    assert i(5, 5, 0, 10) == 0 and i(0, 10, 5, 5) == 0 and i(5, 5, 5, 5) == 0   # a lane of no length
    assert i(0.0, 2.5, 1.5, 9.0) == 1.0
    assert battery.intersection_share([(0, 10), (5, 50)]) == 0.5 and battery.intersection_share([(0, 0), (0, 5)]) == 0.0


# by how much (recorded, declined) move for ONE repetition; every lane that is not named: (0, 0)
COUNTERS = {"msd-runs-keys": (1, 0), "msd-runs-pairs": (1, 0), "msd-declined-keys": (1, 1), "msd-declined-pairs-skips": (1, 1),
            "msd-all-equal": (1, 0), "msd-indirect-small": (1, 0), "msd-indirect-declined": (1, 1), "tail-split": (1, 1),
            "block-sums": (1, 1), "ordered-msd": (1, 0), "wide-two-sorts-indirect": (2, 0), "full10-pairs": (1, 0),
            "full10-streamed-keys": (1, 0), "eleven-pairs": (1, 0)}


@pytest.mark.parametrize("name", flight.NAMES)
def test_expected_counters_lane_by_lane(name):
    """The table above is the independent statement: expected_counters must give its row.  The second half only ties the
    table to the lane's keys: plan_model's verdict on them is the verdict the row states, and turned down means VERDICT_NONE;
    how many sorts a row records is restated from the same rule as in_flight_cases.msd_sorts, so it adds nothing there."""
    call = flight.BY_NAME[name]
    assert flight.expected_counters([(call, 1)]) == COUNTERS.get(name, (0, 0))
    assert flight.expected_counters([(call, 7)]) == tuple(7 * c for c in COUNTERS.get(name, (0, 0)))
    assert flight.expected_counters([(call, 3)], "ballot") == (0, 0)
    recorded = 0
    if call.plan == "msd" and not cases.is_wide(call):
        recorded = 2 if (cases.has_wide_values(call) and call.form == "two-sorts") else 1
    verdict = flight.verdict_of(call)[0] if call.verdict != INHERITED else INHERITED
    assert verdict == call.verdict
    declined = recorded if verdict == model.VERDICT_NONE else 0
    assert flight.expected_counters([(call, 1)]) == (recorded, declined)


def test_expected_counters_and_sticky_words_add_up():
    lanes = [(flight.BY_NAME[name], reps) for name, reps in (("msd-declined-keys", 3), ("wide-two-sorts-indirect", 2),
                                                             ("ballot-hybrid", 5), ("eleven-pairs", 2), ("empty", 9))]
    assert flight.expected_counters(lanes) == (3 + 4 + 2, 3) and flight.expected_counters(lanes, "ballot") == (0, 0)
    everything = [(call, 8) for call in flight.LANES]
    assert flight.expected_counters(everything) == tuple(8 * sum(c[i] for c in COUNTERS.values()) for i in (0, 1))
    calls = [flight.BY_NAME[name] for name in ("segmented-invalid", "hybrid-runs", "empty", "ballot-hybrid")]
    assert flight.expected_sticky(calls, "atomic") == api.STATUS_SEGMENTS_INVALID and flight.expected_sticky(calls, "ballot") == 0
    assert flight.expected_sticky(calls[1:], "atomic") == 0


def test_the_hands_hold_both_sorters_and_every_family():
    hands = flight.deal()
    assert sorted(hands[0] + hands[1]) == sorted(flight.NAMES) and abs(len(hands[0]) - len(hands[1])) <= 1
    families = (cases.is_segmented, cases.is_wide, cases.is_range_sort, cases.is_ordered32, cases.has_wide_values,
                flight.is_heavy, lambda c: c.sorter == "ballot", lambda c: c.sorter == "atomic", lambda c: c.plan == "msd",
                lambda c: c.plan == "hybrid-8", lambda c: c.count is not None, lambda c: c.bits is not None)
    for hand in hands:
        for family in families:
            assert any(family(flight.BY_NAME[name]) for name in hand), family


@pytest.mark.parametrize("name", flight.HEAVY_NAMES)
def test_the_plan_takes_the_heavy_inputs_and_they_hold_ties(name):
    call = flight.BY_NAME[name]
    form = flight.HEAVY_FORMS[name]
    keys, values, offsets = flight.input_set(call.inputs)
    assert len(keys) == len(values) == call.bound == form.bound and offsets is None
    # the first size of the form (plan_check_tool.ATOMIC_TABLE) is not above the bound
    assert call.bound >= {10: 18_149_377, 11: 36_649_985}[form.bits]
    bits, cap = flight.heavy_constants(call)
    window = model.msd_window(keys, call.bound, bits, cap)
    assert (window["mode"], window["varying"], window["lowest"]) == (model.MODE_PLAN, flight.KEY_BITS, flight.heavy_window(call))
    assert window["lowest"] + bits < 32                      # the window lies below a prefix
    assert flight.verdict_of(call) == (model.VERDICT_MSD_RUNS, flight.heavy_window(call)) and call.verdict == model.VERDICT_MSD_RUNS
    assert bool(((keys >> np.uint32(flight.KEY_BITS)) == np.uint32(model.PREFIX >> flight.KEY_BITS)).all())
    counts = np.bincount(keys & np.uint32((1 << flight.KEY_BITS) - 1), minlength=1 << flight.KEY_BITS)
    tied = int(counts[counts > 1].sum())
    assert tied > call.bound // 2, tied                      # most keys have a tie ...
    assert not np.array_equal(values[:4096], np.arange(4096))   # ... and the values are no index


# ---- the battery on host tensors -----------------------------------------------------------------------------------------

FAULTS = ("cross-status", "middle-repetition", "lost-counter", "stray-sticky", "one-behind-the-other")
TINY_MSD = Call("tiny-msd-declined", "atomic", "vrdxCmdSortKeyValue", "key-value", 16_384, None, "msd", "8-bit", NONE, 0)
SOURCE = SimpleNamespace(input_set=flight.input_set, expected_of=cases.expected_of, verdict_of=lambda call: (call.verdict, None))
REQUIRED = 4096


class FakeEvent:
    def __init__(self, at, open_=False):
        self.at, self.open = at, open_

    def query(self):
        return self.open


class HostRig:
    """in_flight_battery's rig on host tensors.  `record` leaves what the call must leave: the expected arrays, the header
    words (count | verdict or whole plan word | 0 | failure word), its failure word in the sorter's sticky word, its count in
    the plan counters.  Every recording takes 10 us of its lane's clock; both lanes start when the gate opens.
    fault: one of FAULTS.  open_gates: how many gates are already open when the last enqueue is through."""

    def __init__(self, worlds, fault=None, open_gates=0):
        self.torch, self.worlds, self.fault, self.open_gates = torch, worlds, fault, open_gates
        self.clock, self.lane, self.fills = [0, 0], None, []
        self.words = {kind: 0 for kind in battery.KINDS}
        self.plans = {kind: [0, 0] for kind in battery.KINDS}

    @contextlib.contextmanager
    def stream(self, i):
        self.lane = i
        yield
        self.lane = None

    def fill(self, copies):
        self.fills.append(copies)
        self.clock = [0, 0]
        self.open_gates -= 1
        return FakeEvent(0, self.open_gates >= 0)

    def wait(self, i, gate):
        if self.fault == "one-behind-the-other" and i == 1:
            self.clock[1] = self.clock[0]

    def mark(self, i):
        return FakeEvent(self.clock[i])

    def since(self, gate, event):
        return float(event.at - gate.at)

    def record(self, w, call, d, rep):
        assert self.lane is not None and w is self.worlds[self.lane]
        self.clock[self.lane] += 10
        if call.verdict == INHERITED:
            return
        b = d.buffers
        b.keys.copy_(d.expected_keys)
        if d.key_value:
            b.values.copy_(d.expected_values)
            if self.fault == "middle-repetition" and self.lane == 1 and rep == 1:
                b.values[5] ^= 1
        failure = call.failure
        word = d.plan_word if d.plan_word is not None else call.verdict
        header = w.storage[w.off:w.off + 16].view(torch.int32)
        header[:3].copy_(torch.tensor([cases.sorted_count(call) & 0x7FFFFFFF, word, 0], dtype=torch.int32))
        if self.fault != "cross-status":
            header[3] = failure
        elif failure != 0:   # the failure word lands in the neighbour's storage (whose own clean word goes astray)
            header[3] = 0
            other = self.worlds[1 - self.lane]
            other.storage[other.off:other.off + 16].view(torch.int32)[3] = failure
        self.words[call.sorter] |= failure
        for verdict in flight.msd_sorts(call):
            if not (self.fault == "lost-counter" and self.lane == 1 and rep == 1):
                self.plans[call.sorter][0] += 1
            self.plans[call.sorter][1] += 1 if verdict == NONE else 0
        if self.fault == "stray-sticky" and rep == 0:
            self.words["atomic"] |= api.STATUS_LOOKBACK_GAVE_UP

    def synchronize(self):
        pass

    def sticky(self, kind):
        word, self.words[kind] = self.words[kind], 0
        return word

    def counters(self, kind):
        return tuple(self.plans[kind])


@pytest.fixture(scope="module")
def host():
    """two worlds on host tensors, small lanes: a key+value sort with the MSD plan in front that the device turns down, a
    segmented sort that leaves STATUS_SEGMENTS_INVALID, the empty sort, a sort on the other sorter"""
    calls = [TINY_MSD] + [flight.BY_NAME[name] for name in ("segmented-invalid", "empty", "one-workgroup", "range-ballot")]
    shared = {}
    devices = {call.name: recorded_call.device_call(torch, call, shared, REQUIRED, None, source=SOURCE, device="cpu")
               for call in calls}
    first = battery.new_world(torch, devices, recorded_call.OFFSETS[0], device="cpu")
    worlds = [first, battery.second_world(torch, first, recorded_call.OFFSETS[1], device="cpu")]
    return SimpleNamespace(worlds=worlds, calls={call.name: call for call in calls})


def _lanes(host, a="segmented-invalid", b="tiny-msd-declined", reps=(2, 3)):
    return [(host.worlds[i], host.calls[name], reps[i]) for i, name in enumerate((a, b))]


def test_a_correct_fake_passes(host):
    for a, b in (("segmented-invalid", "tiny-msd-declined"), ("segmented-invalid", "segmented-invalid"), ("empty", "one-workgroup"),
                 ("range-ballot", "tiny-msd-declined"), ("segmented-invalid", "empty")):
        rig = HostRig(host.worlds)
        problems, facts = battery.run_lanes(rig, _lanes(host, a, b), 7)
        assert problems == [] and facts.queued and rig.fills == [7], (a, b, problems)
        assert facts.intervals == [(0.0, 20.0), (0.0, 30.0)] and battery.intersection_share(facts.intervals) == 1.0
    assert facts.sticky == {"atomic": api.STATUS_SEGMENTS_INVALID, "ballot": 0}
    # the worlds differ where they must and share what they may
    d0, d1 = (w.device["tiny-msd-declined"] for w in host.worlds)
    assert d0.buffers.keys.data_ptr() != d1.buffers.keys.data_ptr() and d0.buffers.pristine is d1.buffers.pristine
    assert d0.expected_keys is d1.expected_keys and host.worlds[0].storage.data_ptr() != host.worlds[1].storage.data_ptr()
    assert [w.off for w in host.worlds] == [0, 48]


@pytest.mark.parametrize("fault,says", [
    ("cross-status", ["lane 0 segmented-invalid: failure word 0x0, not 0x4", "lane 1 tiny-msd-declined: failure word 0x4, not 0x0"]),
    ("middle-repetition", ["lane 1 tiny-msd-declined: values differ in 1 of 3 repetitions"]),
    ("lost-counter", ["plan counters of the atomic sorter moved by (2, 3), not (3, 3): an update was lost"]),
    ("stray-sticky", ["sticky word of the atomic sorter 0x5, not 0x4: nobody owns 0x1"]),
    ("one-behind-the-other", ["the lanes did not intersect: segmented-invalid ran [0, 20) us behind the gate, "
                              "tiny-msd-declined [20, 50)"]),
])
def test_every_planted_fault_is_caught_by_name(host, fault, says):
    assert fault in FAULTS
    problems, _ = battery.run_lanes(HostRig(host.worlds, fault), _lanes(host), 7)
    assert problems == says, problems
    # ... and what the fault left behind does not outlive it: the next correct run passes
    problems, _ = battery.run_lanes(HostRig(host.worlds), _lanes(host), 7)
    assert problems == []


def test_bytes_around_the_storage_and_guards_are_named(host):
    w = host.worlds[1]
    d = w.device["tiny-msd-declined"]

    class Scribbler(HostRig):
        def record(self, w_, call, d_, rep):
            super().record(w_, call, d_, rep)
            if self.lane == 1 and rep == 1:
                w_.storage[w_.off - 1] ^= 0xFF
                w_.storage[w_.off + d_.required] ^= 0xFF
                w_.storage[-1] ^= 0xFF
                d_.buffers.keys[-1] ^= 1
                d_.buffers.keys[0] ^= 1
    lanes = [(host.worlds[0], host.calls["one-workgroup"], 2), (w, TINY_MSD, 3)]
    problems, _ = battery.run_lanes(Scribbler(host.worlds), lanes, 1)
    assert problems == ["lane 1 tiny-msd-declined: keys differ in 1 of 3 repetitions",
                        "lane 1 tiny-msd-declined: the guard behind the keys changed in 1 of 3 repetitions",
                        "lane 1 tiny-msd-declined: wrote in front of the storage offset",
                        "lane 1 tiny-msd-declined: wrote behind its own storage requirement",
                        "lane 1 tiny-msd-declined: wrote the band behind the storage"], problems
    w.storage[w.off - 1] ^= 0xFF
    w.storage[w.off + d.required] ^= 0xFF
    w.storage[-1] ^= 0xFF
    assert battery.run_lanes(HostRig(host.worlds), lanes, 1)[0] == []


def test_the_filler_doubles_until_the_gate_holds(host):
    filler = SimpleNamespace(copies_per_repetition=1.5, doubled=0)
    rig = HostRig(host.worlds, open_gates=2)     # the first two gates open before the last enqueue
    problems, facts = battery.run_pair(rig, _lanes(host), filler)
    assert problems == [] and facts.queued and rig.fills == [8, 15, 30] and (filler.copies_per_repetition, filler.doubled) == (6.0, 2)
    rig = HostRig(host.worlds, open_gates=99)    # a gate that never holds: four runs, then the pair fails and says why
    problems, facts = battery.run_pair(rig, _lanes(host), filler)
    assert len(rig.fills) == 4 and filler.doubled == 5
    assert problems == ["the gate opened before the last enqueue behind a filler of 240 copies"]
    rig = HostRig(host.worlds, fault="middle-repetition", open_gates=99)   # a failing pair is not run again
    problems, facts = battery.run_pair(rig, _lanes(host), filler)
    assert len(rig.fills) == 1 and any("values differ" in p for p in problems)


class ScriptedEvent:
    """query() answers from a script, then keeps giving the last answer"""

    def __init__(self, *answers):
        self.answers = list(answers)

    def query(self):
        return self.answers.pop(0) if len(self.answers) > 1 else self.answers[0]


def test_calls_beside_says_which_calls_began_inside_the_lane(host):
    calls = []
    # the start event passes at the third poll; the end event has passed when the second call returns
    lane = SimpleNamespace(start=ScriptedEvent(False, False, True), end=ScriptedEvent(False, False, False, True))
    stood = battery.calls_beside(lane, lambda: calls.append(1), 3)
    assert stood == [(True, True), (True, False), (False, False)] and len(calls) == 3
    # a lane that is over before the first call: nothing began inside it
    lane = SimpleNamespace(start=ScriptedEvent(True), end=ScriptedEvent(True))
    assert battery.calls_beside(lane, lambda: None, 2) == [(False, False)] * 2
    # a start event that never passes: the polling gives up, the calls are made and none of them counts
    lane = SimpleNamespace(start=ScriptedEvent(False), end=ScriptedEvent(False))
    assert battery.calls_beside(lane, lambda: None, 2, patience_s=0.01) == [(False, True)] * 2
    # run_lanes hands the hook the lanes in flight, their events among them, between the last enqueue and the synchronise
    seen = []
    problems, _ = battery.run_lanes(HostRig(host.worlds), _lanes(host), 1, while_in_flight=lambda flights: seen.extend(flights))
    assert problems == [] and [lane.call.name for lane in seen] == ["segmented-invalid", "tiny-msd-declined"]
    assert all(hasattr(lane.start, "query") and hasattr(lane.end, "query") for lane in seen)
