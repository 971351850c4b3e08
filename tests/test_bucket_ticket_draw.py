"""The bucket launch's draw (BucketSort2Body in vrdx_kernels.hip), restated without a GPU: W workgroups draw from one ticket
word until it reaches T = 2^bits, bucket = ticket.  Whatever the interleaving, every bucket is sorted exactly once -- for fewer
workgroups than buckets (the resident ones of the fused launch), as many (the half-size kernel's grid) and more (the key+value
launch of 1032 workgroups, the eleven-bit plan's late ones) -- and the word ends at T + W: every workgroup's last draw is the
one that tells it to return.

Inside a workgroup lane 0 of wave 0 draws, and the ticket reaches the other waves through one of TWO words of LDS, taken in
turns.  The first ticket has a barrier of its own; every later one is drawn inside the bucket in front of it and handed on
by that bucket's last barrier -- a bucket without keys has no pass and gets one barrier for this.  Behind such a bucket a wave
that runs ahead draws again before a slower wave has read its ticket, so with a single word that ticket would be overwritten:
the model below runs the waves of a workgroup as coroutines under seeded schedules, shows that two words are enough, and that
the planted fault "one word" is caught.  The model restates the barriers of BucketSort2Body / BucketSort2Bucket by hand: it
pins the design, not the code, and whoever moves a barrier or the draw in those functions has to move it in Workgroup.wave too.

The keys-only output policy follows the ticket: bucket < T - min(plainTail, T) is streamed, the rest keep plain stores, and
the plain ones are the last tickets drawn.
"""
import random

import pytest

T10, T11 = 1 << 10, 1 << 11


# ---- W workgroups, one ticket word ---------------------------------------------------------------------------------------

def draw_all(workgroups, tickets, pick):
    """Every workgroup loops `t = fetch_add(word, 1); if t >= tickets: return; sort bucket t`; pick(alive) names the workgroup
    that takes the next step.  Returns ([(workgroup, bucket), ...] in the order the buckets were taken, the word at the end)."""
    word = 0
    alive = list(range(workgroups))
    taken = []
    while alive:
        w = pick(alive)
        t, word = word, word + 1
        if t >= tickets:
            alive.remove(w)
        else:
            taken.append((w, t))
    return taken, word


def schedules(seed):
    rng = random.Random(seed)
    yield "round-robin", (lambda state: lambda alive: alive[next(state) % len(alive)])(iter(range(1 << 30)))
    yield "first-alive", lambda alive: alive[0]          # one workgroup takes everything, the others arrive to nothing
    yield "last-alive", lambda alive: alive[-1]
    yield "random", lambda alive: rng.choice(alive)
    # a few fast workgroups and many slow ones (a long bucket keeps a workgroup away from the word)
    yield "skewed", lambda alive: alive[min(int(rng.expovariate(1.0)), len(alive) - 1)]


@pytest.mark.parametrize("tickets", [T10, T11])
@pytest.mark.parametrize("workgroups", ["one", "cus", "half", "equal", "kv-grid", "twice"])
def test_every_bucket_is_drawn_exactly_once(tickets, workgroups):
    w = {"one": 1, "cus": 256, "half": tickets // 2, "equal": tickets, "kv-grid": tickets + 8, "twice": 2 * tickets}[workgroups]
    for name, pick in schedules(tickets + w):
        taken, word = draw_all(w, tickets, pick)
        buckets = [b for _, b in taken]
        assert buckets == list(range(tickets)), (name, "buckets are taken in index order, each once")
        assert word == tickets + w, (name, "every workgroup draws once more than it sorts")
        per_workgroup = {}
        for wg, b in taken:
            per_workgroup.setdefault(wg, []).append(b)
        assert all(v == sorted(v) for v in per_workgroup.values()), name
        if name == "first-alive":
            assert len(per_workgroup) == 1


def test_workgroups_that_arrive_late_find_nothing():
    """the resident workgroups have drawn everything: a workgroup started afterwards draws once and returns"""
    taken, word = draw_all(256, T10, lambda alive: alive[0] if alive[0] != 0 else alive[-1] if len(alive) > 1 else 0)
    assert sorted(b for _, b in taken) == list(range(T10)) and word == T10 + 256
    assert all(wg != 0 for wg, _ in taken), "workgroup 0 was scheduled last"


# ---- one workgroup: the ticket's way to every wave ----------------------------------------------------------------------

class Workgroup:
    """V waves as coroutines.  A wave yields "step" after every action another wave could observe and "barrier" at a barrier;
    the scheduler resumes a wave at a barrier only when every live wave stands at one."""

    def __init__(self, waves, tickets, empty, words):
        self.tickets, self.empty, self.words = tickets, empty, words
        self.word = 0                      # the global ticket word
        self.lds = [None] * words          # the words of the staging buffer the ticket travels through
        self.seen = [[] for _ in range(waves)]
        self.waves = [self.wave(v) for v in range(waves)]

    def wave(self, v):
        if v == 0:                         # the first ticket, with a barrier of its own
            self.lds[0], self.word = self.word, self.word + 1
            yield "step"
        yield "barrier"
        turn = 0
        while True:
            yield "step"                   # (leaving a barrier and reading behind it are two events)
            ticket = self.lds[turn % self.words]
            yield "step"
            if ticket >= self.tickets:
                return
            self.seen[v].append(ticket)
            if ticket not in self.empty:   # a bucket with keys: the barriers of its passes in front of the last one
                yield "barrier"
            if v == 0:                     # the next ticket: in the last pass, or at once for a bucket without keys
                self.lds[(turn + 1) % self.words], self.word = self.word, self.word + 1
                yield "step"
            yield "barrier"                # the last pass's last barrier | the empty bucket's only one
            turn += 1

    def run(self, rng):
        state = {i: next(w) for i, w in enumerate(self.waves)}
        while state:
            ready = [i for i, s in state.items() if s == "step"]
            if not ready:                  # every live wave stands at a barrier: all of them pass it
                ready = list(state)
                for i in ready:
                    self._advance(state, i)
                continue
            self._advance(state, rng.choice(ready))
        return self.seen

    def _advance(self, state, i):
        try:
            state[i] = next(self.waves[i])
        except StopIteration:
            del state[i]


def _mismatches(words, seeds, empty):
    bad = 0
    for seed in seeds:
        seen = Workgroup(16, 24, empty, words).run(random.Random(seed))
        bad += any(s != list(range(24)) for s in seen)
    return bad


@pytest.mark.parametrize("empty", [(), tuple(range(24)), tuple(range(0, 24, 2)), (5, 6, 7, 8, 23)],
                         ids=["none-empty", "all-empty", "every-other", "a-run-and-the-last"])
def test_two_words_taken_in_turns_carry_every_ticket_to_every_wave(empty):
    assert _mismatches(2, range(200), set(empty)) == 0


def test_one_word_loses_tickets_behind_empty_buckets():
    """the planted fault: with one word a wave behind an empty bucket reads the ticket of the draw after its own"""
    assert _mismatches(1, range(200), set(range(24))) > 0
    assert _mismatches(1, range(50), set()) == 0, "with a barrier in every bucket one word would do"


# ---- the output policy by ticket ----------------------------------------------------------------------------------------

def streamed(bucket, tickets, plain_tail):
    return bucket < tickets - min(plain_tail, tickets)


@pytest.mark.parametrize("plain_tail", [0, 1, 256, 512, T10, 4 * T10])
def test_the_plain_buckets_are_the_last_tickets_drawn(plain_tail):
    taken, _ = draw_all(256, T10, random.Random(plain_tail).choice)
    kinds = [streamed(b, T10, plain_tail) for _, b in taken]   # in drawing order
    plain = min(plain_tail, T10)
    assert kinds == [True] * (T10 - plain) + [False] * plain
