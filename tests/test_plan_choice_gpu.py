"""What the DEVICE decides about a sort whose host recorded a two-trip plan, at the inputs where such a decision goes wrong
for some key distributions only: the MSD plan's window at every position (every split of the bucket kernel's two passes,
both bucket kernels, keys-only and key+value), the sample's `cap << spread` rule at its boundary, the prefix check at bit
`shift + BITS` and at every place a key can hide from the sample, the plan's last size, tiny device counts under a large
bound, and the byte the hybrid plan scatters by.

Every sort is compared bit for bit with the oracle, keys-only and key+value (values = iota: the permutation itself and its
stability), and the verdict word the device leaves in the storage -- verdict and, when the MSD plan runs, the window's shift
-- with tests/plan_model.py, a plain restatement of the kernels' rules (tests/test_plan_model.py checks it without a GPU).
"""
import functools

import numpy as np
import pytest

import plan_check_tool
import plan_model as model
from guarded_call import ballot_sorter, sorter, torch_mod  # noqa: F401 (fixtures)
from test_sort_gpu import gpu_sort, msd_capacity, MSD_FROM, MSD_HALF_UP_TO  # noqa: F401

HALF = 8_600_003      # the half-size bucket kernel (10 bits, buckets of 18432); n % 4 == 3
FULL10 = 19_000_001   # the full-size bucket kernel, 10 bits (36864)
ELEVEN = 37_000_003   # 11 bits (36864)
LAST = 1 << 26        # 2048 tiles of 32768 = kMsdMaxTiles: the plan's last size


@functools.lru_cache(maxsize=1)
def _uniform():
    """one stream of uniform 32-bit keys, sliced by every test (2^26 + 1 of them)"""
    return np.random.default_rng(2026).integers(0, 1 << 32, size=LAST + 1, dtype=np.uint64).astype(np.uint32)


def plan_storage_word(storage):
    """word 1 of the storage as a whole: the verdict in the low byte, and the MSD window's shift in bits 8-13 when it runs"""
    return int(storage[4:8].cpu().numpy().view(np.uint32)[0])


def expected_word(verdict, shift):
    return verdict | ((shift << 8) if verdict == model.VERDICT_MSD_RUNS else 0)


def model_verdict(sorter, keys, bound, n):
    """the model's (verdict, shift or byte) for the plan the host records for `bound` elements, on the first n keys (the
    same plan keys-only and key+value at the sizes tested here)"""
    info = sorter.describe_plan(bound, False)
    other = sorter.describe_plan(bound, True)
    assert (info.name, info.bits) == (other.name, other.bits), bound
    if info.name == "msd":
        return model.msd_verdict(keys, n, int(info.bits), msd_capacity(bound, int(info.bits)))
    if info.name == "hybrid-8":
        return model.hybrid_verdict(keys, n, model.hybrid_capacity(bound))
    return model.VERDICT_NONE, None


def check(torch, sorter, oracle, keys, count=None, indirect=False, expect=None, what=""):
    """Sorts `keys` keys-only and key+value (values = iota), direct or indirect with a device-side count; both bit for bit
    against ONE oracle run, the tail behind the count untouched, and the word the device left in the storage against the
    model.  expect: the (verdict, shift | byte) the input was built for, checked against the model first.  Returns the
    model's (verdict, shift | byte)."""
    n_buf = len(keys)
    n = n_buf if count is None else count
    bound = n_buf if indirect else n
    iota = np.arange(n_buf, dtype=np.uint32)
    ek, ep, _ = oracle.sort(keys, iota, count=count)
    want = model_verdict(sorter, keys, bound, n)
    if expect is not None:
        assert want == expect, (what, want, expect)
    for values in (None, iota):
        kept = []
        gk, gp = gpu_sort(torch, sorter, keys, values, count=count, indirect=indirect,
                          max_count=bound if indirect else None, storage_out=kept)
        mode = "keys-only" if values is None else "key+value"
        assert np.array_equal(gk, ek), (what, mode)
        assert values is None or np.array_equal(gp, ep), (what, mode)
        if n > 0:
            word = plan_storage_word(kept[0])
            assert word == expected_word(*want), (what, mode, hex(word), want)
    return want


# ---- 1. what the host records: plan and launch count by size -----------------------------------------------------------

# (n, plan, launches): one size inside each shape of a recorded sort and the sizes either side of each switch, the same
# keys-only and key+value with the one-atomic ranking.  Launches are kernels (the state fill and the copy of an indirect
# count are not): the one kernel; histogram + bucket sort + four passes; histogram, spine, scatter (also pass 0), half-size
# buckets, passes 1-3; the same with full-size buckets that are also pass 1; histogram + four passes.
PLAN_TABLE = [(1, "one-workgroup", 1), (4096, "one-workgroup", 1), (16384, "one-workgroup", 1),
              (16385, "hybrid-8", 6), (1 << 20, "hybrid-8", 6), (8_144_384, "hybrid-8", 6),
              (8_144_385, "msd", 7), (12_000_001, "msd", 7), (18_149_376, "msd", 7),
              (18_149_377, "msd", 6), (1 << 25, "msd", 6), (LAST, "msd", 6),
              (LAST + 1, "four-passes", 5), (100_000_000, "four-passes", 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("key_value", [False, True])
@pytest.mark.parametrize("n,plan,launches", PLAN_TABLE)
def test_recorded_plan_and_launch_count_by_size(sorter, n, plan, launches, key_value):
    info = sorter.describe_plan(n, key_value)
    assert (info.name, int(info.launches)) == (plan, launches), (n, key_value)


def _described(sorter, sizes):
    """{(n, key_value): (name, bits, launches)} by vrdxHipDescribePlan"""
    infos = {(n, kv): sorter.describe_plan(n, kv) for n in sizes for kv in (False, True)}
    return {at: (info.name, int(info.bits), int(info.launches)) for at, info in infos.items()}


@pytest.mark.gpu
def test_described_plans_are_the_planners_either_side_of_every_edge(torch_mod, sorter, ballot_sorter):
    """vrdxHipDescribePlan against tests/native/plan_check (the same vrdx_plan.h, compiled for the CPU) for this device's CU
    count, either side of every size at which the plan changes under either ranking: nothing is launched.  A sorter's whole
    set is one table or the other -- the one-atomic ranking's for the sorter every other test here presumes it of (an
    MI355X serves LDS atomics in lane order), the ballot ranking's for the sorter created under VRDX_RANK=ballot."""
    cus = torch_mod.cuda.get_device_properties(0).multi_processor_count
    sizes = sorted(set(plan_check_tool.edge_sizes(plan_check_tool.ATOMIC_TABLE) + plan_check_tool.edge_sizes(plan_check_tool.BALLOT_TABLE) + [1 << 25]))
    tables = {atomic: {at: (row.name, row.bits, row.launches) for at, row in plan_check_tool.describe(cus, atomic, sizes).items()}
              for atomic in (True, False)}
    assert tables[True] != tables[False]
    for which, atomic in ((sorter, True), (ballot_sorter, False)):
        got = _described(which, sizes)
        came_up_atomic = got[1 << 25, False][0] == "msd"   # (only the one-atomic ranking records the MSD plan)
        assert got == tables[came_up_atomic], sorted(at for at in got if got[at] != tables[came_up_atomic][at])
        assert came_up_atomic == atomic


# ---- 2. the window at every position -----------------------------------------------------------------------------------

SWEEP = ([(HALF, v, model.PREFIX) for v in range(2, 33)] + [(HALF, v, 0) for v in (12, 17, 24)]
         + [(FULL10, v, model.PREFIX) for v in range(12, 33)] + [(ELEVEN, v, model.PREFIX) for v in range(13, 33)])


@pytest.mark.gpu
@pytest.mark.parametrize("n,v,prefix", SWEEP)
def test_window_at_every_position(torch_mod, sorter, oracle, n, v, prefix):
    """keys = a constant prefix | v uniform low bits: the window lies right below the prefix, at lowest = max(v, BITS + 2) -
    BITS -- every `below` of the bucket kernel (2 ... 22 at ten bits, 2 ... 21 at eleven: every W0 | W1 split) under the
    half-size kernel, the full-size one and eleven bits; and v = 2 ... 11, which the sample turns down (v = 11 at ten bits:
    512 buckets of 16.8 K still fit)."""
    info = sorter.describe_plan(n, False)
    assert info.name == "msd" and info.bits == (11 if n == ELEVEN else 10)
    bits = int(info.bits)
    keys = model.narrow_keys(_uniform()[:n], v, prefix)
    expect = (model.VERDICT_MSD_RUNS, max(v, bits + 2) - bits) if v >= bits + 1 else None
    verdict, shift = check(torch_mod, sorter, oracle, keys, expect=expect, what=f"n={n} v={v} prefix={prefix:#x}")
    print(f"window n={n} v={v} prefix={prefix:#010x}: verdict {verdict} shift {shift}")
    if v <= bits:
        assert verdict == model.VERDICT_NONE


# ---- 3. the sample's cap << spread rule at its boundary ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,v", [(9_437_184, 11), (9_437_185, 11), (18_874_368, 11), (18_874_369, 11),
                                 (37_748_736, 12), (37_748_737, 12)])
def test_sample_rule_at_cap_times_two_to_the_spread(torch_mod, sorter, oracle, n, v):
    """A random permutation of prefix | (i mod 2^v): every used bucket of the window at bit 2 holds n >> spread keys.  At
    n = cap << spread the plan runs with every bucket exactly full; one key more and the sample turns it down."""
    info = sorter.describe_plan(n, False)
    bits = int(info.bits)
    cap = msd_capacity(n, bits)
    full = n % 2 == 0
    assert info.name == "msd" and ((n if full else n - 1) == cap << (v - 2))
    keys = model.balanced_keys(n, v, seed=n)
    assert model.msd_window(keys, n, bits, cap)["mode"] == (model.MODE_PLAN if full else model.MODE_DECLINED)
    check(torch_mod, sorter, oracle, keys, expect=(model.VERDICT_MSD_RUNS, 2) if full else (model.VERDICT_NONE, None),
          what=f"balanced n={n} v={v}")


# ---- 4. the prefix check at its edges ----------------------------------------------------------------------------------

def _hidden_positions(n):
    """indices the sample never reads: index 1, the four keys of one 16-byte vector of the body, the first and the last key
    of an interior tile of the plan's per-tile counts (tiles are a multiple of 4096 keys, at most 32768), the n & 3 tail"""
    quad = 4 * (n // 12) + 4
    tile = 32768 * 97
    where = [1, quad, quad + 1, quad + 2, quad + 3, tile - 1, tile, n - 3, n - 2]
    assert n % 4 == 3 and not set(where) & set(model.sample_indices(n))
    return where


PREFIX_CASES = [(kind, bit) for kind, bits in (("24-bit", (24, 31)), ("identical", (0, 31))) for bit in bits]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,bit", PREFIX_CASES)
def test_one_key_outside_the_prefix_wherever_the_sample_does_not_look(torch_mod, sorter, oracle, kind, bit):
    """24-bit keys under a prefix (window at bit 14, the prefix checked from bit 24 = shift + BITS up) with ONE key that
    breaks it only at bit 24 or only at bit 31; all keys identical but one that differs only in bit 0 or only in bit 31.  At
    every index the sample does not read the plan must be turned down and the four passes must still sort exactly."""
    n = HALF
    base = (model.narrow_keys(_uniform()[:n], 24) if kind == "24-bit"
            else np.full(n, model.PREFIX, np.uint32))
    assert model_verdict(sorter, base, n, n) == ((model.VERDICT_MSD_RUNS, 14) if kind == "24-bit"
                                                        else (model.VERDICT_MSD_SORTED, None))
    for where in _hidden_positions(n):
        keys = base.copy()
        keys[where] ^= np.uint32(1 << bit)
        check(torch_mod, sorter, oracle, keys, expect=(model.VERDICT_NONE, None), what=f"{kind} bit {bit} at {where}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,bit", PREFIX_CASES)
def test_a_broken_key_and_the_indirect_count(torch_mod, sorter, oracle, kind, bit):
    """The same keys under an indirect count (count % 4 == 2: its last vector is split): a broken key at index count or
    behind it is not part of the sort and must not turn the plan down; at count - 2 (not sampled) it must; at count - 1 it
    is sampled -- the window moves up instead (or the sample sees the keys differ) and the model says what happens."""
    n = HALF
    count = n - n // 3
    count -= (count - 2) % 4
    base = (model.narrow_keys(_uniform()[:n], 24) if kind == "24-bit"
            else np.full(n, model.PREFIX, np.uint32))
    unbroken = (model.VERDICT_MSD_RUNS, 14) if kind == "24-bit" else (model.VERDICT_MSD_SORTED, None)
    assert count % 4 == 2 and count - 2 not in model.sample_indices(count) and count - 1 in model.sample_indices(count)
    for where, expect in ((count, unbroken), (count + 1, unbroken), (n - 1, unbroken), (count - 2, (model.VERDICT_NONE, None)),
                          (count - 1, None)):
        keys = base.copy()
        keys[where] ^= np.uint32(1 << bit)
        got = check(torch_mod, sorter, oracle, keys, count=count, indirect=True, expect=expect,
                    what=f"{kind} bit {bit} at {where}, count {count}")
        print(f"{kind} bit {bit} at count {'%+d' % (where - count)}: verdict {got}")


# ---- 5. the plan's last size -------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_twenty_four_bit_keys_at_the_plans_last_size(torch_mod, sorter, oracle):
    """2^26 keys = 2048 tiles of 32768, eleven bits: 24-bit keys under a prefix take the window at bit 13."""
    info = sorter.describe_plan(LAST, False)
    assert info.name == "msd" and info.bits == 11 and sorter.describe_plan(LAST, True).name == "msd"
    keys = model.narrow_keys(_uniform()[:LAST], 24)
    check(torch_mod, sorter, oracle, keys, expect=(model.VERDICT_MSD_RUNS, 13), what="24-bit at 2^26")


@pytest.mark.gpu
def test_first_size_past_the_plan_runs_four_passes(torch_mod, sorter, oracle):
    """2^26 + 1 keys: 2049 tiles, beyond the MSD plan -- the four passes, whose last tile holds one key."""
    n = LAST + 1
    assert sorter.describe_plan(n, False).name != "msd" and sorter.describe_plan(n, True).name != "msd"
    check(torch_mod, sorter, oracle, _uniform()[:n].copy(), expect=(model.VERDICT_NONE, None), what="2^26 + 1")


# ---- 6. tiny device counts under an MSD-sized bound --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("bound", [8_150_007, 1 << 25, LAST])
def test_tiny_counts_under_a_large_bound(torch_mod, sorter, oracle, bound):
    """The sample indexes t (n - 1) / 63 of the DEVICE count: with 2 ... 63 keys it reads keys twice, with one it finds them
    identical.  Uniform and 24-bit keys, counts from 0 to a bucket's capacity and past it; the tail stays untouched."""
    info = sorter.describe_plan(bound, False)
    assert info.name == "msd" and bound >= MSD_FROM
    cap = msd_capacity(bound, int(info.bits))
    assert cap == (18432 if bound <= MSD_HALF_UP_TO else 36864)
    uniform = _uniform()[:bound]
    for name, keys in (("uniform", uniform), ("24-bit", model.narrow_keys(uniform, 24))):
        for count in (0, 1, 2, 3, 5, 63, 64, 65, 4097, 32768, 32769, cap, cap + 1, 8_149_999):
            got = check(torch_mod, sorter, oracle, keys, count=count, indirect=True, what=f"{name} count {count} of {bound}")
            if count == 1:
                assert got == (model.VERDICT_MSD_SORTED, None)


# ---- 7. the hybrid plan's byte -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [300_007, 900_001, 1_900_003, 7_600_001])
@pytest.mark.parametrize("byte", [2, 1, 0])
def test_hybrid_plan_by_every_byte_at_the_bucket_capacity(torch_mod, sorter, oracle, n, byte):
    """The highest byte that varies is 2, 1 or 0 (the bytes above it constant): the hybrid plan scatters by it -- with byte 0
    the bucket kernel has no bits left to sort.  One value of that byte brought to exactly the capacity (the plan runs) and
    to one more (the four passes), keys-only and key+value, direct and indirect with a smaller count."""
    assert sorter.describe_plan(n, False).name == "hybrid-8" and sorter.describe_plan(n, True).name == "hybrid-8"
    cap = model.hybrid_capacity(n)
    for heavy, verdict in ((cap, model.VERDICT_HYBRID_RUNS), (cap + 1, model.VERDICT_HYBRID_DECLINED)):
        keys = model.hybrid_keys(n, byte, heavy, seed=n + byte)
        check(torch_mod, sorter, oracle, keys, expect=(verdict, byte), what=f"byte {byte} heavy {heavy}")
        check(torch_mod, sorter, oracle, keys, count=n - n // 3, indirect=True, what=f"byte {byte} heavy {heavy} indirect")
