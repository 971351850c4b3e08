"""The 32-bit sorts on caller arrays that start at any uint32 of a larger allocation.

The contract (include/vk_radix_sort.h, "Alignment and bounds"): keysBuffer + keysOffset, valuesBuffer + valuesOffset and
indirectBuffer + indirectOffset are multiples of 4 and nothing more; nothing outside [0, elementCount) of the caller's arrays
is written.  The kernels read keys sixteen bytes at a time in the two histogram kernels and the ranking tiles of the
passes store sorted quads sixteen bytes at a time (u32x4_a4 in vrdx_kernels.hip; profiles/r11_alignment_audit.txt), so every
plan is run here with its arrays at 0, 4, 8 and 12 mod 16, between two bands of sentinel bytes, through the C-ABI's offset
arguments:

  one workgroup | the hybrid plan | its four passes (all, three + a copy, two, one + a copy) | the MSD plan with the
  half-size and the full-size bucket kernel, ten and eleven bits, the non-temporal bucket output from 2^25 keys | the four
  passes behind a declined MSD plan and past its last size | the count word at any residue, alone and right behind the keys |
  the MSD window and verdict against tests/plan_model.py | one captured graph replayed | the ballot ranking.

Values are random words, never the index: a value stored one slot off differs from the right one.  References: np.sort for
keys-only, the oracle's stable sort for key+value (kept out of the three largest sizes).
"""
import functools

import numpy as np
import pytest

import plan_model as model
from guarded_call import (BAND_BYTE, FRONT, TAIL, address, ballot_sorter, guarded_call, poisoned_storage, sorter, to_device,  # noqa: F401
                          to_host, torch_mod)
from test_sort_gpu import msd_capacity, MSD_FROM, MSD_HALF_UP_TO
from test_plan_choice_gpu import plan_storage_word, expected_word, model_verdict

pytestmark = pytest.mark.gpu

RESIDUES = (0, 4, 8, 12)
LAST = 1 << 26      # the MSD plan's last size


@functools.lru_cache(maxsize=1)
def _uniform():
    """one stream of uniform 32-bit keys, sliced by every test (2^26 + 1 of them)"""
    return np.random.default_rng(1018).integers(0, 1 << 32, size=LAST + 1, dtype=np.uint64).astype(np.uint32)


@functools.lru_cache(maxsize=1)
def _payload():
    """one stream of random values for every key+value case (none beyond 18.2 M elements)"""
    return np.random.default_rng(4242).integers(0, 1 << 32, size=18_149_379, dtype=np.uint64).astype(np.uint32)


def reference(oracle, keys, values=None, count=None):
    """(keys, values) of the whole arrays after a stable sort of the first `count` elements; the rest as it was"""
    if values is not None:
        ek, ev, _ = oracle.sort(keys, values, count=count)
        return ek, ev
    n = len(keys) if count is None else count
    ek = keys.copy()
    ek[:n] = np.sort(keys[:n])
    return ek, None


def run_placed(torch, sorter, keys, values, a_keys, a_values, want, count=None, count_at=None, a_count=0, word=None, what=""):
    """One vrdxCmdSort* on arrays guarded_call places: keys at a_keys mod 16 of a buffer of their own, values at a_values
    mod 16 of another, both between sentinel bands, the offsets passed as keysOffset / valuesOffset.  count: the indirect
    form, bound = len(keys), the count word at a_count mod 16 of its own buffer (count_at = "own") or right behind the last
    key in the keys' buffer ("keys": its residue is then a_keys + 4 len(keys) mod 16).  want: (keys, values) of `reference`.
    Checks keys and values (the tail behind the count with them), every sentinel band, the count word, the guard behind the
    storage requirement, read_status == 0 and, where given, the plan word the device left in the storage."""
    n_buf = len(keys)
    indirect = count is not None
    n = count if indirect else n_buf
    key_value = values is not None
    what = (what, f"n={n_buf} count={count} at {count_at} a_keys={a_keys} a_values={a_values} a_count={a_count} kv={key_value}")
    assert {a_keys, a_values, a_count} <= set(RESIDUES) and FRONT % 16 == 0 and (not indirect or count_at in ("own", "keys"))
    try:
        got = guarded_call(torch, sorter, keys, values, device_count=count, keys_off=a_keys, values_off=a_values,
                           indirect_off=a_count, count_behind_keys=0 if indirect and count_at == "keys" else None, recorded=n > 0)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from e
    assert np.array_equal(got.keys[n:], keys[n:]), (what, "keys from the count on were touched")
    assert np.array_equal(got.keys, want[0]), (what, "keys")
    if key_value:
        assert np.array_equal(got.values[n:], values[n:]), (what, "values from the count on were touched")
        assert np.array_equal(got.values, want[1]), (what, "values")
    if word is not None:
        assert plan_storage_word(got.storage) == word, (what, hex(plan_storage_word(got.storage)), hex(word))
    return got.storage


def other_residue(a, k):
    """a residue different from a, chosen by k"""
    return (a + 4 * (1 + k % 3)) % 16


def every_mode(torch, sorter, oracle, keys, values, a_keys, a_values, word=None, count_word=None, what=""):
    """keys-only and key+value, direct and indirect with count = n - 3 (the count word at the values' residue)"""
    n = len(keys)
    count = max(n - 3, 0)
    for cnt in (None, count):
        want = reference(oracle, keys, values, count=cnt)
        w = word if cnt is None else count_word
        run_placed(torch, sorter, keys, None, a_keys, a_values, want, count=cnt, count_at="own", a_count=a_values, word=w, what=what)
        run_placed(torch, sorter, keys, values, a_keys, a_values, want, count=cnt, count_at="own", a_count=a_keys, word=w, what=what)


# ---- one workgroup: 1 ... 16384 elements --------------------------------------------------------------------------------

ONE_WORKGROUP_SIZES = [1, 2, 3, 4, 5, 7] + list(range(4093, 4100)) + list(range(16381, 16385))


def one_workgroup_row(torch, sorter, oracle, n, a):
    assert sorter.describe_plan(n, False).name == "one-workgroup" and sorter.describe_plan(n, True).name == "one-workgroup"
    k, v = oracle.generate(100 + n % 89, n, 32)
    every_mode(torch, sorter, oracle, k, v, a, other_residue(a, n), what="one workgroup")


@pytest.mark.parametrize("a", RESIDUES)
@pytest.mark.parametrize("n", ONE_WORKGROUP_SIZES)
def test_one_workgroup_at_every_residue(torch_mod, sorter, oracle, n, a):
    """Both forms of the one-workgroup kernel (256 threads to 4096 elements, 1024 to 16384) at their edges and at n mod 4 =
    0 ... 3; values at another residue than the keys; direct, and indirect with count = n - 3."""
    one_workgroup_row(torch_mod, sorter, oracle, n, a)


# ---- the hybrid plan and the four passes at its sizes -------------------------------------------------------------------

HYBRID_SIZES = [16385, 70_001, 70_002, 70_003, 70_004]
HYBRID_ROWS = [(n, a) for n in HYBRID_SIZES for a in RESIDUES] + [(3_000_001, 4)]


def hybrid_row(torch, sorter, oracle, n, a):
    assert sorter.describe_plan(n, False).name == "hybrid-8" and sorter.describe_plan(n, True).name == "hybrid-8"
    k, v = _uniform()[:n].copy(), _payload()[:n].copy()
    runs = (model.VERDICT_HYBRID_RUNS, 3)
    assert model.hybrid_verdict(k, n, model.hybrid_capacity(n)) == runs and model.hybrid_verdict(k, n - 3, model.hybrid_capacity(n)) == runs
    every_mode(torch, sorter, oracle, k, v, a, other_residue(a, n), word=model.VERDICT_HYBRID_RUNS,
               count_word=model.VERDICT_HYBRID_RUNS, what="hybrid")


@pytest.mark.parametrize("n,a", HYBRID_ROWS)
def test_hybrid_plan_at_every_residue(torch_mod, sorter, oracle, n, a):
    """Uniform keys: the histogram's sixteen-byte loads, the scatter by the top byte out of the caller's arrays and one
    workgroup per bucket back into them.  The first size of the plan, n mod 4 = 0 ... 3 at 70 K, and 3 M (tiles of 32 keys
    per thread)."""
    hybrid_row(torch_mod, sorter, oracle, n, a)


@pytest.mark.parametrize("byte", [3, 2, 1, 0])
@pytest.mark.parametrize("n,a", HYBRID_ROWS)
def test_four_passes_at_a_hybrid_size(torch_mod, sorter, oracle, n, a, byte):
    """One value of the highest varying byte occurs once more than a bucket holds (test_sort_gpu.py,
    test_hybrid_plan_and_its_fallback_at_the_bucket_capacity): the device declines the plan and the four passes run from the
    misaligned arrays.  Keys of 32, 24, 16 and 8 significant bits under a constant prefix: four ranking passes; three and a
    copy pass; two, the other two skipped; one and a copy pass -- whichever pass is last writes the caller's arrays."""
    cap = model.hybrid_capacity(n)
    assert sorter.describe_plan(n, False).name == "hybrid-8" and 0 < cap < n
    k = model.hybrid_keys(n, byte, cap + 1, seed=n + byte)
    v = _payload()[:n].copy()
    assert model.hybrid_verdict(k, n, cap) == (model.VERDICT_HYBRID_DECLINED, byte)
    want = reference(oracle, k, v)
    a_values = other_residue(a, n + byte)
    what = f"four passes, {8 * byte + 8}-bit keys"
    run_placed(torch_mod, sorter, k, None, a, a_values, want, word=model.VERDICT_HYBRID_DECLINED, what=what)
    run_placed(torch_mod, sorter, k, v, a, a_values, want, word=model.VERDICT_HYBRID_DECLINED, what=what)
    count = n - 3   # (the heavy value may lose up to three keys: the verdict is the model's)
    want = reference(oracle, k, v, count=count)
    run_placed(torch_mod, sorter, k, v, a, a_values, want, count=count, count_at="own", a_count=other_residue(a_values, byte),
               word=model.hybrid_verdict(k, count, cap)[0], what=what + " indirect")


# ---- the ballot ranking: the same rows of the one-workgroup kernel and the hybrid plan ------------------------------------

@pytest.mark.parametrize("a", RESIDUES)
@pytest.mark.parametrize("n", ONE_WORKGROUP_SIZES)
def test_ballot_ranking_one_workgroup_at_every_residue(torch_mod, ballot_sorter, oracle, n, a):
    one_workgroup_row(torch_mod, ballot_sorter, oracle, n, a)


@pytest.mark.parametrize("n,a", HYBRID_ROWS)
def test_ballot_ranking_hybrid_plan_at_every_residue(torch_mod, ballot_sorter, oracle, n, a):
    hybrid_row(torch_mod, ballot_sorter, oracle, n, a)


# ---- the MSD plan ---------------------------------------------------------------------------------------------------------

def msd_word(sorter, keys, n=None):
    """(plan word the model expects, its (verdict, shift)) for a direct sort of these keys, or of the first n under the bound"""
    want = model_verdict(sorter, keys, len(keys), len(keys) if n is None else n)
    return expected_word(*want), want


def hidden_index(n):
    """an index in the middle of the array that the sample of 64 keys does not read"""
    where = n // 2 + 1
    assert where not in model.sample_indices(n)
    return where


@pytest.mark.parametrize("n,a_keys,a_values", [(8_150_001, 4, 12), (8_150_002, 8, 4), (8_150_003, 12, 8), (8_150_004, 4, 4)])
@pytest.mark.parametrize("declined", [False, True])
def test_msd_plan_with_half_size_buckets(torch_mod, sorter, oracle, n, a_keys, a_values, declined):
    """The first sizes of the MSD plan (ten bits, buckets of at most 18432, the 512-thread bucket kernel), n mod 4 = 1, 2,
    3, 0.  Uniform keys: verdict 3.  Declined: 24-bit keys under a prefix with ONE key outside it where the sample does not
    look -- the histogram kernel has to see it through its misaligned loads, and the four passes then run."""
    info = sorter.describe_plan(n, True)
    assert info.name == "msd" and info.bits == 10 and msd_capacity(n, 10) == 18432 and n > MSD_FROM
    if declined:
        k = model.narrow_keys(_uniform()[:n], 24)
        assert msd_word(sorter, k)[1] == (model.VERDICT_MSD_RUNS, 14)
        k[hidden_index(n)] ^= np.uint32(1 << 31)
    else:
        k = _uniform()[:n].copy()
    v = _payload()[:n].copy()
    word, verdict = msd_word(sorter, k)
    assert verdict == ((model.VERDICT_NONE, None) if declined else (model.VERDICT_MSD_RUNS, 22))
    want = reference(oracle, k, v)
    run_placed(torch_mod, sorter, k, None, a_keys, a_values, want, word=word, what="msd half")
    run_placed(torch_mod, sorter, k, v, a_keys, a_values, want, word=word, what="msd half")


@pytest.mark.parametrize("a_keys,a_values", [(4, 12), (12, 8)])
@pytest.mark.parametrize("key_value", [False, True])
@pytest.mark.parametrize("n", [18_149_377, 18_149_379])
def test_msd_plan_with_full_size_buckets(torch_mod, sorter, oracle, n, key_value, a_keys, a_values):
    """The first sizes of the full-size bucket kernel (buckets of at most 36864; its launch is also pass 1)."""
    info = sorter.describe_plan(n, key_value)
    assert info.name == "msd" and info.bits == 10 and msd_capacity(n, 10) == 36864 and n > MSD_HALF_UP_TO
    k = _uniform()[:n].copy()
    v = _payload()[:n].copy() if key_value else None
    word, verdict = msd_word(sorter, k)
    assert verdict == (model.VERDICT_MSD_RUNS, 22)
    run_placed(torch_mod, sorter, k, v, a_keys, a_values, reference(oracle, k, v), word=word, what="msd full")


@pytest.mark.parametrize("a", [4, 12])
@pytest.mark.parametrize("kind", ["uniform", "24-bit"])
@pytest.mark.parametrize("n", [(1 << 25) + 1, (1 << 25) + 3])
def test_non_temporal_bucket_output(torch_mod, sorter, oracle, n, kind, a):
    """From 2^25 keys the keys-only bucket kernel streams all but the last bucket of every CU out with non-temporal stores
    (tests/test_bucket_output_policy_gpu.py covers aligned arrays): uniform keys (window at the top) and 24-bit keys (window
    at bit 14)."""
    assert sorter.describe_plan(n, False).name == "msd"
    k = _uniform()[:n].copy() if kind == "uniform" else model.narrow_keys(_uniform()[:n], 24)
    word, verdict = msd_word(sorter, k)
    assert verdict == (model.VERDICT_MSD_RUNS, 22 if kind == "uniform" else 14)
    run_placed(torch_mod, sorter, k, None, a, 0, reference(oracle, k), word=word, what="non-temporal " + kind)


def test_eleven_bit_window(torch_mod, sorter, oracle):
    """The first sizes of the eleven-bit plan, keys at 8 mod 16.  Ten bits end where ceil(n / 1024) * 103 // 100 exceeds
    36864 (MsdBits in vrdx_plan.h), which is n = 36 649 985: this is the third size past it, n mod 4 == 3."""
    n = 36_649_987
    info = sorter.describe_plan(n, False)
    assert info.name == "msd" and info.bits == 11 and n % 4 == 3
    k = _uniform()[:n].copy()
    word, verdict = msd_word(sorter, k)
    assert verdict == (model.VERDICT_MSD_RUNS, 21)
    run_placed(torch_mod, sorter, k, None, 8, 0, reference(oracle, k), word=word, what="eleven bits")


def test_four_passes_past_the_msd_plan(torch_mod, sorter, oracle):
    """2^26 + 1 keys at 4 mod 16: the four passes of the large regime, recorded with no plan in front (the last tile holds
    one key)."""
    n = LAST + 1
    assert sorter.describe_plan(n, False).name == "four-passes"
    k = _uniform()[:n].copy()
    run_placed(torch_mod, sorter, k, None, 4, 0, reference(oracle, k), word=model.VERDICT_NONE, what="past the plan")


# ---- the window and the verdict off alignment -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["uniform", "24-bit", "identical"])
@pytest.mark.parametrize("n,a", [(8_150_001, 4), (8_150_002, 8), (8_150_003, 12)])
def test_window_and_verdict_under_misalignment(torch_mod, sorter, oracle, n, a, kind):
    """The histogram kernel of the MSD plan samples the keys, places the window, checks every key against the prefix and
    counts the buckets -- all through its sixteen-byte loads.  The plan word it leaves (verdict, shift) against the model, as
    test_plan_choice_gpu.check does: window at bit 22, at bit 14 below a prefix, and verdict 4 for identical keys (every key
    compared with key 0).  A histogram that counts wrongly off alignment fails here first."""
    k = {"uniform": lambda: _uniform()[:n].copy(), "24-bit": lambda: model.narrow_keys(_uniform()[:n], 24),
         "identical": lambda: np.full(n, model.PREFIX, np.uint32)}[kind]()
    v = _payload()[:n].copy()
    word, verdict = msd_word(sorter, k)
    assert verdict == {"uniform": (model.VERDICT_MSD_RUNS, 22), "24-bit": (model.VERDICT_MSD_RUNS, 14),
                       "identical": (model.VERDICT_MSD_SORTED, None)}[kind]
    want = (k, v) if kind == "identical" else reference(oracle, k, v)
    a_values = other_residue(a, n)
    run_placed(torch_mod, sorter, k, None, a, a_values, want, word=word, what="window " + kind)
    run_placed(torch_mod, sorter, k, v, a, a_values, want, word=word, what="window " + kind)
    if kind == "identical":   # ... and one key that differs in bit 0 only, where the sample does not look: the four passes
        k[hidden_index(n)] ^= np.uint32(1)
        word, verdict = msd_word(sorter, k)
        assert verdict == (model.VERDICT_NONE, None)
        run_placed(torch_mod, sorter, k, v, a, a_values, reference(oracle, k, v), word=word, what="identical but one")


# ---- the count word -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("residue", [4, 8, 12])
@pytest.mark.parametrize("count_at", ["own", "keys"])
@pytest.mark.parametrize("bound,count", [(5003, 4098), (8_150_003, 5_012_345)])
def test_count_word_at_every_residue(torch_mod, sorter, oracle, bound, count, count_at, residue):
    """The indirect forms read one uint32 at indirectBuffer + indirectOffset: at 4, 8 and 12 mod 16, in a buffer of its own
    and in the keys' buffer right behind the last key (where a kernel that reads or writes one vector past the keys meets
    it).  A one-workgroup size, and an MSD-size bound whose count ends in the middle of a tile and of a sixteen-byte vector."""
    a_keys = (residue - 4 * bound) % 16 if count_at == "keys" else other_residue(residue, bound)
    a_values = other_residue(a_keys, count)
    k, v = _uniform()[:bound].copy(), _payload()[:bound].copy()
    assert count % 4 != 0 and count % 4096 != 0
    word = msd_word(sorter, k, count)[0] if bound > MSD_FROM else None
    want = reference(oracle, k, v, count=count)
    for values in (None, v):
        run_placed(torch_mod, sorter, k, values, a_keys, a_values, want, count=count, count_at=count_at, a_count=residue,
                   word=word, what="count word")


# ---- one captured sort ----------------------------------------------------------------------------------------------------

def test_graph_replay_on_misaligned_arrays(torch_mod, sorter, oracle):
    """One key+value sort at an MSD size captured on arrays at 4 (keys) and 12 (values) mod 16 -- on a single stream, after
    one eager sort, as test_sort_gpu.py captures -- and replayed on uniform keys, 24-bit keys and identical keys: window and
    verdict are the device's at every replay, the sentinel bands stay intact."""
    torch = torch_mod
    n = 8_150_003
    uniform, v = _uniform()[:n].copy(), _payload()[:n].copy()
    inputs = [("uniform", uniform), ("24-bit", model.narrow_keys(uniform, 24)), ("identical", np.full(n, model.PREFIX, np.uint32))]
    dk, dv = to_device(torch, uniform, FRONT + 4, TAIL), to_device(torch, v, FRONT + 12, TAIL)
    size = sorter.key_value_storage_requirements(n).size
    storage = poisoned_storage(torch, size)

    def record(stream):
        sorter.cmd_sort_key_value(stream, n, *address(dk), *address(dv), storage.data_ptr(), 0)

    record(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        record(torch.cuda.current_stream().cuda_stream)
    stream = torch.cuda.current_stream().cuda_stream
    for name, k in inputs:
        dk.copy_(torch.from_numpy(k.view(np.int32)))
        dv.copy_(torch.from_numpy(v.view(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ek, ev = (k, v) if name == "identical" else reference(oracle, k, v)
        assert np.array_equal(to_host(dk, guarded=True, what=f"{name} keys"), ek), name
        assert np.array_equal(to_host(dv, guarded=True, what=f"{name} values"), ev), name
        assert plan_storage_word(storage) == msd_word(sorter, k)[0], name
        assert bool((storage[size:] == BAND_BYTE).all()), name
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0, name
