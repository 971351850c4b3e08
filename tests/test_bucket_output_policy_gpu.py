"""The MSD bucket launch's output policy: which buckets are written with non-temporal stores and which with plain ones
(vrdx_kernels.hip, BucketSort2Body) never shows in the result, so every sort here is compared bit for bit with
np.sort and a stable argsort, keys-only and key+value (values = iota: the permutation and its stability),
at the sizes either side of every switch of the rule:

  * kStreamingLoadsAbove = 2^24 elements, from which key+value writes every bucket non-temporally (the half-size kernel);
  * 18 149 376 | 18 149 377: the half-size bucket kernel | the full-size one (both with plain stores keys-only);
  * 2^25 - 1 | 2^25 (vrdx_kernels.h kMsdStreamedOutputFrom): from here the keys-only full-size launch streams every bucket
    but the last `plainTail` (one per CU) of the launch's order;
  * the last size of the ten-bit plan | the first of the eleven-bit one (plain stores keys-only);
  * inside the full-size ten-bit launch, under an indirect count: keys that fill ONLY buckets of the tail (every store
    plain) and keys that fill NONE of them (every store non-temporal); uniform keys fill both kinds, and workgroups 0 ... 255
    of 512 (buckets b and b + 512) have no tail bucket while the others' second bucket is one.

Next to uniform keys every size runs 24-bit keys, and 2^25 ascending ids: inputs the device takes under a LOWER window.  The
verdict word is read after every sort: a plan the device turned down fails the test, since the four passes would sort the
keys without the bucket launch."""
import functools

import numpy as np
import pytest

import plan_model as model
from test_plan_choice_gpu import plan_storage_word
from guarded_call import sorter, torch_mod  # noqa: F401 (fixtures)
from test_sort_gpu import gpu_sort, MSD_HALF_UP_TO

STREAMING_ABOVE = 1 << 24     # vrdx_kernels.h kStreamingLoadsAbove
TEN_BITS_UP_TO = 36_649_984   # vrdx_plan.h MsdBits (pinned by tests/test_plan_check.py): ceil(n / 1024) * 103 // 100 <= 36864
FULL_CAP = 36864
BUCKETS = 1024                # of the ten-bit plan

SIZES = [STREAMING_ABOVE, STREAMING_ABOVE + 1, MSD_HALF_UP_TO, MSD_HALF_UP_TO + 1, (1 << 25) - 1, 1 << 25, TEN_BITS_UP_TO,
         TEN_BITS_UP_TO + 1]


@functools.lru_cache(maxsize=1)
def _uniform():
    return np.random.default_rng(7025).integers(0, 1 << 32, size=TEN_BITS_UP_TO + 1, dtype=np.uint64).astype(np.uint32)


def check(torch, sorter, keys, shift, count=None, what=""):
    """Sorts the first `count` keys (a device-side count under the bound len(keys) when given) keys-only and key+value with
    values = iota, against np.sort and a stable argsort; the tail behind the count stays as it was; the verdict word must
    say that the MSD plan ran with its window at `shift`."""
    n = len(keys) if count is None else count
    iota = np.arange(len(keys), dtype=np.uint32)
    order = np.argsort(keys[:n], kind="stable").astype(np.uint32)
    want_keys = np.concatenate([keys[:n][order], keys[n:]])
    assert np.array_equal(want_keys[:n], np.sort(keys[:n]))
    want_values = np.concatenate([order, iota[n:]])
    for values in (None, iota):
        kept = []
        got_keys, got_values = gpu_sort(torch, sorter, keys, values, count=count, indirect=count is not None,
                                        max_count=len(keys) if count is not None else None, storage_out=kept)
        mode = "keys-only" if values is None else "key+value"
        word = plan_storage_word(kept[0])
        assert word == (model.VERDICT_MSD_RUNS | (shift << 8)), (what, mode, hex(word), "the device turned the plan down or moved its window")
        assert np.array_equal(got_keys, want_keys), (what, mode)
        assert values is None or np.array_equal(got_values, want_values), (what, mode)


def _expect_shape(sorter, n):
    """the plan the host records at n: (bits, half-size bucket kernel)"""
    for key_value in (False, True):
        info = sorter.describe_plan(n, key_value)
        assert info.name == "msd" and int(info.bits) == (10 if n <= TEN_BITS_UP_TO else 11), (n, info.name, info.bits)
        assert int(info.launches) == (7 if n <= MSD_HALF_UP_TO else 6), (n, info.launches)
    return int(info.bits)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "24-bit"])
@pytest.mark.parametrize("n", SIZES)
def test_sorts_either_side_of_every_switch(torch_mod, sorter, n, kind):
    bits = _expect_shape(sorter, n)
    keys = _uniform()[:n].copy() if kind == "uniform" else model.narrow_keys(_uniform()[:n], 24)
    shift = (32 if kind == "uniform" else 24) - bits
    check(torch_mod, sorter, keys, shift, what=f"{kind} n={n}")


@pytest.mark.gpu
def test_ascending_ids_at_the_headline_size(torch_mod, sorter):
    """0 ... 2^25 - 1: 25 bits vary, the window lies at bit 15 and bucket b is the b-th run of 32768 ids."""
    n = 1 << 25
    assert _expect_shape(sorter, n) == 10
    keys = np.arange(n, dtype=np.uint32)
    check(torch_mod, sorter, keys, 15, what="ascending ids")


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["tail-only", "tail-free"])
def test_keys_that_fill_only_the_tail_or_none_of_it(torch_mod, sorter, where):
    """A bound of 2^25 (the full-size ten-bit launch, the rule switched on) with a device-side count small enough for the keys
    to crowd into part of the buckets: only the last `tail` window values (the tail = one bucket per CU of this device, as
    vrdx_kernels.h MsdPlainTail has it: plain stores throughout) or only the values in front of them (non-temporal stores
    throughout).  The first and the last key, which the sample reads, are 0 and 0xFFFFFFFF, so that the window stays on the
    top ten bits (they put one key into a bucket of the other kind)."""
    bound = 1 << 25
    assert _expect_shape(sorter, bound) == 10
    tail = int(torch_mod.cuda.get_device_properties(torch_mod.cuda.current_device()).multi_processor_count)
    assert 16 <= tail <= BUCKETS - 16, tail
    lo, hi = (BUCKETS - tail, BUCKETS) if where == "tail-only" else (0, BUCKETS - tail)
    count = (hi - lo) * 30_000 + 3  # a mean of 30 000 per used bucket: 40 sigma under the capacity
    keys = _uniform()[:bound].copy()
    top = lo + ((keys[:count].astype(np.uint64) * np.uint64(hi - lo)) >> np.uint64(32))  # evenly over lo ... hi - 1
    keys[:count] = (top.astype(np.uint32) << np.uint32(22)) | (keys[:count] & np.uint32((1 << 22) - 1))
    keys[0], keys[count - 1] = 0, 0xFFFFFFFF
    used = np.bincount(keys[:count] >> np.uint32(22), minlength=BUCKETS)
    assert used.max() <= FULL_CAP and used[lo:hi].sum() >= count - 2
    assert model.msd_verdict(keys, count, 10, FULL_CAP) == (model.VERDICT_MSD_RUNS, 22)
    check(torch_mod, sorter, keys, 22, count=count, what=f"{where} count={count}")
