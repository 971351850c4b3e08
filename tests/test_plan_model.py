"""The model of the device's plan decisions (tests/plan_model.py) on the cases the GPU tests already document, and on the
inputs tests/test_plan_choice_gpu.py plants: each lands on the side of the rule it is meant to (no GPU needed)."""
import numpy as np
import pytest

import plan_model as model
from plan_model import VERDICT_MSD_RUNS, VERDICT_MSD_SORTED, VERDICT_NONE, VERDICT_HYBRID_RUNS, VERDICT_HYBRID_DECLINED

HALF_CAP, FULL_CAP = 18432, 36864


def _uniform(n, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def test_sample_indices_take_the_first_and_the_last_key():
    assert model.sample_indices(0) == []
    assert model.sample_indices(1) == [0] * 64
    assert model.sample_indices(2) == [0] * 63 + [1]
    idx = model.sample_indices(8_600_003)
    assert idx[0] == 0 and idx[-1] == 8_600_002 and len(set(idx)) == 64 and idx == sorted(idx)


@pytest.mark.parametrize("n", [8_150_007, (1 << 25) - 12345])
def test_the_documented_msd_cases(n):
    """test_msd_plan_stability_window_choice_and_inputs_it_declines and test_one_captured_graph...: uniform keys take the
    top window, 24-bit keys the window under their prefix, 12-bit keys the lowest window there is, eight-bit keys and four
    values are turned down, all keys identical are left alone, one key outside the prefix where no sample looks declines."""
    cap = HALF_CAP if n < 18_149_376 else FULL_CAP
    r = _uniform(n)
    assert model.msd_verdict(r, n, 10, cap) == (VERDICT_MSD_RUNS, 22)
    k24 = r >> np.uint32(8)
    assert model.msd_verdict(k24, n, 10, cap) == (VERDICT_MSD_RUNS, 14)
    assert model.msd_verdict(r >> np.uint32(20), n, 10, cap) == (VERDICT_MSD_RUNS, 2)
    assert model.msd_window(r >> np.uint32(24), n, 10, cap)["mode"] == model.MODE_DECLINED
    assert model.msd_verdict(r >> np.uint32(24), n, 10, cap) == (VERDICT_NONE, None)
    four = np.array([0xFFFFFFFF, 0, 0x80000001, 0x7FFFFF00], np.uint32)[np.random.default_rng(2).integers(0, 4, n)]
    assert model.msd_verdict(four, n, 10, cap) == (VERDICT_NONE, None)
    for where in (n - 2, n // 2 + 1):
        broken = k24.copy()
        broken[where] |= np.uint32(0x40000000)
        assert where not in model.sample_indices(n)
        assert model.msd_verdict(broken, n, 10, cap) == (VERDICT_NONE, None)
    same = np.full(n, 0x12345678, np.uint32)
    assert model.msd_window(same, n, 10, cap)["mode"] == model.MODE_IDENTICAL
    assert model.msd_verdict(same, n, 10, cap) == (VERDICT_MSD_SORTED, None)
    same[n - 2] ^= np.uint32(1)
    assert model.msd_verdict(same, n, 10, cap) == (VERDICT_NONE, None)


def test_dense_ids_and_the_eleven_bit_window():
    n = 1 << 25
    iota = np.arange(n, dtype=np.uint32)
    assert model.msd_verdict(n - 1 - iota, n, 10, FULL_CAP) == (VERDICT_MSD_RUNS, 15)
    assert model.msd_verdict(iota, n, 10, FULL_CAP) == (VERDICT_MSD_RUNS, 15)
    r = _uniform(37_000_003)
    assert model.msd_verdict(r, len(r), 11, FULL_CAP) == (VERDICT_MSD_RUNS, 21)
    assert model.msd_verdict(r >> np.uint32(8), len(r), 11, FULL_CAP) == (VERDICT_MSD_RUNS, 13)


@pytest.mark.parametrize("n,bits,cap,v", [(9_437_184, 10, HALF_CAP, 11), (18_874_368, 10, FULL_CAP, 11),
                                          (37_748_736, 11, FULL_CAP, 12)])
def test_balanced_keys_sit_on_the_sample_rule_boundary(n, bits, cap, v):
    """n = cap << spread: every used bucket exactly full, the plan runs; one key more: the sample turns it down unseen."""
    assert n == cap << (v - 2)
    k = model.balanced_keys(n, v, seed=v)
    w = model.msd_window(k, n, bits, cap)
    assert (w["varying"], w["lowest"], w["spread"], w["mode"]) == (v, 2, v - 2, model.MODE_PLAN)
    buckets = np.bincount((k >> np.uint32(2)) & np.uint32((1 << bits) - 1), minlength=1 << bits)
    assert int((buckets == cap).sum()) == 1 << (v - 2) and int(buckets.sum()) == n
    assert model.msd_verdict(k, n, bits, cap) == (VERDICT_MSD_RUNS, 2)
    k1 = model.balanced_keys(n + 1, v, seed=v)
    assert model.msd_window(k1, n + 1, bits, cap)["mode"] == model.MODE_DECLINED


def test_window_sweep_covers_every_split_of_the_bucket_kernel():
    """prefix | v uniform bits: below = max(v, BITS + 2) - BITS runs through 2 ... 22 (ten bits) and 2 ... 21 (eleven)."""
    r = _uniform(8_600_003)
    n = len(r)
    seen = set()
    for v in range(12, 33):
        verdict, shift = model.msd_verdict(model.narrow_keys(r, v), n, 10, HALF_CAP)
        assert verdict == VERDICT_MSD_RUNS and shift == max(v, 12) - 10, v
        seen.add(shift)
    assert seen == set(range(2, 23))
    assert model.msd_verdict(model.narrow_keys(r, 11), n, 10, HALF_CAP) == (VERDICT_MSD_RUNS, 2)   # 512 buckets of 16.8 K
    for v in range(2, 11):
        assert model.msd_window(model.narrow_keys(r, v), n, 10, HALF_CAP)["mode"] == model.MODE_DECLINED, v


def test_tiny_counts_repeat_sampled_keys():
    r = _uniform(70)
    assert model.msd_window(r, 1, 10, HALF_CAP)["mode"] == model.MODE_IDENTICAL
    assert model.msd_verdict(r, 1, 10, HALF_CAP) == (VERDICT_MSD_SORTED, None)
    assert model.msd_verdict(r, 2, 10, HALF_CAP) == (VERDICT_MSD_RUNS, 22)
    assert model.msd_verdict(r >> np.uint32(8), 65, 11, FULL_CAP) == (VERDICT_MSD_RUNS, 13)
    assert model.msd_verdict(r, 0, 10, HALF_CAP) == (VERDICT_MSD_RUNS, 2)   # (the sort does nothing; nobody reads this)


def test_prefix_rule_is_checked_from_the_bit_above_the_window():
    n = 8_600_003
    k = model.narrow_keys(_uniform(n), 24)
    assert model.msd_verdict(k, n, 10, HALF_CAP) == (VERDICT_MSD_RUNS, 14)
    for bit, expect in ((23, (VERDICT_MSD_RUNS, 14)), (24, (VERDICT_NONE, None)), (31, (VERDICT_NONE, None))):
        broken = k.copy()
        broken[n - 3] ^= np.uint32(1 << bit)
        assert model.msd_verdict(broken, n, 10, HALF_CAP) == expect, bit
    # the last key is sampled: flipped at bit 24 it moves the window up by one, and the plan runs there
    broken = k.copy()
    broken[n - 1] ^= np.uint32(1 << 24)
    assert model.msd_verdict(broken, n, 10, HALF_CAP) == (VERDICT_MSD_RUNS, 15)


@pytest.mark.parametrize("n", [300_007, 900_001, 1_900_003, 7_600_001])
def test_hybrid_byte_and_capacity(n):
    cap = model.hybrid_capacity(n)
    assert cap == {300_007: 4096, 900_001: 8192, 1_900_003: 16384, 7_600_001: 32768}[n]
    for byte in (3, 2, 1, 0):
        assert model.hybrid_verdict(model.hybrid_keys(n, byte, cap, seed=byte), n, cap) == (VERDICT_HYBRID_RUNS, byte)
        assert model.hybrid_verdict(model.hybrid_keys(n, byte, cap + 1, seed=byte), n, cap) == (VERDICT_HYBRID_DECLINED, byte)
    assert model.hybrid_verdict(np.full(n, 7, np.uint32), n, cap) == (VERDICT_HYBRID_DECLINED, None)
    assert model.hybrid_capacity(8_144_384) == 32768 and model.hybrid_capacity(8_144_385) == 0
