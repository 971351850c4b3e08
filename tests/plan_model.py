"""A plain-Python model of what the DEVICE decides about a sort whose host recorded a two-trip plan in front of the four
passes -- restated from vrdx_kernels.hip, not derived from the kernels' output:

  MSD plan (histogram_msd_kernel, spine_msd_kernel, the scatter role of msd_scatter_or_pass0_kernel):
    wave 0 samples 64 keys at indices t (n - 1) / 63 of the DEVICE count n; `varying` = one past the highest bit in which
    two sampled keys differ; the window of BITS bits starts at lowest = max(varying, BITS + 2) - BITS; spread = the varying
    bits inside it.  Then, in this order:
      identical   all sampled keys equal (n != 0, varying == 0): verdict 4 if ALL n keys equal key 0, else the four passes;
      declined    spread < BITS and n > cap << spread (too few buckets can hold anything);
      skew        a window bucket holds seen >= 8 of the 64 sampled keys with seen * n / 64 > cap;
      prefix      (window below the top only) a key that differs from key 0 at bit lowest + BITS or above;
      spine       a window bucket beyond cap keys.
    Any of the last four: the four passes run (verdict 0).  Otherwise verdict 3, and the scatter's shift (= the bits the
    bucket kernel sorts below the window) is `lowest`.

  hybrid plan (HybridByte): t = the highest byte that is not the same in all n keys; verdict 1 if no value of byte t occurs
    more than the capacity times, else 2 (also when all keys are equal: no byte varies).
"""
import numpy as np

SAMPLE_KEYS = 64   # kMsdSampleKeys
SAMPLE_SKEW = 8    # kMsdSampleSkew

VERDICT_NONE, VERDICT_HYBRID_RUNS, VERDICT_HYBRID_DECLINED, VERDICT_MSD_RUNS, VERDICT_MSD_SORTED = 0, 1, 2, 3, 4

MODE_PLAN, MODE_DECLINED, MODE_IDENTICAL = "plan", "declined", "identical"


def sample_indices(n):
    """the 64 indices wave 0 reads (first and last key among them; repeated keys when n < 64)"""
    return [(t * (n - 1)) // (SAMPLE_KEYS - 1) for t in range(SAMPLE_KEYS)] if n else []


def msd_window(keys, n, bits, cap):
    """What the sample says: dict(varying, lowest, spread, mode)."""
    sampled = [int(keys[i]) for i in sample_indices(n)] or [0] * SAMPLE_KEYS   # (n == 0: nothing is loaded, lanes hold 0)
    ones = zeros = 0
    for s in sampled:
        ones |= s
        zeros |= ~s & 0xFFFFFFFF
    varying = (ones & zeros).bit_length()
    lowest = max(varying, bits + 2) - bits
    spread = varying - lowest if varying > lowest else 0
    if n != 0 and varying == 0:
        mode = MODE_IDENTICAL
    elif spread < bits and n > (cap << spread):
        mode = MODE_DECLINED
    else:
        mode = MODE_PLAN
        seen = {}
        for s in sampled:
            b = (s >> lowest) & ((1 << bits) - 1)
            seen[b] = seen.get(b, 0) + 1
        # (lane by lane the atomic hands out 1 ... c in a bucket of c sampled keys: the largest is the one that decides)
        if any(c >= SAMPLE_SKEW and c * n // SAMPLE_KEYS > cap for c in seen.values()):
            mode = MODE_DECLINED
    return dict(varying=varying, lowest=lowest, spread=spread, mode=mode)


def msd_verdict(keys, n, bits, cap):
    """(verdict, shift): (VERDICT_MSD_RUNS, the window's lowest bit), (VERDICT_MSD_SORTED, None) or (VERDICT_NONE, None)
    for the first n keys under the plan recorded with `bits` and `cap` (describe_plan of the bound, msd_capacity)."""
    w = msd_window(keys, n, bits, cap)
    k = np.asarray(keys[:n], dtype=np.uint32)
    if w["mode"] == MODE_DECLINED:
        return VERDICT_NONE, None
    if w["mode"] == MODE_IDENTICAL:
        return (VERDICT_MSD_SORTED, None) if bool((k == k[0]).all()) else (VERDICT_NONE, None)
    shift = w["lowest"]
    if n == 0:
        return VERDICT_MSD_RUNS, shift
    if shift != 32 - bits:   # the window lies below a prefix: every key is checked against key 0 from bit shift + BITS up
        if bool(((k ^ k[0]) >> np.uint32(shift + bits)).any()):
            return VERDICT_NONE, None
    buckets = np.bincount((k >> np.uint32(shift)) & np.uint32((1 << bits) - 1), minlength=1 << bits)
    if int(buckets.max()) > cap:
        return VERDICT_NONE, None
    return VERDICT_MSD_RUNS, shift


def hybrid_capacity(n):
    """HybridCapacity (vrdx_plan.h; pinned by tests/test_plan_check.py) for the one-atomic ranking: the smallest of 4096 ... 32768 that leaves twice the
    mean bucket of the host's element count, the largest also with 3 % room; 0 = no hybrid plan."""
    mean = -(-n // 256)
    need, need_last = mean * 200 // 100, mean * 103 // 100
    for cap in (4096, 8192, 16384, 32768):
        if need <= cap:
            return cap
    return 32768 if need_last <= 32768 else 0


def hybrid_verdict(keys, n, cap):
    """(verdict, byte): (VERDICT_HYBRID_RUNS, t) or (VERDICT_HYBRID_DECLINED, t or None) for the first n keys."""
    k = np.asarray(keys[:n], dtype=np.uint32)
    top = None
    for byte in range(3, -1, -1):
        counts = np.bincount((k >> np.uint32(8 * byte)) & np.uint32(0xFF), minlength=256)
        if int(counts.max()) != n:   # (a byte whose one value holds every key is constant)
            top = byte
            break
    if top is None:
        return VERDICT_HYBRID_DECLINED, None
    return (VERDICT_HYBRID_RUNS if int(counts.max()) <= cap else VERDICT_HYBRID_DECLINED), top


# ---- the inputs the tests plant ------------------------------------------------------------------------------------------
PREFIX = 0xA5C35A96   # the constant the narrow keys carry above their varying bits (nonzero in every position)


def prefix_of(v, prefix=PREFIX):
    """the bits of `prefix` above the low v"""
    return (prefix & ~((1 << v) - 1)) & 0xFFFFFFFF


def narrow_keys(uniform, v, prefix=PREFIX):
    """prefix | v uniform low bits (the top v bits of uniform 32-bit keys)"""
    low = uniform >> np.uint32(32 - v) if v > 0 else np.zeros_like(uniform)
    return low | np.uint32(prefix_of(v, prefix))


def balanced_keys(n, v, seed, prefix=PREFIX):
    """a random permutation of prefix | (i mod 2^v), i < n: every window bucket the low v bits reach holds the same number
    of keys when 2^v divides n"""
    perm = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    return (perm & np.uint32((1 << v) - 1)) | np.uint32(prefix_of(v, prefix))


def hybrid_keys(n, byte, heavy, seed, value=0x5A, prefix=PREFIX):
    """keys whose highest byte that varies is `byte` (the bytes above it are the prefix's), uniform below, with EXACTLY
    `heavy` keys whose byte `byte` is `value` (the others' values of that byte are drawn from the remaining 255)"""
    rng = np.random.default_rng(seed)
    bits = 8 * byte
    low = rng.integers(0, 1 << bits, size=n, dtype=np.uint64).astype(np.uint32) if bits else np.zeros(n, np.uint32)
    digit = rng.integers(0, 255, size=n, dtype=np.uint64).astype(np.uint32)
    digit += (digit >= value).astype(np.uint32)                  # never `value` ...
    digit[rng.choice(n, size=heavy, replace=False)] = value      # ... except exactly `heavy` keys
    return low | (digit << np.uint32(bits)) | np.uint32(prefix_of(bits + 8, prefix))
