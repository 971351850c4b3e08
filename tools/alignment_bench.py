#!/usr/bin/env python3
"""What a caller pays for arrays off a 16-byte boundary: vrdxCmdSort / vrdxCmdSortKeyValue on arrays at byte offset 256 + a of
their allocations, a in --residues (keys and values at the same residue), taking turns sort by sort in one process.

Per workload and mode: --rounds rounds, each round one event-timed sort per residue (in rotating order) on a fresh copy of the
same input; the median and the minimum GPU time per residue, the ratio of the medians to residue 0, and whether every
residue's result equals residue 0's.  One JSON line per workload and mode.

Workloads: uniform keys at --n (the MSD plan at 2^25), the same with one heavy bucket (the device declines the plan: the four
passes, whose ranking tiles store quads into the caller's arrays), uniform keys at --n-hybrid (the hybrid plan).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--n-hybrid", type=int, default=1 << 22)
    ap.add_argument("--residues", default="0,4,12")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import vulkan_radix_sort_amd as vrdx

    residues = [int(x) for x in args.residues.split(",")]
    assert residues[0] == 0 and all(a % 4 == 0 and 0 <= a < 16 for a in residues)
    sorter = vrdx.Sorter(0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(11)

    def keys_of(kind, n):
        k = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        if kind == "declined":  # 40000 keys with the same top eleven bits: more than a bucket of either bucket kernel holds
            step = max(1, n // 40000)
            k[::step][:40000] = (k[::step][:40000] & np.uint32(0x001FFFFF)) | np.uint32(0x2AC << 21)
        return k

    for name, kind, n in (("uniform", "uniform", args.n), ("declined", "declined", args.n), ("hybrid-size", "uniform", args.n_hybrid)):
        keys = torch.from_numpy(keys_of(kind, n).view(np.int32)).cuda()
        values = torch.from_numpy(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
        for key_value in (False, True):
            size = (sorter.key_value_storage_requirements(n) if key_value else sorter.storage_requirements(n)).size
            storage = torch.empty(size, dtype=torch.uint8, device="cuda")
            bufs = {}
            for a in residues:
                kb = torch.zeros(256 + 16 + 4 * n, dtype=torch.uint8, device="cuda")
                vb = torch.zeros(256 + 16 + 4 * n, dtype=torch.uint8, device="cuda")
                assert kb.data_ptr() % 16 == 0 and vb.data_ptr() % 16 == 0
                bufs[a] = (kb, vb, kb[256 + a:256 + a + 4 * n].view(torch.int32), vb[256 + a:256 + a + 4 * n].view(torch.int32))
            times = {a: [] for a in residues}
            for r in range(args.warmup + args.rounds):
                order = residues[r % len(residues):] + residues[:r % len(residues)]
                for a in order:
                    kb, vb, kview, vview = bufs[a]
                    kview.copy_(keys)
                    vview.copy_(values)
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    if key_value:
                        sorter.cmd_sort_key_value(stream, n, kb.data_ptr(), 256 + a, vb.data_ptr(), 256 + a, storage.data_ptr(), 0)
                    else:
                        sorter.cmd_sort(stream, n, kb.data_ptr(), 256 + a, storage.data_ptr(), 0)
                    stop.record()
                    stop.synchronize()
                    if r >= args.warmup:
                        times[a].append(start.elapsed_time(stop))
            verdict = sorter.read_plan_verdict(stream, storage.data_ptr(), 0)
            same = all(bool((bufs[a][2] == bufs[0][2]).all()) and (not key_value or bool((bufs[a][3] == bufs[0][3]).all()))
                       for a in residues)
            ordered = bool((bufs[0][2].to(torch.int64) & 0xFFFFFFFF).diff().ge(0).all())
            med = {a: statistics.median(times[a]) for a in residues}
            print(json.dumps({"workload": name, "n": n, "key_value": key_value, "plan": sorter.describe_plan(n, key_value).name,
                              "verdict": verdict, "rounds": args.rounds,
                              "median_ms": {str(a): round(med[a], 5) for a in residues},
                              "min_ms": {str(a): round(min(times[a]), 5) for a in residues},
                              "median_vs_residue_0": {str(a): round(med[a] / med[0], 4) for a in residues},
                              "results_equal": same, "sorted": ordered, "status": sorter.read_sorter_status(stream)}), flush=True)
            del bufs, storage
    sorter.destroy()


if __name__ == "__main__":
    main()
