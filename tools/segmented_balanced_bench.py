#!/usr/bin/env python3
"""Times the balanced segmented sort (vrdxHipCmdBalancedSortSegmented[KeyValue]) on one GPU against what a caller had without
it.  All variants run in ONE process and take turns, step by step, on fresh copies of the same seeded keys; times are
device-event times (a pair of torch events around what the variant enqueues, inputs prepared and the device idle before the
first event), medians over the steps after --warmup rounds; each row prints ONE JSON line.

  balanced    (a) one vrdxHipCmdBalancedSortSegmented[KeyValue] call
  segmented   (b) one vrdxHipCmdSortSegmented[KeyValue] call, the same library
  loop        (c) one vrdxCmdSort[KeyValue] per segment, with offsets the HOST knows -- only where there are at most 64
              segments
  torch_sort  (d) a stable torch.sort of segment id << 32 | key packed into int64, and the gather of the values

Shapes: 'SxL' = S segments of L keys; 'mixed' = the log-uniform set of tools/segmented_bench.py; 'one_among' = one segment of
2^22 keys among 255 of 50000.  On every row the result of (a) must equal that of (b) bit for bit ("match"), on the timed
input and on one of another seed; the program exits with status 1 if any row does not.  The row also carries what the device
decided (vrdxHipReadBalancedSplit).

usage: python tools/segmented_balanced_bench.py [--shapes 65536x256,...] [--modes keys,kv] [--steps 7] [--warmup 2] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_SHAPES = ("65536x256,8192x2048,1024x16384,64x262144,4x4194304,mixed,1x16777216,256x65537,128x131072,64x196609,"
                  "one_among")
LOOP_UP_TO = 64


def segment_sizes(shape, rng):
    if shape == "mixed":   # (tools/segmented_bench.py: sizes log-uniform in [1, 100000], every 16th segment empty, 2^24 keys)
        sizes, total = [], 0
        while total < (1 << 24):
            s = 0 if len(sizes) % 16 == 15 else int(math.exp(rng.uniform(0.0, math.log(100000.0))))
            s = min(s, (1 << 24) - total) if total + s > (1 << 24) else s
            sizes.append(s)
            total += s
        return np.array(sizes, dtype=np.int64)
    if shape == "one_among":
        return np.array([50000] * 127 + [1 << 22] + [50000] * 128, dtype=np.int64)
    count, length = (int(x) for x in shape.split("x"))
    return np.full(count, length, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--modes", default="keys,kv")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import vulkan_radix_sort_amd as vrdx

    if not torch.cuda.is_available():
        sys.exit("segmented_balanced_bench.py needs a GPU (there is no CPU fallback)")
    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    stream = torch.cuda.current_stream().cuda_stream
    out = open(args.out, "a") if args.out else None
    all_match = True

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        result = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), result

    def random_words(n, seed):   # every bit random: 32-bit patterns held in int32
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        return torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32)

    for shape in args.shapes.split(","):
        sizes = segment_sizes(shape, np.random.default_rng(args.seed))
        host_offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n, segments = int(host_offsets[-1]), len(sizes)
        offsets = torch.from_numpy(host_offsets.astype(np.int32)).cuda()
        ids = torch.repeat_interleave(torch.arange(segments, dtype=torch.int64, device="cuda"),
                                      torch.from_numpy(sizes).cuda())
        master, payload = random_words(n, args.seed), random_words(n, args.seed + 7)
        for mode in args.modes.split(","):
            kv = mode == "kv"
            req = sorter.key_value_storage_requirements(n) if kv else sorter.storage_requirements(n)
            storage = torch.empty(req.size, dtype=torch.uint8, device="cuda")
            keys, values = torch.empty_like(master), torch.empty_like(payload) if kv else None

            def load(source):
                keys.copy_(source)
                if kv:
                    values.copy_(payload)

            def record(method):
                if kv:
                    getattr(sorter, method + "_key_value")(stream, n, segments, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                                           values.data_ptr(), 0, storage.data_ptr(), 0)
                else:
                    getattr(sorter, method)(stream, n, segments, offsets.data_ptr(), 0, keys.data_ptr(), 0, storage.data_ptr(), 0)

            def loop():
                for b, e in zip(host_offsets[:-1], host_offsets[1:]):
                    b, e = int(b), int(e)
                    if kv:
                        sorter.cmd_sort_key_value(stream, e - b, keys.data_ptr(), 4 * b, values.data_ptr(), 4 * b, storage.data_ptr(), 0)
                    else:
                        sorter.cmd_sort(stream, e - b, keys.data_ptr(), 4 * b, storage.data_ptr(), 0)

            def torch_sort():
                packed = (ids << 32) | (master.to(torch.int64) & 0xFFFFFFFF)
                ordered, index = torch.sort(packed, stable=True)
                return (ordered & 0xFFFFFFFF).to(torch.int32), (payload[index] if kv else None)

            ways = {"balanced": lambda: record("cmd_balanced_sort_segmented"), "segmented": lambda: record("cmd_sort_segmented"),
                    "torch_sort": torch_sort}
            if segments <= LOOP_UP_TO:
                ways["loop"] = loop
            times = {name: [] for name in ways}
            match = True
            for step in range(args.warmup + args.steps):
                results = {}
                for name, fn in ways.items():
                    load(master)
                    ms, _ = timed(fn)
                    if step >= args.warmup:
                        times[name].append(ms)
                    if step == 0 and name in ("balanced", "segmented"):
                        results[name] = (keys.clone(), values.clone() if kv else None)
                if step == 0:
                    a, b = results["balanced"], results["segmented"]
                    match = bool(torch.equal(a[0], b[0]) and (not kv or torch.equal(a[1], b[1])))
            # another input: (a) against (b), bit for bit
            extra = random_words(n, args.seed + 1000)
            load(extra)
            record("cmd_balanced_sort_segmented")
            split = sorter.read_balanced_split(stream, storage.data_ptr(), n)
            status = sorter.read_status(stream, storage.data_ptr(), 0)
            got = (keys.clone(), values.clone() if kv else None)
            load(extra)
            record("cmd_sort_segmented")
            torch.cuda.synchronize()
            match = match and bool(torch.equal(got[0], keys) and (not kv or torch.equal(got[1], values)))
            all_match = all_match and match
            info = sorter.describe_balanced_segmented_plan(n, segments, kv)
            result = {"shape": shape, "n": n, "segments": segments, "key_value": kv, "form": info.name, "launches": info.launches,
                      "listed": split.listedSegments, "spread": split.spreadSegments, "pieces": split.pieces,
                      "piece_keys": split.pieceKeys, "steps": args.steps}
            for name, xs in times.items():
                result[name + "_ms"] = float(np.median(xs))
                result[name + "_min_ms"] = float(np.min(xs))
                result[name + "_max_ms"] = float(np.max(xs))
            for name in times:
                if name != "balanced":
                    result[name + "_over_balanced"] = result[name + "_ms"] / result["balanced_ms"]
            result["balanced_minus_segmented_us"] = 1000.0 * (result["balanced_ms"] - result["segmented_ms"])
            result["status"] = status
            result["match"] = match
            line = json.dumps(result)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del storage, keys, values, extra, got
            torch.cuda.empty_cache()
        del master, payload, offsets, ids
    if out:
        out.close()
    sorter.destroy()
    sys.exit(0 if all_match else 1)


if __name__ == "__main__":
    main()
