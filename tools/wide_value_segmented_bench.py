#!/usr/bin/env python3
"""Times the segmented sort of 32-bit keys with 64-bit values (vrdxHipCmdWideValueSortSegmented) on one GPU against what a
caller had before it, on the project's four shapes of 16.8 M elements per call:

  call        (a) one vrdxHipCmdWideValueSortSegmented
  workaround  (b) torch.arange, vrdxHipCmdSortSegmentedKeyValue on (keys, index), values[index] -- three launches and a
              temporary of the caller's
  floor       (c) one vrdxHipCmdSortSegmentedKeyValue alone, with 4-byte values: by bytes the call would cost 1.5 x this in
              the in-LDS classes

The variants take turns in one process, step by step, each between one pair of events, every one on a fresh copy of the same
uniform keys; times are medians over --steps.  Each shape prints ONE JSON line; the call's result of the last step is compared
with the workaround's and with a stable torch.sort per row.

usage: python tools/wide_value_segmented_bench.py [--shapes 65536x256,...] [--steps 21] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = "65536x256,8192x2048,1024x16384,64x262144"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vulkan_radix_sort_amd as vrdx

    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    stream = torch.cuda.current_stream().cuda_stream
    out = open(args.out, "a") if args.out else None
    for shape in args.shapes.split(","):
        segments, length = (int(x) for x in shape.split("x"))
        n = segments * length
        gen = torch.Generator(device="cuda")
        source_keys = torch.empty(n, dtype=torch.int32, device="cuda")
        source_values = torch.empty(n, dtype=torch.int64, device="cuda")
        keys, values = torch.empty_like(source_keys), torch.empty_like(source_values)
        values32 = torch.empty(n, dtype=torch.int32, device="cuda")
        offsets = torch.arange(0, n + 1, length, dtype=torch.int32, device="cuda")
        storage = torch.empty(sorter.wide_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
        assert storage.numel() >= sorter.key_value_storage_requirements(n).size
        result = {}

        def fresh(step):
            gen.manual_seed(args.seed * 1000003 + step)
            source_keys.copy_(torch.randint(-2**31, 2**31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32))
            source_values.copy_(torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device="cuda", generator=gen))

        def call():
            sorter.cmd_wide_value_sort_segmented(stream, n, segments, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                                 values.data_ptr(), 0, storage.data_ptr(), 0)
            result["call"] = (keys, values)

        def workaround():
            index = torch.arange(n, dtype=torch.int32, device="cuda")
            sorter.cmd_sort_segmented_key_value(stream, n, segments, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                                index.data_ptr(), 0, storage.data_ptr(), 0)
            result["workaround"] = (keys, values[index])

        def floor():
            sorter.cmd_sort_segmented_key_value(stream, n, segments, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                                values32.data_ptr(), 0, storage.data_ptr(), 0)

        ways = {"call": call, "workaround": workaround, "floor": floor}
        times = {name: [] for name in ways}
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for step in range(args.warmup + args.steps):
            fresh(step)
            for name, run in ways.items():
                keys.copy_(source_keys)
                values.copy_(source_values)
                begin.record()
                run()
                end.record()
                end.synchronize()
                if step >= args.warmup:
                    times[name].append(begin.elapsed_time(end))
        # the last step's results: the call against the workaround and against torch, row by row
        as_unsigned = (source_keys.to(torch.int64) & 0xFFFFFFFF).reshape(segments, length)
        want_keys, index = torch.sort(as_unsigned, dim=1, stable=True)
        want_values = torch.gather(source_values.reshape(segments, length), 1, index)
        match = True
        for name in ("call", "workaround"):
            keys.copy_(source_keys)
            values.copy_(source_values)
            ways[name]()
            got_keys, got_values = result[name]
            match = match and torch.equal(got_keys.to(torch.int64).reshape(segments, length) & 0xFFFFFFFF, want_keys)
            match = match and torch.equal(got_values.reshape(segments, length), want_values)
        del as_unsigned, want_keys, want_values, index
        line = {"shape": shape, "n": n, "steps": args.steps}
        line.update({f"{name}_ms": round(statistics.median(t), 6) for name, t in times.items()})
        line["workaround_over_call"] = round(line["workaround_ms"] / line["call_ms"], 4)
        line["call_over_floor"] = round(line["call_ms"] / line["floor_ms"], 4)
        line["status"] = sorter.read_sorter_status(stream)
        line["match"] = bool(match)
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        result.clear()
        del storage, keys, values, values32, source_keys, source_values
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
