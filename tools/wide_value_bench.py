#!/usr/bin/env python3
"""Times the sort of 32-bit keys with 64-bit values (vrdxHipCmdWideValueSort) on one GPU against what a caller had before it:

  call        (a) one vrdxHipCmdWideValueSort
  workaround  (b) torch.arange, vrdxCmdSortKeyValue on (keys, index), values[index] -- the same work in more launches, with a
              temporary of the caller's
  torch_sort  (c) a stable torch.sort of the keys as int64, plus the gather of the values by its indices
  floor       (d) one vrdxCmdSortKeyValue of n alone: what any composition around one inner sort cannot beat

The variants take turns in one process, step by step, each between one pair of events, every one on a fresh copy of the same
uniform keys; times are medians over --steps.  Each shape prints ONE JSON line; the call's result of the last step is compared
with torch's.

--libraries name=path[,name=path...] adds, as further variants that take their turn with the others, the same call through
other BUILDS of the library (tools/build_variants.sh, e.g. gather:-DVRDX_WIDE_VALUE_TWO_SORTS_FROM=0xFFFFFFFFu and
two_sorts:-DVRDX_WIDE_VALUE_TWO_SORTS_FROM=0u): how kWideValueTwoSortsFrom (vrdx_plan.h) is measured.

usage: python tools/wide_value_bench.py [--sizes 1024,4096,...] [--steps 21] [--warmup 3] [--libraries ...] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = "1024,4096,8192,16384,65536,262144,1048576,4194304,16777216,33554432"


def sorter_of(path):
    """A Sorter on another build of the library (the binding caches ONE library: it is swapped while this sorter is made)."""
    from vulkan_radix_sort_amd import api
    own, api._LIB = api._LIB, None
    os.environ["VRDX_LIBRARY"] = path
    try:
        return api.Sorter(0)
    finally:
        del os.environ["VRDX_LIBRARY"]
        api._LIB = own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--libraries", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import vulkan_radix_sort_amd as vrdx

    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    others = {name: sorter_of(path) for name, path in (item.split("=", 1) for item in args.libraries.split(",") if item)}
    stream = torch.cuda.current_stream().cuda_stream
    out = open(args.out, "a") if args.out else None
    for n in (int(x) for x in args.sizes.split(",")):
        gen = torch.Generator(device="cuda")
        source_keys = torch.empty(n, dtype=torch.int32, device="cuda")
        source_values = torch.empty(n, dtype=torch.int64, device="cuda")
        keys, values = torch.empty_like(source_keys), torch.empty_like(source_values)
        storage = torch.empty(sorter.wide_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
        result = {}

        def fresh(step):
            gen.manual_seed(args.seed * 1000003 + step)
            source_keys.copy_(torch.randint(-2**31, 2**31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32))
            source_values.copy_(torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device="cuda", generator=gen))

        def call_of(s):
            def run():
                s.cmd_wide_value_sort(stream, n, keys.data_ptr(), 0, values.data_ptr(), 0, storage.data_ptr(), 0)
                result["call"] = (keys, values)
            return run

        def workaround():
            index = torch.arange(n, dtype=torch.int32, device="cuda")
            sorter.cmd_sort_key_value(stream, n, keys.data_ptr(), 0, index.data_ptr(), 0, storage.data_ptr(), 0)
            result["workaround"] = (keys, values[index])

        def torch_sort():
            sorted_keys, index = torch.sort(keys.to(torch.int64) & 0xFFFFFFFF, stable=True)
            result["torch_sort"] = (sorted_keys, values[index])

        def floor():
            sorter.cmd_sort_key_value(stream, n, keys.data_ptr(), 0, values.data_ptr(), 0, storage.data_ptr(), 0)

        ways = {"call": call_of(sorter), "workaround": workaround, "torch_sort": torch_sort, "floor": floor}
        ways.update({name: call_of(s) for name, s in others.items()})
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
        # the last step's results: the call, every other build's and the workaround against torch's
        want_keys, want_values = result["torch_sort"]
        match = True
        for name in ["call", "workaround"] + list(others):
            keys.copy_(source_keys)
            values.copy_(source_values)
            ways[name]()
            got_keys, got_values = result["workaround" if name == "workaround" else "call"]
            match = match and torch.equal(got_keys.to(torch.int64) & 0xFFFFFFFF, want_keys) and torch.equal(got_values, want_values)
        info = sorter.describe_wide_value_sort_plan(n)
        line = {"n": n, "form": info.name, "launches": int(info.launches), "bytes_per_element": int(info.bytesPerElement),
                "steps": args.steps}
        line.update({f"{name}_ms": round(statistics.median(t), 6) for name, t in times.items()})
        line["workaround_over_call"] = round(line["workaround_ms"] / line["call_ms"], 4)
        line["torch_over_call"] = round(line["torch_sort_ms"] / line["call_ms"], 4)
        line["call_over_floor"] = round(line["call_ms"] / line["floor_ms"], 4)
        line["status"] = sorter.read_sorter_status(stream) | max([s.read_sorter_status(stream) for s in others.values()] or [0])
        line["match"] = bool(match)
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        del storage, keys, values, source_keys, source_values
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
