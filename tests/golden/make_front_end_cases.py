"""Records what the five torch front ends (sort_segments, sort64, sort_segments64, sort_bits, sort_segments_bits) make of their
arguments: which exception they raise, with its full message, or which recording call they make on the sorter, with every
argument.  Writes tests/golden/front_end_cases.json, which tests/test_front_end_cases.py replays against the working tree.

    python3 tests/golden/make_front_end_cases.py                  # both sections (the cuda one needs a GPU)
    python3 tests/golden/make_front_end_cases.py --section cpu    # one section, the other is kept from the file as it is
    python3 tests/golden/make_front_end_cases.py --root DIR       # ... of the package of another checkout

The sorter is a stub: its storage-requirement methods return REQUIRED bytes and note that they were asked, every ``cmd_*``
attribute notes the method's name and its arguments, addresses replaced by the names of the tensors they belong to.  Nothing
is launched, and no tensor has more than 16400 elements.

Per front end the cases are every valid combination of the optional arguments, and a list of faults -- an argument that is no
tensor, has the wrong dtype, two dimensions, a stride, another length, lives on the CPU, a bad bit range or order, a storage
that is too small or misaligned ... -- applied to the call with every optional argument given, one at a time and in all
pairs (the first of the pair first), so that the file pins WHICH refusal wins.  Every case is recorded in two sections: "cpu"
with every tensor on the CPU, "cuda" with every tensor on the GPU except where the fault says otherwise.

The file is never edited by hand: it was recorded from the package as it stood before the front ends' checks moved into
_checks.py, and this script reproduces it byte for byte from the package since.
"""
import argparse
import json
import os
import re
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "front_end_cases.json")
REQUIRED = 4096   # what the stub sorter asks for, whatever the count
SECTIONS = ("cpu", "cuda")

ORDERS = ((None, False), ("uint64", False), ("uint64", True), ("int64", False), ("int64", True), ("float64", False),
          ("float64", True))
RANGES = ((8, 24), (0, 32), (5, 5))

# name -> (the tensor arguments, the keys' dtype, the other arguments of the call that every fault is applied to)
FRONT_ENDS = {
    "sort_segments": (("keys", "offsets", "values", "storage"), "int32", {}),
    "sort64": (("keys", "values", "count", "storage"), "int64", {"order": "int64", "descending": False}),
    "sort_segments64": (("keys", "offsets", "values", "storage"), "int64", {"order": "int64", "descending": False}),
    "sort_bits": (("keys", "values", "count", "storage"), "int32", {"begin_bit": 8, "end_bit": 24}),
    "sort_segments_bits": (("keys", "offsets", "values", "storage"), "int32", {"begin_bit": 8, "end_bit": 24}),
}


class StubSorter:
    """What the front ends see of a Sorter; ``log`` is everything they did with it, in order."""

    def __init__(self):
        self.log = []

    def _required(self, text):
        self.log.append(text)
        return types.SimpleNamespace(size=REQUIRED)

    def storage_requirements(self, n):
        return self._required(f"storage_requirements({n})")

    def key_value_storage_requirements(self, n):
        return self._required(f"key_value_storage_requirements({n})")

    def storage_requirements64(self, n, key_value=False):
        return self._required(f"storage_requirements64({n}, key_value={key_value})")

    def __getattr__(self, name):
        if not name.startswith("cmd_"):
            raise AttributeError(name)
        return lambda *args, **kwargs: self.log.append((name, args, kwargs))


def _specs(arrays, key_dtype, device):
    """How each tensor argument of the faultless call is made."""
    specs = {"keys": dict(dtype=key_dtype, n=16), "offsets": dict(dtype="int32", n=3), "values": dict(dtype="int32", n=None),
             "count": dict(dtype="int32", n=1), "storage": dict(dtype="uint8", n=REQUIRED)}
    return {a: dict(specs[a], tensor=True, dims=1, step=1, misaligned=0, device=device) for a in arrays}


def _faults(arrays, key_dtype, scalars):
    """(name, argument or None for the other arguments, what to change)"""
    out = []
    for a in arrays:
        out.append((f"{a} not a tensor", a, {"tensor": False}))
        wrong = {"keys": "int64" if key_dtype == "int32" else "int32", "storage": "int32"}.get(a, "int64")
        out.append((f"{a} of the wrong dtype", a, {"dtype": wrong}))
        if a == "keys" and key_dtype == "int64":
            out.append(("keys of float64", a, {"dtype": "float64"}))
        if a not in ("count", "storage"):
            out.append((f"{a} two-dimensional", a, {"dims": 2}))
        if a != "count":
            out.append((f"{a} non-contiguous", a, {"step": 2}))
        if a == "values":
            out.append(("values of another length", a, {"n": 15}))
        if a == "count":
            out.append(("count of two elements", a, {"n": 2}))
        if a == "storage":
            out.append(("storage too small", a, {"n": REQUIRED - 16}))
            out.append(("storage misaligned by 4 bytes", a, {"misaligned": 4}))
        out.append((f"{a} on the CPU", a, {"device": "cpu"}))
    if "begin_bit" in scalars:
        out.append(("bit range of the wrong type", None, {"begin_bit": 8.0}))
        out.append(("bit range of the wrong value", None, {"begin_bit": 9, "end_bit": 8}))
        out.append(("more than 16384 keys with a partial range", "keys", {"n": 16400}))
    if "order" in scalars:
        out.append(("order of the wrong type", None, {"order": 2}))
        out.append(("order of the wrong value", None, {"order": "float32"}))
        out.append(("descending without an order", None, {"order": None, "descending": True}))
        out.append(("descending not a bool", None, {"descending": 1}))
    return out


def _make(torch, spec, keys_n):
    if not spec["tensor"]:
        return [1, 2, 3]
    n = keys_n if spec["n"] is None else spec["n"]
    base = torch.zeros(n * spec["step"] + 32, dtype=getattr(torch, spec["dtype"]), device=spec["device"])
    lead = ((spec["misaligned"] - base.data_ptr()) % 16) // base.element_size()
    t = base[lead:lead + n * spec["step"]:spec["step"]]
    return t.unsqueeze(0) if spec["dims"] == 2 else t


def _outcome(torch, front_end, specs, scalars, stream):
    """One call: everything the front end did with the sorter, then its exception or what it returned, as one line."""
    sorter = StubSorter()
    tensors = {a: _make(torch, spec, specs["keys"]["n"]) for a, spec in specs.items()}
    names = {t.data_ptr(): a for a, t in tensors.items() if isinstance(t, torch.Tensor)}
    if stream is not None:
        names[stream.cuda_stream] = "stream"
    try:
        returned = front_end(sorter, **tensors, **scalars)
    except Exception as e:   # noqa: BLE001 -- the refusal is the record
        sorter.log.append(f"{type(e).__name__}: {e}")
    else:
        if returned is tensors.get("storage"):
            sorter.log.append("returns storage")
        else:
            made = f"torch.empty({returned.numel()}, dtype={returned.dtype}, device={returned.device})"
            names[returned.data_ptr()] = made
            sorter.log.append(f"returns {made}")
    lines = []
    for entry in sorter.log:
        if isinstance(entry, tuple):
            name, args, kwargs = entry
            shown = [names.get(a, repr(a)) if isinstance(a, int) else repr(a) for a in args]
            shown += [f"{k}={names.get(v, repr(v)) if isinstance(v, int) else repr(v)}" for k, v in kwargs.items()]
            entry = f"{name}({', '.join(shown)})"
        lines.append(entry)
    return " | ".join(lines)


def _valid_calls(name, arrays, scalars):
    """(case name, the arguments left out, the other arguments) of every valid combination of the optional arguments"""
    optional = [a for a in arrays if a in ("values", "count", "storage")]
    for mask in range(1 << len(optional)):
        given = [a for i, a in enumerate(optional) if mask >> i & 1]
        absent = [a for a in optional if a not in given]
        label = " ".join(given) or "keys alone"
        if "order" in scalars:
            for order, descending in ORDERS:
                for key_dtype in (("int64", "float64") if order == "float64" else ("int64",)):
                    yield (f"{label}, {key_dtype} keys, order={order!r}, descending={descending}", absent,
                           {"order": order, "descending": descending}, {"dtype": key_dtype})
        elif "begin_bit" in scalars:
            for begin, end in RANGES:
                yield f"{label}, [{begin}, {end})", absent, {"begin_bit": begin, "end_bit": end}, {}
            if name == "sort_segments_bits" or not given:
                yield f"{label}, 16400 keys, [0, 32)", absent, {"begin_bit": 0, "end_bit": 32}, {"n": 16400}
                yield f"{label}, 16400 keys, [7, 7)", absent, {"begin_bit": 7, "end_bit": 7}, {"n": 16400}
            if name == "sort_segments_bits":
                yield f"{label}, 16400 keys, [8, 24)", absent, {"begin_bit": 8, "end_bit": 24}, {"n": 16400}
        else:
            yield label, absent, {}, {}


def cases(torch, package, section, name):
    """case name -> outcome, for one front end, in the file's order: the valid calls, each fault alone, each pair."""
    arrays, key_dtype, scalars = FRONT_ENDS[name]
    front_end = getattr(package, name)
    device = "cpu" if section == "cpu" else "cuda"
    stream = None if section == "cpu" else torch.cuda.Stream()
    out = {}

    def run(specs, others):
        if stream is None:
            return _outcome(torch, front_end, specs, others, None)
        with torch.cuda.stream(stream):
            return _outcome(torch, front_end, specs, others, stream)

    for label, absent, others, keys_edit in _valid_calls(name, arrays, scalars):
        specs = _specs(arrays, key_dtype, device)
        specs["keys"].update(keys_edit)
        for a in absent:
            del specs[a]
        out[f"valid: {label}"] = run(specs, dict(scalars, **others))
    faults = _faults(arrays, key_dtype, scalars)
    for i, first in enumerate(faults):
        for second in [None] + faults[i + 1:]:
            specs, others = _specs(arrays, key_dtype, device), dict(scalars)
            for fault in (first, second):
                if fault is not None:
                    (others if fault[1] is None else specs[fault[1]]).update(fault[2])
            out[first[0] if second is None else f"{first[0]} + {second[0]}"] = run(specs, others)
    assert list(out) == case_names(name), name
    return out


def case_lists(name):
    """(the valid calls, the faults) of one front end by name, as the file lists them"""
    arrays, key_dtype, scalars = FRONT_ENDS[name]
    return {"valid": [call[0] for call in _valid_calls(name, arrays, scalars)],
            "faults": [fault[0] for fault in _faults(arrays, key_dtype, scalars)]}


def case_names(name):
    """The cases of one front end in the file's order: the valid calls, then each fault alone followed by its pairs."""
    lists = case_lists(name)
    names = [f"valid: {label}" for label in lists["valid"]]
    for i, first in enumerate(lists["faults"]):
        names += [first] + [f"{first} + {second}" for second in lists["faults"][i + 1:]]
    return names


def pack(recorded):
    """{case: outcome} as the file holds it: every distinct outcome once, the cases (in case_names' order) as indices."""
    outcomes = list(dict.fromkeys(recorded.values()))
    return {"outcomes": outcomes, "outcome_of_case": [outcomes.index(o) for o in recorded.values()]}


def unpack(name, packed):
    names = case_names(name)
    assert len(names) == len(packed["outcome_of_case"]), name
    return {case: packed["outcomes"][i] for case, i in zip(names, packed["outcome_of_case"])}


def render(fixture):
    """The file's text: one line per outcome and per case name, the index lists on one line each."""
    text = json.dumps(fixture, indent=1)
    return re.sub(r"\[\s+((?:\d+,\s+)*\d+)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text) + "\n"


def record(torch, package, sections, kept=None):
    """The whole file: the cases' names (from this script alone), then per section and front end what was recorded."""
    fixture = {"cases": {name: case_lists(name) for name in FRONT_ENDS}}
    for section in SECTIONS:
        if section in sections:
            fixture[section] = {name: pack(cases(torch, package, section, name)) for name in FRONT_ENDS}
        else:
            fixture[section] = kept[section]
    return fixture


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--section", choices=SECTIONS, help="record this section only and keep the other from the file")
    parser.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)), help="the checkout whose package is recorded")
    parser.add_argument("--output", default=FIXTURE)
    args = parser.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import vulkan_radix_sort_amd as package
    assert os.path.dirname(os.path.dirname(os.path.abspath(package.__file__))) == os.path.abspath(args.root), package.__file__
    sections = SECTIONS if args.section is None else (args.section,)
    kept = {section: {} for section in SECTIONS}   # (the first recording: the other section follows)
    if args.section is not None and os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            kept = json.load(f)
    text = render(record(torch, package, sections, kept))
    with open(args.output, "w") as f:
        f.write(text)
    print(f"{args.output}: {len(text)} bytes")


if __name__ == "__main__":
    main()
