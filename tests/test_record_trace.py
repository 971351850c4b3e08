"""Without a GPU: what the host recorder (vulkan_radix_sort_amd/csrc/vrdx_api.cpp) enqueues for every vrdxCmd* / vrdxHipCmd*
entry point -- launches with their grids, fills, copies, event records, the status bits and each timestamp slot's source --
over the matrix of tests/native/record_trace.cpp, held byte for byte to tests/golden/record_trace.txt.  The golden file was
written by this program from the recorder as it stood before its segmented and 64-bit parts became step lists; a change of
the recorder that is meant to move a launch regenerates it (`tests/native/record_trace 8 256`) and shows the move in review."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
GOLDEN = os.path.join(ROOT, "tests", "golden", "record_trace.txt")


def test_every_entry_point_records_what_the_golden_trace_holds():
    subprocess.run(["make", "-C", NATIVE, "record_trace"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(NATIVE, "record_trace"), "8", "256"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = open(GOLDEN, "rb").read()
    if r.stdout != want:
        got_lines, want_lines = r.stdout.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got_lines, want_lines)) if a != b), min(len(got_lines), len(want_lines)))
        raise AssertionError("line %d: recorded %r, the golden trace holds %r (%d lines against %d)" % (
            first + 1, got_lines[first:first + 1], want_lines[first:first + 1], len(got_lines), len(want_lines)))
