"""GPU tests (-m gpu): every entry of the library inside guard bands around the memory the LIBRARY allocates (tests/cpp/hip_guard_alloc.c; the shim itself
is proved on the CPU by tests/test_guard_alloc_cpu.py).

tests/test_footprint_gpu.py bands the buffers a caller hands in; this file bands the handles' own: every hipMalloc and every plain hipHostMalloc of the
library becomes [guard | payload | guard], all of it poisoned, and after every call of every scenario of tests/guard_scenarios.py (and again after the
handles are closed, each freed block being looked at in its hipFree) no guard byte may have changed.  A kernel that stores one row past an internal
buffer is then a failed assertion with the buffer's size, the ordinal of its allocation and the offset, not a store into a neighbouring allocation.

Each test runs some scenarios in two fresh child processes, one after the other: plain, and with the shim loaded (ctypes, RTLD_GLOBAL) before the
library, under poison 0xFF and then under 0x00.  The parent asserts
* the binding: the shim has banded allocations after the first call, and a buffer the child takes from the shim's hipMalloc and hits one byte behind
  its payload with the runtime's own hipMemset is reported at offset n with a count of 1;
* the guards: the child's assertions held (its exit status);
* the bytes: every describe() string and every output of every scenario is byte-equal (a digest) between the plain child and both guarded passes.  The
  payloads are poisoned too, so an internal buffer read before it was written, or a read past an internal buffer that reaches an output, fails here.

A child that ends by a signal, at its time limit or with an illegal-address text fails its test with its output, and every later test of the file
skips: nothing more is started on the device.

MEASURED on one MI355X, each test with both its children: routes 0-19 7.1 s, routes 19-42 6.5 s, fused 3.1 s, tail 0-12 7.3 s, tail 12-24
7.7 s, tail 24-31 4.1 s, tail 31-36 7.7 s, around 2.8 s; the file 47 s.  Of a test's time about a third is the plain child's and two thirds the guarded
child's (two passes, and every check copies all guards home); about 1 s of each child is its start (interpreter, runtime, first handle).  The time limits
in PARTS are about five times a child's share, and never below 15 s, so that a loaded machine's slow start is not taken for a hang.  routes and tail
went over ten seconds as one test each (12 s and 20 s) and were split by scenario; nothing was thinned."""
import json
import subprocess
import sys

import pytest

import guard_alloc as GA

pytestmark = pytest.mark.gpu
CHILD = GA.ROOT + "/tests/guard_scenarios.py"

# (group, first scenario, last + 1, time limit of the plain child, time limit of the guarded child)
PARTS = [
    ("routes", 0, 19, 20, 40),
    ("routes", 19, 42, 20, 40),
    ("fused", 0, 34, 15, 20),
    ("tail", 0, 12, 15, 30),
    ("tail", 12, 24, 15, 30),
    ("tail", 24, 31, 15, 30),
    ("tail", 31, 36, 15, 30),
    ("around", 0, 6, 15, 20),
]
TROUBLE = []            # why nothing more is started on the device


def child(args, limit):
    """one child at a time; returns its result line"""
    if TROUBLE:
        pytest.skip("an earlier child of this file ended in trouble, nothing more is started on the device: " + TROUBLE[0])
    cmd = [sys.executable, CHILD] + [str(a) for a in args]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        TROUBLE.append("%r did not end within %d s" % (args, limit))
        pytest.fail("%s\n%s\n%s" % (TROUBLE[0], e.stdout, e.stderr))
    text = r.stdout + r.stderr
    if r.returncode < 0 or "illegal memory access" in text or "illegal address" in text.lower():
        TROUBLE.append("%r ended with status %d" % (args, r.returncode))
        pytest.fail("%s\n%s" % (TROUBLE[0], text))
    assert r.returncode == 0, text[-6000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, text[-6000:]
    res = json.loads(lines[0][len("RESULT "):])
    assert "errors" not in res, res["errors"]
    return res


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return GA.build_shim(str(tmp_path_factory.mktemp("guard") / "libhipguard.so"))


@pytest.mark.parametrize("group,lo,hi,t_plain,t_guarded", PARTS, ids=["%s %d-%d" % p[:3] for p in PARTS])
def test_inside_guard_bands(shim, group, lo, hi, t_plain, t_guarded):
    plain = child([group, lo, hi], t_plain)
    guarded = child([group, lo, hi, shim], t_guarded)
    # the binding
    assert guarded["banded after the first call"] > 0, "the shim saw none of the library's allocations"
    banded, freed = guarded["counts"]
    assert banded > 2 and 0 < freed <= banded, (banded, freed)
    for byte in GA.POISONS:
        b = guarded["binding 0x%02X" % byte]
        assert (b["total"], b["payload"], b["first"], b["last"], b["count"], b["clean"]) == (1, 1000, 1000, 1000, 1, 0), b
    # the bytes (the guards: the guarded child's exit status, asserted in child())
    want = plain["plain"]
    assert len(want) > 0
    for byte in GA.POISONS:
        got = guarded["0x%02X" % byte]
        assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
        differ = [k for k in sorted(want) if got[k] != want[k]]
        assert not differ, "under poison 0x%02X %d of %d outputs differ from the plain child's: %s" % (byte, len(differ), len(want), differ[:20])
