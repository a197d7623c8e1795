"""GPU test (-m gpu): no hipMalloc / hipFree / hipHostMalloc / hipHostFree in the steady state of the waterfall entries (fdc_waterfall_work,
fdc_pipeline_work_waterfall on the one-launch route, the group-sum route and the spectrum route).  The counting shim of test_no_alloc_gpu.py
(tests/cpp/hip_alloc_counter.c), loaded with RTLD_GLOBAL in a fresh process before the library; three warm-up calls, then fifty more of each."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import ctypes as C, sys
import numpy as np
shim = C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL)
sys.path.insert(0, sys.argv[2])
import gr_fdc_amd as G

def counts():
    v = (C.c_long * 4)()
    shim.fdc_test_alloc_counts(v)
    return list(v)

rng = np.random.default_rng(3)
def noise(n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)

entries = {}
w0 = G.Waterfall(4096, 1e6, 4, 3, 0, -45.0, -20.0, 0, 0, max_items=8)
pw = (np.abs(noise(7 * 4096)) ** 2).astype(np.float32)
entries["fdc_waterfall_work"] = lambda: w0.work(pw)
for name, N, R, plan, nb in (("one launch (N = 4096)", 4096, 4, [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0)], 8),
                             ("group sums (N = 65536)", 65536, 2, [(256 * c, 256, 0.88, 1.0) for c in (0, 5, 9)], 4),
                             ("spectrum (N = 8192)", 8192, 2, [(100, 256, 0.8, 1.0)], 4)):
    p = G.Pipeline(N, R, plan, max_blocks=nb)
    w = G.Waterfall(N, 1e6, R, 2, 0, -45.0, -20.0, 0, 0, max_items=nb)
    x = noise(nb * (N - N // R))
    entries["fdc_pipeline_work_waterfall, " + name] = (lambda p=p, w=w, x=x: p.work_waterfall(x, w))
bad = []
for name, call in entries.items():
    for _ in range(3):
        call()
    before = counts()
    for _ in range(50):
        call()
    after = counts()
    print(name, [a - b for a, b in zip(after, before)])
    if after != before:
        bad.append((name, [a - b for a, b in zip(after, before)]))
assert not bad, bad
print("OK")
'''


def test_no_allocation_in_the_steady_state_of_the_waterfall_entries(tmp_path):
    shim = str(tmp_path / "libhipcount.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hip_alloc_counter.c"), "-o", shim,
                           "-ldl", "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([sys.executable, "-c", CHILD, shim, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
