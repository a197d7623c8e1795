"""GPU tests (-m gpu) of who owns the handles' memory (csrc/fdc_pipeline.hpp, csrc/fdc_faces.hip, csrc/fdc_buffers.hpp).

* Over the life of a handle — create, calls through the entries that allocate lazily, close — every hipMalloc has its hipFree and every hipHostMalloc its
  hipHostFree, exactly.  Counted by tests/cpp/hip_alloc_counter.c, loaded as tests/test_no_alloc_gpu.py loads it (ctypes, RTLD_GLOBAL, a fresh process,
  before the library); the shim does not count hipFree(NULL), so a zero-size hipMalloc that came back null would show as a malloc without a free.
* fdc_overlap_save keeps its history when its buffers grow: calls of 2, 5 and 3 items equal the CPU oracle's overlap_save over the 10 items, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import ctypes as C, sys
import numpy as np
shim = C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL)
sys.path.insert(0, sys.argv[2])
import gr_fdc_amd as G
from gr_fdc_amd import _lib
lib = G.lib()
hip = C.CDLL("libamdhip64.so")          # looked up in the runtime itself: the test's own device buffers are not counted

def counts():
    v = (C.c_long * 4)()
    shim.fdc_test_alloc_counts(v)
    return list(v)

def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)

def iq16(n, seed):
    return np.random.default_rng(seed).integers(-2000, 2000, size=2 * n, dtype=np.int16)

nb = 8

def small():
    N, R = 4096, 2
    H = N - N // R
    plan = [(301, 64, 0.6, 0.85), (0, 256, 0.8, 1.0), (1024 + 7, 512, 0.8, 0.95)]
    x = noise(nb * H, 3)
    p = G.Pipeline(N, R, plan, max_blocks=nb, keep_spectrum=True)
    assert p.path() == 5, p.describe()
    p.work(x)                                                   # unregistered outputs: d_ring, d_out, pin_out, pin_tab
    outs = [np.empty(nb * lo, np.complex64) for lo in p.lout]
    for o in outs:
        G.register_host(o)
    try:
        p.work(x, outs=outs)                                    # registered outputs: the scatter table
    finally:
        for o in outs:
            G.unregister_host(o)
    p.work_real(x.real.copy(), want_spectrum=True)              # d_real, d_specfull
    p.reset()                                                   # (the input form is latched: the integer call needs a reset, and so does the next float call)
    p.work_iq(iq16(nb * H, 4), scale=2.0 ** -11)                # d_iq
    p.reset()
    p.set_output_format("sc16", 1000.0)
    p.work(x)                                                   # d_oq
    p.set_output_format(None)
    p.set_fine_tuning([0.01, -0.02, 0.03])
    p.work(x)                                                   # d_fine, d_fstep, d_f4fine
    p.set_fine_tuning(None)
    p.enable_timing(True)
    p.work(x)                                                   # the events vector
    assert p.last_kernel_ms()[3] >= 1
    p.close()
    # the same real-input call on a handle WITHOUT keep_spectrum is refused before it allocates: nothing may be left behind either
    q = G.Pipeline(N, R, plan, max_blocks=nb)
    try:
        q.work_real(x.real.copy(), want_spectrum=True)
        raise AssertionError("a spectrum without keep_spectrum was not refused")
    except G.FdcError:
        pass
    q.close()

def large():
    N, R = 16384, 4
    H, ovl = N - N // R, N // R
    plan = [(256 * c, 256, 0.88, 1.0) for c in range(64)] + [(8192, 8192, 0.8, 1.0)]
    p = G.Pipeline(N, R, plan, max_blocks=nb)
    p.work(noise(nb * H, 5))
    n_out = p.output_samples(nb)
    ring = iq16(ovl + nb * H, 6)
    d_ring, d_out = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(ring.nbytes)) == 0 and hip.hipMalloc(C.byref(d_out), C.c_size_t(8 * n_out)) == 0
    try:
        assert hip.hipMemcpy(d_ring, C.c_void_p(ring.ctypes.data), C.c_size_t(ring.nbytes), 1) == 0
        p.process_device_iq("sc16", 2.0 ** -11, d_ring, 0, nb, d_out)       # a caller's ring: d_iqw where the plan widens
        p.synchronize()
    finally:
        hip.hipFree(d_ring); hip.hipFree(d_out)
    p.close()

def face(make, item_values, dtype):
    def run():
        b = make()
        for n in (2, 5, 3):                                     # grows once, then a call that fits
            b.work(np.arange(n * item_values, dtype=dtype))
        b.close()
    return run

handles = {
    "pipeline N = 4096": small,
    "pipeline N = 16384, split plan": large,
    "overlap_save": face(lambda: G.overlap_save(8, 4096, 2048), 2 * 2048, np.float32),
    "vector_cut": face(lambda: G.vector_cut_vxx(8, 4096, 2413, 256), 2 * 4096, np.float32),
    "phase_window": face(lambda: G.phase_shifting_windowing_vcc(256, 2, 1, 0.88, 1.0, 1), 256, np.complex64),
}
fin = noise(4 * 1024, 7)
G.fft_vcc(1024, True, True, fin)                                # fdc_fft_vcc's cache lives as long as the process: out of the picture
for run in handles.values():                                    # warm-up: the runtime's own first-use work
    run()
assert counts()[0] > 0                                          # the shim sees the library's allocations
bad = []
for name, run in handles.items():
    before = counts()
    run()
    d = [a - b for a, b in zip(counts(), before)]
    print(name, "hipMalloc %d hipFree %d hipHostMalloc %d hipHostFree %d" % tuple(d))
    if d[0] != d[1] or d[2] != d[3] or d[0] == 0:
        bad.append((name, d))
assert not bad, bad
print("OK")
'''


def test_allocations_balance_over_a_handles_life(tmp_path):
    shim = str(tmp_path / "libhipcount.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hip_alloc_counter.c"), "-o", shim,
                           "-ldl", "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([sys.executable, "-c", CHILD, shim, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


@pytest.mark.parametrize("outputlen,overlaplen", [(4096, 2048), (64, 0)])
@pytest.mark.parametrize("itemsize", [8, 4])
def test_overlap_save_keeps_its_history_across_a_grow(oracle, itemsize, outputlen, overlaplen):
    H = outputlen - overlaplen
    raw = np.random.default_rng(itemsize + outputlen).integers(0, 256, size=10 * H * itemsize, dtype=np.uint8)
    want = oracle.OverlapSave(itemsize, outputlen, overlaplen).work(raw)
    blk = G.overlap_save(itemsize, outputlen, overlaplen)
    got, at = [], 0
    for n in (2, 5, 3):                                          # the second call grows the buffers, the third fits the grown ones
        got.append(blk.work(raw[at * H * itemsize:(at + n) * H * itemsize]))
        at += n
    blk.close()
    got = np.concatenate(got)
    assert got.shape == want.shape and (got == want).all()
