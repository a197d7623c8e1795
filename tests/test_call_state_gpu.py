"""GPU tests (-m gpu): a call leaves nothing behind on the handle.  What an entry brings with it — waterfall rows, the spectrum staging it may write
without keep_spectrum, group powers — lives for that call only (csrc/fdc_pipeline.hpp, DeviceCall): the next call through ANOTHER entry on the same
handle computes what a fresh handle computes, is refused what a fresh handle is refused, and takes the kernels a fresh handle takes."""
import ctypes as C

import numpy as np
import pytest

import gr_fdc_amd as G
from test_parity_gpu import noise

pytestmark = pytest.mark.gpu
FORCED = any(G.defaults.get(k) for k in ("FDC_FORCE_GENERIC", "FDC_NO_POLY", "FDC_NO_BLOCK", "FDC_NO_FUSED"))


class Dev:
    """device buffers of one test, freed together"""
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.bufs = []

    def alloc(self, a):
        """a: an array to upload, or a byte count to zero"""
        n = a if isinstance(a, int) else a.nbytes
        d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d), C.c_size_t(max(1, n))) == 0
        self.bufs.append(d)
        if isinstance(a, int):
            assert self.hip.hipMemset(d, 0, C.c_size_t(n)) == 0
        else:
            assert self.hip.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(n), 1) == 0
        return d

    def fetch(self, d, n, dtype):
        a = np.empty(n, dtype)
        assert self.hip.hipMemcpy(C.c_void_p(a.ctypes.data), d, C.c_size_t(a.nbytes), 2) == 0
        return a

    def free(self):
        for d in self.bufs:
            self.hip.hipFree(d)


def test_waterfall_call_leaves_nothing_on_the_handle():
    """N = 4096, four 256-bin channels on the grid (path 5), keep_spectrum off: work_waterfall, then the other entries on the same handle"""
    N, R, nb = 4096, 2, 8
    H, ovl = N - N // R, N // R
    chans = [(256 * c, 256, 0.8, 1.0) for c in (1, 5, 9, 13)]
    x = noise(2 * nb * H, 31)
    a = G.Pipeline(N, R, chans, max_blocks=nb)
    b = G.Pipeline(N, R, chans, max_blocks=nb)
    assert FORCED or a.path() == 5, a.describe()
    a.work_waterfall(x[:nb * H], G.Waterfall(N, 1e6, R, 1, 0, -45.0, -20.0, 0, 0, max_items=nb))
    got = a.work(x[nb * H:])
    b.work(x[:nb * H])
    want = b.work(x[nb * H:])
    for c, (u, v) in enumerate(zip(got, want)):
        assert u.tobytes() == v.tobytes(), "ch%d: work() behind work_waterfall() differs from a fresh handle's" % c
    dev = Dev()
    try:
        ring, out, spec = dev.alloc(8 * (ovl + nb * H)), dev.alloc(8 * a.output_samples(nb)), dev.alloc(8 * nb * N)
        with pytest.raises(G.FdcError, match="spectrum output needs keep_spectrum"):      # the waterfall call's own spectrum staging was allowed
            a.process_device(ring, 0, nb, out, d_spectrum=spec)
        a.process_device_iq("sc16", 1.0, ring, 0, nb, out)                              # (a zeroed ring reads as sc16 zeros)
        a.synchronize()
        assert FORCED or "input sc16: fused" in a.describe(), a.describe()              # rows would send the call to the widened form
    finally:
        dev.free()


def test_group_power_call_leaves_nothing_on_the_handle():
    """N = 16384, a bank of 256-bin channels: process_device_power (spectrum + group powers), then process_device on the same handle"""
    N, R, nb = 16384, 2, 4
    H, ovl = N - N // R, N // R
    chans = [(256 * c, 256, 0.88, 1.0) for c in range(N // 256)]
    x = noise(ovl + 2 * nb * H, 32)
    a = G.Pipeline(N, R, chans, max_blocks=nb, keep_spectrum=True)
    b = G.Pipeline(N, R, chans, max_blocks=nb, keep_spectrum=True)
    n_out = a.output_samples(nb)
    dev = Dev()
    try:
        ring, spec, gpow = dev.alloc(x), dev.alloc(8 * nb * N), dev.alloc(4 * nb * N // 16)
        oa, ob = dev.alloc(8 * n_out), dev.alloc(8 * n_out)
        second = ring.value + 8 * nb * H
        a.process_device(ring, 0, nb, oa, d_spectrum=spec, d_group_power=gpow)
        a.process_device(second, nb, nb, oa)
        a.synchronize()
        b.process_device(second, nb, nb, ob)
        b.synchronize()
        assert a.describe() == b.describe()
        got, want = dev.fetch(oa, n_out, np.complex64), dev.fetch(ob, n_out, np.complex64)
    finally:
        dev.free()
    assert np.abs(want).max() > 0
    assert got.tobytes() == want.tobytes(), "process_device() behind process_device_power() differs from a fresh handle's"
