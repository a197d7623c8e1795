"""GPU tests (-m gpu) of the stage-1 tables of the one-block-per-CU kernel for banks of 256-bin channels (fdc_block256.hip: the W_256 twiddle rows, the
inter-pass twiddles with the window, the per-column constants), one case per kernel form and block length.

Every case runs a uniform bank (every slot of the band) through Pipeline.process_device on nb = 2 * (compute units) + 3 blocks.  With one
workgroup per compute unit (every form but the two below) the persistent workgroups run two and three blocks each and the last round is ragged;
N = 16384 on the grid and half a slot up at R = 2 launches two workgroups per compute unit: three of them run a second block, the others one.
Either way whatever a pass fetches ahead wraps into a workgroup's next block, and the blocks behind the wrap are among the checked ones.  Checked against
the oracle with the tolerance of tests/test_parity_gpu.py (relative L2 <= 1e-5 and max-abs / max <= 1e-5): blocks 0 and 1, the two on either side
of every multiple of the compute-unit count (the grid is one or two workgroups per compute unit), and the last; all channels at N = 16384, every
16th and the last above.  Every output sample depends on all passes, all eight waves and all four column roles of its block: a wrong row, a wrong
index or a wrong fold shows.  A single table entry that is slightly off (1e-5 rad) does NOT show at 1e-5 on noise (tests/test_fft_model_cpu.py);
tests/test_block_accuracy_gpu.py holds the forward form of this kernel, which shares these tables, to float32-grade error on impulses, and says what
is still missing for the channelizing forms.

sc16 in and out: the float output on sc16 input against the oracle (on the widened samples), and the sc16 output byte for byte against the output
contract (tests/test_iq_output_gpu.py: saturate(rint(y * scale))) applied to that float output."""
import ctypes as C

import numpy as np
import pytest

import gr_fdc_amd as G

pytestmark = pytest.mark.gpu
TOL = 1e-5
FORCED = any(G.defaults.get(k) for k in ("FDC_FORCE_GENERIC", "FDC_NO_POLY", "FDC_NO_BLOCK"))
IN_SCALE, OUT_SCALE = 2.0 ** -10, 200.0

_hip = None
_noise = {}


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    return _hip


def noise(n):
    """the first n samples of one seeded complex64 stream (made once for the longest ring)"""
    if "x" not in _noise or _noise["x"].size < n:
        rng = np.random.default_rng(20256)
        m = max(n, 16384 + 600 * 49152)
        _noise["x"] = (rng.standard_normal(m, dtype=np.float32) + 1j * rng.standard_normal(m, dtype=np.float32)).astype(np.complex64)
    return _noise["x"][:n]


def noise_sc16(n):
    if "i" not in _noise or _noise["i"].size < 2 * n:
        rng = np.random.default_rng(20257)
        _noise["i"] = rng.integers(-32768, 32768, size=2 * max(n, 32768 + 600 * 32768), dtype=np.int16)
    return _noise["i"][:2 * n]


class Dev:
    """a device buffer that frees itself"""

    def __init__(self, nbytes, src=None):
        self.p = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.p), C.c_size_t(max(1, nbytes))) == 0
        if src is not None:
            assert hip().hipMemcpy(self.p, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), 1) == 0

    def back(self, byte_off, a):
        assert hip().hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(self.p.value + byte_off), C.c_size_t(a.nbytes), 2) == 0
        return a

    def __del__(self):
        if self.p:
            hip().hipFree(self.p)
            self.p = C.c_void_p()


def rel(a, b):
    a = a.astype(np.complex128); b = b.astype(np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(np.abs(a - b).max() / np.abs(b).max())


def assert_close(a, b, what):
    assert a.shape == b.shape, what
    l2, mx = rel(a, b)
    assert l2 <= TOL and mx <= TOL, "%s: l2=%.3g max=%.3g" % (what, l2, mx)


def spans_of(nb, ncu):
    """runs of consecutive checked blocks: 0, 1, both sides of every multiple of ncu below nb, and the last"""
    want = {0, 1, nb - 1}
    for g in range(ncu, nb, ncu):
        want |= {g - 1, g}
    want = sorted(want)
    runs, a = [], want[0]
    for u, v in zip(want, want[1:] + [None]):
        if v != u + 1:
            runs.append((a, u + 1 - a))
            a = v
    return runs


def model(y, scale, dtype):
    info = np.iinfo(dtype)
    t = np.rint(np.ascontiguousarray(y, np.complex64).view(np.float32) * np.float32(scale))
    return np.clip(t, info.min, info.max).astype(dtype).reshape(-1, 2)


FORMS = {
    # name: (R, offset r, first_block, keep_spectrum)
    "grid": (2, 0, 0, False),
    "offset37": (2, 37, 13, False),          # odd r at an odd first block: the per-block sign, the rotated exchange and the second twiddle row
    "half": (2, 128, 0, False),
    "r4": (4, 0, 0, False),
    "spectrum": (2, 0, 0, True),             # keep_spectrum: the kernel as the forward transform of the block
}
CASES = [(N, f) for N in (16384, 32768, 65536) for f in FORMS] + [(65536, "sc16")]


@pytest.mark.parametrize("N,form", CASES, ids=["N%d-%s" % c for c in CASES])
def test_every_form_against_the_oracle(oracle, N, form):
    if FORCED:
        pytest.skip("suite run under a forced path")
    sc16 = form == "sc16"
    R, r, first, keep = FORMS["grid" if sc16 else form]
    nslots = N // 256 - (1 if r else 0)
    chans = [(256 * c + r, 256, 0.88, 1.0) for c in range(nslots)]
    ovl, H = N // R, N - N // R
    probe = G.Pipeline(N, R, chans, windowtype=1, max_blocks=1, keep_spectrum=keep)
    ncu = probe.reserve_compute_units(0)
    probe.close()
    nb = 2 * ncu + 3
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, keep_spectrum=keep)
    assert p.path() == 3, p.describe()          # (a call that hands out its spectrum runs the forward-transform form and the channel kernels)
    lout = p.lout[0]
    assert all(lo == lout for lo in p.lout)
    n_out = p.output_samples(nb)
    if sc16:
        raw = noise_sc16(ovl + nb * H)
        ring = (raw.astype(np.float32) * np.float32(IN_SCALE)).view(np.complex64)
        d_ring = Dev(raw.nbytes, raw)
    else:
        ring = noise(ovl + nb * H)
        d_ring = Dev(ring.nbytes, ring)
    d_out = Dev(n_out * 8)
    d_spec = Dev(nb * N * 8) if keep else None
    if sc16:
        p.process_device_iq("sc16", IN_SCALE, d_ring.p, first, nb, d_out.p)
    else:
        p.process_device(d_ring.p, first, nb, d_out.p, d_spec.p if keep else None)
    p.synchronize()
    if sc16:
        d_nar = Dev(n_out * 4)
        p.set_output_format("sc16", OUT_SCALE)
        p.process_device_iq("sc16", IN_SCALE, d_ring.p, first, nb, d_nar.p)
        p.synchronize()
        d = p.describe()                          # the integer instantiations of the kernel, not a widened copy in front or a narrowing pass behind
        assert "input sc16: fused" in d and "output " in d and ": fused" in d.split("output ")[1], d
    which = list(range(nslots)) if N == 16384 else sorted(set(range(0, nslots, 16)) | {nslots - 1})
    sub = [chans[c] for c in which]
    for t0, k in spans_of(nb, ncu):
        ref, rspec = oracle.channelizer(N, R, 1, sub, ring[ovl + t0 * H:ovl + (t0 + k) * H], prefix=ring[t0 * H:t0 * H + ovl],
                                        first_block=first + t0, want_spectrum=keep, nthreads=8)
        for c, want in zip(which, ref):
            off = p.channel_offset(c, nb) + t0 * lout
            got = d_out.back(off * 8, np.empty(k * lout, np.complex64))
            assert_close(got, want, "N=%d %s blocks %d..%d channel %d" % (N, form, t0, t0 + k - 1, c))
            if sc16:
                nar = d_nar.back(off * 4, np.empty((k * lout, 2), np.int16))
                assert nar.tobytes() == model(got, OUT_SCALE, np.int16).tobytes(), "sc16 out, blocks %d.. channel %d" % (t0, c)
        if keep:
            got = d_spec.back(t0 * N * 8, np.empty(k * N, np.complex64))
            assert_close(got, rspec, "N=%d spectrum of blocks %d..%d" % (N, t0, t0 + k - 1))
    p.close()
