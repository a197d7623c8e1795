"""GPU tests (-m gpu) of the stage-1 table scheme SROW of the one-block-per-CU kernel for banks of 256-bin channels (fdc_block256.hip, kBlkSrow): the
wave's twiddle row W_N^(16 q (32 pass + 4 wave)) read from memory through the scalar path in four pieces per pass (the half-slot form: with its two
halves swapped), and cb as ONE entry of the table cbt[32 pass + 4 wave][b] in LDS.

Every case runs a uniform bank (every slot of the band) of seeded noise through Pipeline.process_device at three block counts through one handle and
one ring: nb = 1 (the last pass fetches "the same rows again, unused"), nb = (compute units) + 1 and nb = 2 * (compute units) + 3 (workgroups run two
and three blocks, the last round is ragged, what the last pass fetches ahead wraps into the workgroup's next block).  A block's output does not depend
on how many blocks the call has, so the oracle is computed once per case, for the blocks checked at the largest count: 0, 1, both sides of every
multiple of the compute-unit count, and the last; the smaller counts are held to the same reference.  Tolerance of
tests/test_block256_stage1_tables_gpu.py: relative L2 <= 1e-5 and max-abs / max <= 1e-5, per run of blocks and channel; every 16th channel and the
last.  Every output sample depends on all passes, all eight waves and all sixteen entries of each wave row of its block: a wrong piece, a piece used
before it arrived or a wrong cb row shows.  One entry that is slightly off (1e-5 rad) does NOT show at 1e-5 on noise (tests/test_fft_model_cpu.py):
see tests/test_block_accuracy_gpu.py for what is held to float32-grade error and what is not yet.

Forms at N = 32768 (P = 4) and N = 65536 (P = 8): grid, half (half a slot up, first_block = 13) and sc16 (complex int16 input: the float output
against the oracle on the widened samples, and the sc16 output byte for byte against the output contract, saturate(rint(y * scale)), applied to that
float output — the integer-output forms take the scheme with their float form, or the two would round apart).  Which forms take the scheme is the
kernel's business (kBlkSrow): all of these at N = 65536, none at N = 32768, whose forms keep the row table UR in LDS and the two-factor cb.
offset37 at N = 65536 (odd offset at an odd first block) is a form the scheme leaves alone whatever the block length: it must give the answer it
gave."""
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
        rng = np.random.default_rng(20260)
        m = max(n, 32768 + 520 * 32768)
        _noise["x"] = (rng.standard_normal(m, dtype=np.float32) + 1j * rng.standard_normal(m, dtype=np.float32)).astype(np.complex64)
    return _noise["x"][:n]


def noise_sc16(n):
    if "i" not in _noise or _noise["i"].size < 2 * n:
        rng = np.random.default_rng(20261)
        _noise["i"] = rng.integers(-32768, 32768, size=2 * max(n, 32768 + 520 * 32768), dtype=np.int16)
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


def model(y, scale, dtype):
    """the output contract of tests/test_iq_output_gpu.py: saturate(rint(y * scale))"""
    info = np.iinfo(dtype)
    t = np.rint(np.ascontiguousarray(y, np.complex64).view(np.float32) * np.float32(scale))
    return np.clip(t, info.min, info.max).astype(dtype).reshape(-1, 2)


def spans_of(nb, ncu):
    """runs of consecutive checked blocks: 0, 1, both sides of every multiple of ncu below nb, and the last"""
    want = {0, nb - 1} | ({1} if nb > 1 else set())
    for g in range(ncu, nb, ncu):
        want |= {g - 1, g}
    want = sorted(want)
    runs, a = [], want[0]
    for u, v in zip(want, want[1:] + [None]):
        if v != u + 1:
            runs.append((a, u + 1 - a))
            a = v
    return runs


FORMS = {
    # name: (offset r, first_block, sc16 input)
    "grid": (0, 0, False),
    "half": (128, 13, False),
    "sc16": (0, 0, True),
    "offset37": (37, 13, False),
}
CASES = [(N, f) for N in (32768, 65536) for f in ("grid", "half", "sc16")] + [(65536, "offset37")]


@pytest.mark.parametrize("N,form", CASES, ids=["N%d-%s" % c for c in CASES])
def test_scalar_row_forms_against_the_oracle(oracle, N, form):
    if FORCED:
        pytest.skip("suite run under a forced path")
    R = 2
    r, first, sc16 = FORMS[form]
    nslots = N // 256 - (1 if r else 0)
    chans = [(256 * c + r, 256, 0.88, 1.0) for c in range(nslots)]
    ovl, H = N // R, N - N // R
    probe = G.Pipeline(N, R, chans, windowtype=1, max_blocks=1)
    ncu = probe.reserve_compute_units(0)
    probe.close()
    nbmax = 2 * ncu + 3
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nbmax, min_block_launch=1)
    assert p.path() == 3, p.describe()
    lout = p.lout[0]
    assert all(lo == lout for lo in p.lout)
    if sc16:
        raw = noise_sc16(ovl + nbmax * H)
        ring = (raw.astype(np.float32) * np.float32(IN_SCALE)).view(np.complex64)
        d_ring = Dev(raw.nbytes, raw)
    else:
        ring = noise(ovl + nbmax * H)
        d_ring = Dev(ring.nbytes, ring)
    d_out = Dev(p.output_samples(nbmax) * 8)
    which = sorted(set(range(0, nslots, 16)) | {nslots - 1})
    sub = [chans[c] for c in which]
    want = {}                                     # (first block of the run, channel) -> the oracle's samples of the run, from the largest count
    d_nar = Dev(p.output_samples(nbmax) * 4) if sc16 else None
    for nb in (nbmax, ncu + 1, 1):
        if sc16:
            p.set_output_format(None)
            p.process_device_iq("sc16", IN_SCALE, d_ring.p, first, nb, d_out.p)
            assert "input sc16: fused" in p.describe(), p.describe()
            p.synchronize()
            p.set_output_format("sc16", OUT_SCALE)
            p.process_device_iq("sc16", IN_SCALE, d_ring.p, first, nb, d_nar.p)
            d = p.describe()                      # the integer instantiations of the kernel, not a widened copy in front or a narrowing pass behind
            assert "input sc16: fused" in d and "output " in d and ": fused" in d.split("output ")[1], d
        else:
            p.process_device(d_ring.p, first, nb, d_out.p)
        p.synchronize()
        for t0, k in spans_of(nb, ncu):
            if nb == nbmax:
                ref, _ = oracle.channelizer(N, R, 1, sub, ring[ovl + t0 * H:ovl + (t0 + k) * H], prefix=ring[t0 * H:t0 * H + ovl],
                                            first_block=first + t0, nthreads=8)
                for c, w in zip(which, ref):
                    want[t0, c] = w
            for c in which:
                # the run of a smaller count starts where a run of the largest does and is no longer
                w = want[t0, c][:k * lout]
                got = d_out.back((p.channel_offset(c, nb) + t0 * lout) * 8, np.empty(k * lout, np.complex64))
                assert w.shape == got.shape
                l2, mx = rel(got, w)
                print("N=%d %s nb=%d blocks %d..%d channel %d: l2=%.3g max=%.3g" % (N, form, nb, t0, t0 + k - 1, c, l2, mx))
                assert l2 <= TOL and mx <= TOL, "N=%d %s nb=%d blocks %d..%d channel %d: l2=%.3g max=%.3g" % (N, form, nb, t0, t0 + k - 1, c, l2, mx)
                if sc16:
                    nar = d_nar.back((p.channel_offset(c, nb) + t0 * lout) * 4, np.empty((k * lout, 2), np.int16))
                    assert nar.tobytes() == model(got, OUT_SCALE, np.int16).tobytes(), "sc16 out, N=%d nb=%d blocks %d.. channel %d" % (N, nb, t0, c)
    p.close()
