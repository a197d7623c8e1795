"""GPU tests (-m gpu) of where a pass of stage 1 of the one-block-per-CU kernel (fdc_block256.hip, one_pass) issues the row loads of the next pass.

The spread forms (SPREAD, plain input loads) issue them in four groups between the phases of the pass; a launch with streamed input loads
(FDC_BLOCK_HINTS bit 1, FDC_PIPE_NT_LOADS) takes the form with all sixteen at the top of the pass.  The hint changes no value and the arithmetic is the
same, so a handle with default hints and one with FDC_BLOCK_HINTS = 3 must give the same bytes for the same ring: every output sample of every channel
is compared (tobytes() equality over the whole output), for N = 16384, 32768, 65536, the forms grid / offset37 / half / r4, sc16 input at N = 65536, and
the integer forms below N = 65536 (sc8 and sc16 input, sc16 and sc8 output, each served by the kernel's own loads and stores).

Block counts, all through the same two handles and the same ring: nb = 2 * (compute units) + 3 (workgroups run two and three blocks, the last round is
ragged, what a pass fetches ahead wraps into the workgroup's next block), nb = 1 (the last pass fetches "the same rows again, unused") and
nb = (compute units) + 1.

Forms without a spread instantiation (kBlkSpread), which run the same top-of-pass form under both hints, so that their cases pass and say nothing
about placement, 4 of the 19: offset37 at N = 16384, 32768 and 65536 (offset plans), and r4 at N = 65536 (R = 4 at P = 8).  The forward-transform form
(keep_spectrum) has none either and no case here; tests/test_block256_stage1_tables_gpu.py holds it, and every form above, to the oracle at these
block counts."""
import ctypes as C

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import _default_cfg_fields

pytestmark = pytest.mark.gpu
FORCED = any(G.defaults.get(k) for k in ("FDC_FORCE_GENERIC", "FDC_NO_POLY", "FDC_NO_BLOCK"))
IN_SCALE = {"sc16": 2.0 ** -10, "sc8": 2.0 ** -3}
OUT_SCALE = {"sc16": 200.0, "sc8": 100.0}

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
        rng = np.random.default_rng(20258)
        m = max(n, 16384 + 520 * 49152)
        _noise["x"] = (rng.standard_normal(m, dtype=np.float32) + 1j * rng.standard_normal(m, dtype=np.float32)).astype(np.complex64)
    return _noise["x"][:n]


def noise_int(fmt, n):
    """the first n samples (interleaved I/Q) of one seeded integer stream per format"""
    dt = np.int16 if fmt == "sc16" else np.int8
    if fmt not in _noise or _noise[fmt].size < 2 * n:
        rng = np.random.default_rng(20259)
        info = np.iinfo(dt)
        _noise[fmt] = rng.integers(info.min, info.max + 1, size=2 * max(n, 32768 + 520 * 32768), dtype=dt)
    return _noise[fmt][:2 * n]


class Dev:
    """a device buffer that frees itself"""

    def __init__(self, nbytes, src=None):
        self.p = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.p), C.c_size_t(max(1, nbytes))) == 0
        if src is not None:
            assert hip().hipMemcpy(self.p, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), 1) == 0

    def back(self, a):
        assert hip().hipMemcpy(C.c_void_p(a.ctypes.data), self.p, C.c_size_t(a.nbytes), 2) == 0
        return a

    def __del__(self):
        if self.p:
            hip().hipFree(self.p)
            self.p = C.c_void_p()


FORMS = {
    # name: (R, offset r, first_block)
    "grid": (2, 0, 0),
    "offset37": (2, 37, 13),
    "half": (2, 128, 0),
    "r4": (4, 0, 0),
}
# (N, form, input format, output format): None = complex64
CASES = [(N, f, None, None) for N in (16384, 32768, 65536) for f in FORMS] + [(65536, "grid", "sc16", None)]
CASES += [(16384, "grid", "sc8", None), (32768, "grid", "sc8", None), (16384, "grid", None, "sc16"), (32768, "half", None, "sc8"),
          (32768, "r4", "sc16", "sc8"), (16384, "r4", "sc8", "sc16")]


def case_id(c):
    N, form, fin, fout = c
    if (N, form, fin, fout) == (65536, "grid", "sc16", None):
        return "N65536-sc16"
    return "N%d-%s" % (N, form) + ("-in_%s" % fin if fin else "") + ("-out_%s" % fout if fout else "")


@pytest.mark.parametrize("N,form,fin,fout", CASES, ids=[case_id(c) for c in CASES])
def test_spread_loads_give_the_bytes_of_the_streamed_load_form(N, form, fin, fout):
    if FORCED:
        pytest.skip("suite run under a forced path")
    R, r, first = FORMS[form]
    nslots = N // 256 - (1 if r else 0)
    chans = [(256 * c + r, 256, 0.88, 1.0) for c in range(nslots)]
    ovl, H = N // R, N - N // R
    probe = G.Pipeline(N, R, chans, windowtype=1, max_blocks=1)
    ncu = probe.reserve_compute_units(0)
    probe.close()
    nbmax = 2 * ncu + 3
    base = _default_cfg_fields()[0]
    hints3 = (base & ~_lib.FDC_PIPE_PLAIN_STORES) | _lib.FDC_PIPE_NT_LOADS          # FDC_BLOCK_HINTS = 3
    handles = [G.Pipeline(N, R, chans, windowtype=1, max_blocks=nbmax, flags=fl, min_block_launch=1) for fl in (None, hints3)]
    for p in handles:
        assert p.path() == 3, p.describe()
        if fout:
            p.set_output_format(fout, OUT_SCALE[fout])
    ring = noise_int(fin, ovl + nbmax * H) if fin else noise(ovl + nbmax * H)
    d_ring = Dev(ring.nbytes, ring)
    out_dt, out_per = {None: (np.complex64, 1), "sc16": (np.int16, 2), "sc8": (np.int8, 2)}[fout]
    n_max = handles[0].output_samples(nbmax)
    d_out = [Dev(n_max * out_per * np.dtype(out_dt).itemsize) for _ in handles]
    for nb in (nbmax, 1, ncu + 1):
        n_out = handles[0].output_samples(nb)
        got = []
        for p, d in zip(handles, d_out):
            assert p.output_samples(nb) == n_out
            if fin:
                p.process_device_iq(fin, IN_SCALE[fin], d_ring.p, first, nb, d.p)
            else:
                p.process_device(d_ring.p, first, nb, d.p)
            p.synchronize()
            desc = p.describe()                     # the integer instantiations of the kernel, not a widened copy in front or a narrowing pass behind
            assert not fin or "input %s: fused" % fin in desc, desc
            assert not fout or "output %s: fused" % fout in desc, desc
            got.append(d.back(np.empty(n_out * out_per, out_dt)))
        what = "N=%d %s in=%s out=%s nb=%d" % (N, form, fin, fout, nb)
        if fout is None:
            assert np.isfinite(got[1].view(np.float32)).all(), what
        assert np.count_nonzero(got[1]) > 0, what + ": no output"
        assert got[0].tobytes() == got[1].tobytes(), "%s: %d of %d values differ" % (what, int(np.count_nonzero(got[0] != got[1])), got[0].size)
    for p in handles:
        p.close()
