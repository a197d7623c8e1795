"""GPU tests (-m gpu) of the one-row-set forms of the one-block-per-CU kernel (fdc_block256.hip, kBlkOneSet): the spread forms at N = 32768 and 65536 run
stage 1 on ONE set of sixteen row registers — the next pass's loads land in the registers the pass computes on, the first group of them behind the
first exchange write — and keep the lane's twiddle row W_256^(b p) in registers for the length of a block's stage 1 (twk, read once per block).

What can go wrong: a next-pass load landing in a register the pass still reads; the wrap of the last pass into the workgroup's next block, held
across stage 2; a lone block ("the same rows again, unused"); a stale twk in a workgroup's second block.

Byte equality, the method of tests/test_block256_load_placement_gpu.py: a launch with streamed input loads (FDC_BLOCK_HINTS = 3) takes the form with
all sixteen row loads at the top of a pass, two row sets and the twiddle row read from LDS in every pass; the arithmetic is the same, so default hints
must give the same bytes for the same ring (tobytes() over the whole output).  Block counts nb = 2 * (compute units) + 3, nb = 1 and
nb = (compute units) + 1 through the same two handles.  The cases are the converted forms that file does not reach (its own cases cover grid / half /
r4 on float samples at both lengths, sc16 input at N = 65536 and four integer forms at N = 32768).

One case against the oracle: N = 65536 on the grid, three blocks through ONE workgroup (all compute units but one reserved), every sample of every
channel at the 1e-5 of the other block-kernel tests: the workgroup's second and third block run on a twk read again for each, on rows fetched across
stage 2.  (1e-5 on noise sees a stale or misplaced row, not one slightly wrong table entry — tests/test_fft_model_cpu.py; the byte equality above
carries the arithmetic of the two-set form over, and tests/test_block_accuracy_gpu.py says what is held to float32-grade error.)"""
import ctypes as C

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import _default_cfg_fields

pytestmark = pytest.mark.gpu
TOL = 1e-5
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
        rng = np.random.default_rng(20262)
        m = max(n, 8192 + 520 * 24576)
        _noise["x"] = (rng.standard_normal(m, dtype=np.float32) + 1j * rng.standard_normal(m, dtype=np.float32)).astype(np.complex64)
    return _noise["x"][:n]


def noise_int(fmt, n):
    """the first n samples (interleaved I/Q) of one seeded integer stream per format"""
    dt = np.int16 if fmt == "sc16" else np.int8
    if fmt not in _noise or _noise[fmt].size < 2 * n:
        rng = np.random.default_rng(20263)
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
    # name: (R, offset r)
    "grid": (2, 0),
    "half": (2, 128),
    "r4": (4, 0),
}
# (N, form, input format, output format, first_block): None = complex64
CASES = [(65536, "grid", "sc8", None, 0), (65536, "half", "sc16", None, 13), (65536, "half", "sc8", None, 0), (32768, "grid", "sc16", None, 0),
         (32768, "half", "sc8", "sc8", 0), (32768, "grid", None, "sc16", 0), (32768, "r4", None, None, 0)]


def case_id(c):
    N, form, fin, fout, first = c
    return "N%d-%s" % (N, form) + ("-in_%s" % fin if fin else "") + ("-out_%s" % fout if fout else "") + ("-first%d" % first if first else "")


@pytest.mark.parametrize("N,form,fin,fout,first", CASES, ids=[case_id(c) for c in CASES])
def test_one_row_set_gives_the_bytes_of_the_two_set_form(N, form, fin, fout, first):
    if FORCED:
        pytest.skip("suite run under a forced path")
    R, r = FORMS[form]
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
        what = "N=%d %s in=%s out=%s first=%d nb=%d" % (N, form, fin, fout, first, nb)
        if fout is None:
            assert np.isfinite(got[1].view(np.float32)).all(), what
        assert np.count_nonzero(got[1]) > 0, what + ": no output"
        assert got[0].tobytes() == got[1].tobytes(), "%s: %d of %d values differ" % (what, int(np.count_nonzero(got[0] != got[1])), got[0].size)
    for p in handles:
        p.close()


def rel(a, b):
    a = a.astype(np.complex128); b = b.astype(np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(np.abs(a - b).max() / np.abs(b).max())


def test_three_blocks_through_one_workgroup_against_the_oracle(oracle):
    if FORCED:
        pytest.skip("suite run under a forced path")
    N, R, nb = 65536, 2, 3
    chans = [(256 * c, 256, 0.88, 1.0) for c in range(N // 256)]
    ovl, H = N // R, N - N // R
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, min_block_launch=1)
    assert p.path() == 3, p.describe()
    ncu = p.reserve_compute_units(0)
    assert p.reserve_compute_units(ncu - 1) == 1          # a grid of one workgroup: blocks 0, 1, 2 in turn
    lout = p.lout[0]
    assert all(lo == lout for lo in p.lout)
    ring = noise(ovl + nb * H)
    d_ring = Dev(ring.nbytes, ring)
    n_out = p.output_samples(nb)
    d_out = Dev(n_out * 8)
    p.process_device(d_ring.p, 0, nb, d_out.p)
    p.synchronize()
    got = d_out.back(np.empty(n_out, np.complex64))
    ref, _ = oracle.channelizer(N, R, 1, chans, ring[ovl:], prefix=ring[:ovl], first_block=0, nthreads=8)
    worst = (0.0, 0.0)
    for c, w in enumerate(ref):
        g = got[p.channel_offset(c, nb):p.channel_offset(c, nb) + nb * lout]
        assert w.shape == g.shape
        for t in range(nb):                          # per block: the second and third are the ones a stale row would spoil
            l2, mx = rel(g[t * lout:(t + 1) * lout], w[t * lout:(t + 1) * lout])
            worst = (max(worst[0], l2), max(worst[1], mx))
            assert l2 <= TOL and mx <= TOL, "channel %d block %d: l2=%.3g max=%.3g" % (c, t, l2, mx)
    print("N=65536 grid, 3 blocks through one workgroup, 256 channels: worst l2=%.3g max=%.3g" % worst)
    p.close()
