"""The two numpy models of the channel lag-1 correlation (fdc_pipeline_set_lag1, include/fdc_amd.h) that the tests compare the device with.

    S[m] = sum_{j = 1 .. lout - 1} y[j] conj(y[j - 1])        over the lout samples of row m, the row's own samples only

model64: the reference.  The float32 samples as they are, every product and sum in float64: S64 (complex128) and M = sum_j |y[j]| |y[j - 1]|.
model32: the stated order, in float32 with every product and every sum rounded on its own: the row on 2^lanes_log2(lout) lanes, lane `sub` the sample
pairs sub, sub + lanes, ... in index order; the owner of pair i adds y[2i] conj(y[2i - 1]) where i >= 1, then y[2i + 1] conj(y[2i]) where 2i + 1 < lout;
a term a conj(b) is (a.x b.x + a.y b.y, a.y b.x - a.x b.y); Re and Im apart, from +0; the lanes joined by an xor butterfly from distance 1 upwards.
The device is held to model32 bit for bit (that is what pins "one order") and to model64 within the bound.

The bound (DESIGN.md "Channel lag-1 correlation"): a component of a term is a sum of two products, off by at most 3 2^-24 |a| |b| to first order
(|a.x b.x| + |a.y b.y| <= |a| |b|); any-order float32 summation of n = lout - 1 terms adds at most (n - 1) 2^-24 sum |term|; so each component is
within (lout + 8) 2^-24 M of S64 for lout <= 24576.  Relative to M, not to |S|: the terms may cancel."""
import numpy as np

# the row lengths the GPU tests reach, by what they reach in the kernel (tests/test_lag1_routes_gpu.py); test_lag1_cpu.py draws rows of each
LOUTS = (1, 2, 3, 4, 6, 7, 8, 12, 15, 16, 24, 32, 48, 56, 60, 64, 96, 112, 120, 128, 192, 224, 240, 256, 384, 448, 480, 512, 768, 896, 960, 6144, 12288,
         24576)


def lanes_log2(lout):
    """the lanes of a row, the levels': log2 of the next power of two of its pair count, a wave at the most"""
    npair = (lout + 1) // 2
    return min(6, 0 if npair <= 1 else (npair - 1).bit_length())


def bound(lout):
    return (lout + 8) * 2.0 ** -24


def rows_of(y, lout):
    return np.ascontiguousarray(y, np.complex64).reshape(-1, lout)


def model64(y, lout):
    """(S64[nrows] complex128, M[nrows] float64) of one channel's samples (complex64, nrows * lout of them)"""
    v = rows_of(y, lout).astype(np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (v[:, 1:] * np.conj(v[:, :-1])).sum(axis=1)
        m = (np.abs(v[:, 1:]) * np.abs(v[:, :-1])).sum(axis=1)
    return s, m


def _term(ax, ay, bx, by):
    """a conj(b) in float32, each product and each sum rounded on its own"""
    p, q = ax * bx, ay * by
    u, v = ay * bx, ax * by
    return p + q, u - v


def model32(y, lout):
    """S[nrows] complex64 in the stated order"""
    v = rows_of(y, lout)
    n = v.shape[0]
    re, im = np.ascontiguousarray(v.real, np.float32), np.ascontiguousarray(v.imag, np.float32)
    npair, lanes = (lout + 1) // 2, 1 << lanes_log2(lout)
    acc_re, acc_im = np.zeros((n, lanes), np.float32), np.zeros((n, lanes), np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i0 in range(0, npair, lanes):                              # one step: the pairs i0 + sub of every lane sub that has one
            i = np.arange(i0, min(i0 + lanes, npair))
            sub = i - i0
            first = i >= 1                                             # y[2i] conj(y[2i - 1])
            if first.any():
                k, s = i[first], sub[first]
                tr, ti = _term(re[:, 2 * k], im[:, 2 * k], re[:, 2 * k - 1], im[:, 2 * k - 1])
                acc_re[:, s] = acc_re[:, s] + tr
                acc_im[:, s] = acc_im[:, s] + ti
            second = 2 * i + 1 < lout                                  # then y[2i + 1] conj(y[2i])
            if second.any():
                k, s = i[second], sub[second]
                tr, ti = _term(re[:, 2 * k + 1], im[:, 2 * k + 1], re[:, 2 * k], im[:, 2 * k])
                acc_re[:, s] = acc_re[:, s] + tr
                acc_im[:, s] = acc_im[:, s] + ti
        d, lane = 1, np.arange(lanes)
        while d < lanes:
            acc_re = acc_re + acc_re[:, lane ^ d]
            acc_im = acc_im + acc_im[:, lane ^ d]
            d <<= 1
    out = np.empty(n, np.complex64)
    out.real, out.imag = acc_re[:, 0], acc_im[:, 0]
    return out


def ratio(s, y, lout):
    """the error of s (complex, nrows) against model64 in units of the bound, per row and component: float64[nrows, 2]; rows with M = 0 or a sample that
    is not finite give 0 where s equals S64 exactly (both zero) and inf otherwise"""
    s64, m = model64(y, lout)
    s = np.asarray(s, np.complex128).reshape(-1)
    assert s.shape == s64.shape, (s.shape, s64.shape)
    err = np.stack([np.abs(s.real - s64.real), np.abs(s.imag - s64.imag)], axis=1)
    lim = (bound(lout) * m)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(err == 0, 0.0, err / lim)


def agrees(s, y, lout, what):
    """one channel of a call: s = complex64[nrows] from the device, y the float32 samples the same call returned.  Every row: both components inside
    (lout + 8) 2^-24 M of the float64 sum, and the bits of model32.  Prints the largest ratio before it asserts; returns it."""
    s = np.ascontiguousarray(s)
    assert s.dtype == np.complex64 and s.shape == (np.asarray(y).size // lout,), (what, s.shape, s.dtype)
    assert np.isfinite(rows_of(y, lout)).all(), what + ": the reference rows must be finite (rows that are not have a test of their own)"
    r = ratio(s, y, lout)
    worst = float(r.max()) if r.size else 0.0
    print("%s: lout %d, %d rows, largest error %.3g of its bound" % (what, lout, s.size, worst))
    assert (r <= 1.0).all(), (what, "row %d" % int(np.argmax(r.max(axis=1))), worst)
    want = model32(y, lout)
    diff = np.flatnonzero(s.view(np.uint32).reshape(-1, 2) != want.view(np.uint32).reshape(-1, 2))
    assert diff.size == 0, "%s: %d of %d components differ from the float32 model in bits, first in row %d (%r against %r)" % (
        what, diff.size, 2 * s.size, diff[0] // 2, s[diff[0] // 2], want[diff[0] // 2])
    return worst
