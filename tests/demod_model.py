"""The numpy models of the channel demodulation (fdc_pipeline_set_demod, include/fdc_amd.h) that the tests compare the device with.

With y[t] the complex float32 samples of one channel's stream and y[-1] the sample in front of a call's first (the carry, or 0 at a stream start):

FM   P = y[t] conj(y[t - 1]) = (a.x b.x + a.y b.y, a.y b.x - a.x b.y), a = y[t], b = y[t - 1], in float32 with every product and sum rounded on its own
     (products32); d[t] = float32(gain * atan2f(Im P, Re P)), and +0.0 where both components of P compare equal to zero.
     theta64: the float64 angle of the float64 product of the float32 samples.  The bound (DESIGN.md "Channel demodulation"): each component of the
     computed P is off by at most 3 2^-24 |a| |b| to first order, so its argument by at most 3 sqrt(2) 2^-24 rad whatever the cancellation; atan2f is
     held to OpenCL's 6 ulp, which the device library is built to (no bound of its own is documented with the installed library): 6 2^-23 |theta|; the
     gain product adds 2^-24 |theta|:
         |d - gain theta64| <= |gain| (5 + 13 |theta64|) 2^-24      modulo 2 pi |gain| (a product next to the negative real axis may land on either side)
     Samples with |a| |b| < 2^-60 are outside the bound (the products underflow); fm_check counts them and the tests assert there were none.
MAG  d[t] = float32(gain * sqrt(float32(float32(re re) + float32(im im)))): numpy states it bit for bit in float32 (mag32).  No state.

The carry rule over a list of calls: Carry."""
import numpy as np

F32 = np.float32
TINY = 2.0 ** -60


def c64(y):
    return np.ascontiguousarray(y, np.complex64).reshape(-1)


def with_front(y, front=0):
    """(a, b) = (y[t], y[t - 1]) of one call's run of one channel; front: the sample in front of y[0]"""
    y = c64(y)
    return y, np.concatenate([np.array([front], np.complex64), y[:-1]])


def products32(a, b):
    """(Re P, Im P) as the device computes them: float32, every product and sum rounded on its own"""
    ax, ay, bx, by = (np.ascontiguousarray(v, F32) for v in (a.real, a.imag, b.real, b.imag))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return ax * bx + ay * by, ay * bx - ax * by


def theta64(y, front=0):
    """the float64 angle of the float64 product of the float32 samples, one per sample of y"""
    a, b = with_front(y, front)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.angle(a.astype(np.complex128) * np.conj(b.astype(np.complex128)))


def fm32(y, front=0, gain=1.0):
    """a float32 numpy restatement of the FM output: products32, numpy's float32 arctan2, the zero rule, the gain product"""
    re, im = products32(*with_front(y, front))
    with np.errstate(invalid="ignore"):
        d = (F32(gain) * np.arctan2(im, re)).astype(F32)
    return np.where((re == 0) & (im == 0), F32(0.0), d).astype(F32)


def mag32(y, gain=1.0):
    """the MAG output, bit for bit"""
    y = c64(y)
    re, im = np.ascontiguousarray(y.real, F32), np.ascontiguousarray(y.imag, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (F32(gain) * np.sqrt(re * re + im * im)).astype(F32)


def fm_bound(theta, gain=1.0):
    return abs(float(F32(gain))) * (5.0 + 13.0 * np.abs(theta)) * 2.0 ** -24


def fm_ratio(d, y, front=0, gain=1.0):
    """(ratio[t], outside[t]): the error of d against gain theta64, modulo 2 pi |gain|, in units of the bound; where the float32 product is (0, 0) the
    zero rule holds instead: ratio 0 if d is +0.0 in bits, inf otherwise.  outside: samples the bound does not cover (|a| |b| < 2^-60 and P not zero,
    or a sample that is not finite); their ratio is 0."""
    d = np.ascontiguousarray(d, F32).reshape(-1)
    a, b = with_front(y, front)
    assert d.shape == a.shape, (d.shape, a.shape)
    g = float(F32(gain))
    re, im = products32(a, b)
    zero = (re == 0) & (im == 0)
    th = theta64(y, front)
    with np.errstate(invalid="ignore", over="ignore"):
        small = np.abs(a.astype(np.complex128)) * np.abs(b.astype(np.complex128)) < TINY
        finite = np.isfinite(a.view(F32).reshape(-1, 2)).all(axis=1) & np.isfinite(b.view(F32).reshape(-1, 2)).all(axis=1)
        outside = ~zero & (small | ~finite)
        diff = d.astype(np.float64) - g * th
        period = 2.0 * np.pi * abs(g)
        diff = np.abs(diff - np.round(diff / period) * period)
        ratio = diff / fm_bound(th, g)
    ratio = np.where(zero, np.where(d.view(np.uint32) == 0, 0.0, np.inf), ratio)
    return np.where(outside, 0.0, ratio), outside


def fm_check(d, y, front, gain, what):
    """one channel of one call: every sample of d inside the bound (or the zero rule), none left out.  Prints the largest ratio before it asserts;
    returns it."""
    r, outside = fm_ratio(d, y, front, gain)
    worst = float(r.max()) if r.size else 0.0
    print("%s: %d samples, largest FM error %.3g of its bound" % (what, r.size, worst))
    assert not outside.any(), "%s: %d samples are outside the bound's range (|a| |b| < 2^-60 or not finite)" % (what, int(outside.sum()))
    assert (r <= 1.0).all(), (what, "sample %d" % int(np.argmax(r)), worst)
    return worst


class Carry:
    """The carry rule over a list of calls, for one handle: front(first_block) is the sample in front of each channel's first sample of a call that
    starts at first_block (zeros unless the call continues the stream); done(first_block, nblocks, last) records a successful FM call whose last
    samples were `last` (one per channel); restart() is what create, reset, a change of mode, a switch from OFF and a failed call leave."""

    def __init__(self, nchan):
        self.nchan = nchan
        self.restart()

    def restart(self):
        self.next, self.last = -1, np.zeros(self.nchan, np.complex64)

    def front(self, first_block):
        return self.last.copy() if first_block == self.next else np.zeros(self.nchan, np.complex64)

    def done(self, first_block, nblocks, last):
        self.next, self.last = first_block + nblocks, np.ascontiguousarray(last, np.complex64).copy()


def fm_stream(carry, calls, gain=1.0, f=fm32):
    """calls: [(first_block, nblocks, [y_c of the call, one array per channel])]; the model's output of every call, [[d_c]] (f: fm32)"""
    out = []
    for first, nb, ys in calls:
        fr = carry.front(first)
        out.append([f(y, fr[c], gain) for c, y in enumerate(ys)])
        carry.done(first, nb, [c64(y)[-1] for y in ys])
    return out
