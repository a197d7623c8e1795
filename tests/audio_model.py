"""The numpy model of an audio stage behind the channel demodulation: a decimating FIR over a demodulated port (GNU Radio's fir_filter_fff with
decimation D), which runs on the host today.  It states the arithmetic a device pass would have to reproduce bit for bit.

With d[t] the float32 stream the channel demodulation gives for one channel (tests/demod_model.py), d[t] = +0 in front of the stream's start, D the
decimation and h[0 .. K-1] the float32 taps:

    a[m] = sum over k = 0 .. K-1 of h[k] d[m D - k]

THE ORDER IS PART OF THE DEFINITION: float32, k ascending, from acc = +0, acc = float32(acc + float32(h[k] d[m D - k])): every product and every sum
rounded on its own (fir_decim32).  fir_decim64 is the same sum in float64.  s16: q = saturate(round_half_even(float32(a scale))), NaN -> 0, +-Inf -> the
limits (the rule of sc16 output).

The bound of the float32 sum against the float64 one over the SAME d: the product of tap k carries one rounding and then
passes through the additions of taps k .. K-1, of which the first of all (to +0) is exact: at most K roundings each, so
|a32 - a64| <= ((1 + 2^-24)^K - 1) sum |h[k] d[.]| <= 1.01 K 2^-24 sum |h[k] d[m D - k]| for K <= 256 (no product may underflow).  fir_bound adds
demod's own bound passed through the filter.

The history rule over a list of calls: History."""
import numpy as np

F32 = np.float32


def f32(v):
    return np.ascontiguousarray(v, F32).reshape(-1)


def _front(d, K, hist, dtype):
    """z with z[K - 1 + t] = d[t]: the call's samples behind the K - 1 values in front of them (hist; None: zeros)"""
    h = np.zeros(K - 1, dtype) if hist is None else np.ascontiguousarray(hist, dtype).reshape(-1)
    assert h.size == K - 1, (h.size, K)
    return np.concatenate([h, np.ascontiguousarray(d, dtype).reshape(-1)])


def fir_decim32(d, taps, D, hist=None):
    """the audio of one call of one channel, bit for bit: d its float32 demodulated samples (a multiple of D of them), hist the K - 1 in front"""
    h = f32(taps)
    K = h.size
    z = _front(d, K, hist, F32)
    n = (z.size - (K - 1)) // D
    assert n * D == z.size - (K - 1), "the call's samples are a multiple of the decimation"
    at = (K - 1) + np.arange(n) * D
    acc = np.zeros(n, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(K):
            p = h[k] * z[at - k]            # float32 x float32 -> float32: rounded once
            acc = acc + p                   # and the sum rounded on its own
    assert acc.dtype == F32
    return acc


def fir_decim64(d, taps, D, hist=None):
    """the same sum in float64, of float64 d and the float32 taps"""
    h = f32(taps).astype(np.float64)
    K = h.size
    z = _front(d, K, hist, np.float64)
    n = (z.size - (K - 1)) // D
    at = (K - 1) + np.arange(n) * D
    acc = np.zeros(n, np.float64)
    for k in range(K):
        acc = acc + h[k] * z[at - k]
    return acc


def fir_abs64(d, taps, D, hist=None):
    """sum over k of |h[k] d[m D - k]| in float64"""
    return fir_decim64(np.abs(np.asarray(d, np.float64)), np.abs(f32(taps)), D, None if hist is None else np.abs(np.asarray(hist, np.float64)))


def s16(a, scale):
    """the int16 narrowing of float32 a"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = np.rint(f32(a) * F32(scale))    # the product rounded once in float32; rint rounds half to even
    t = np.where(np.isnan(t), F32(0), t)
    return np.clip(t, -32768.0, 32767.0).astype(np.int16)


def audio32(d, taps, D, fmt="f32", scale=1.0, hist=None):
    a = fir_decim32(d, taps, D, hist)
    return s16(a, scale) if fmt == "s16" else a


def sum_bound(d64, taps, D, hist=None):
    """the float32 summation alone: 1.01 K 2^-24 sum |h[k] d[m D - k]|"""
    return 1.01 * f32(taps).size * 2.0 ** -24 * fir_abs64(d64, taps, D, hist)


def fir_bound(theta64, gain, taps, D):
    """the bound of a against the float64 FIR of gain theta64, for a stream start (zeros in front; the first sample of theta64 is the stream's
    first, whose d is +0 by the zero rule and whose theta64 must be given as 0):
        sum |h[k]| |gain| (5 + 13 |theta64[m D - k]|) 2^-24  +  1.01 K 2^-24 sum |h[k] d64[m D - k]|"""
    g = abs(float(F32(gain)))
    th = np.asarray(theta64, np.float64)
    first = fir_decim64(g * (5.0 + 13.0 * np.abs(th)) * 2.0 ** -24, np.abs(f32(taps)), D)
    return first + sum_bound(float(F32(gain)) * th, taps, D)


class History:
    """The history rule over a list of calls, for one stream: front(first_block) is what stands in front of each channel's first sample of a call that
    starts at first_block (K - 1 values of d; zeros unless the call continues the stream); done(first_block, nblocks, ds) records a successful call
    whose demodulated samples were ds (one array per channel): the new history is the tail of (what stood in front, the call's d), which covers calls
    that bring fewer than K - 1 samples; restart() starts the stream anew."""

    def __init__(self, nchan, K):
        self.nchan, self.K = nchan, K
        self.restart()

    def restart(self):
        self.next, self.hist = -1, [np.zeros(self.K - 1, F32) for _ in range(self.nchan)]

    def front(self, first_block):
        if first_block == self.next:
            return [h.copy() for h in self.hist]
        return [np.zeros(self.K - 1, F32) for _ in range(self.nchan)]

    def done(self, first_block, nblocks, ds):
        fr = self.front(first_block)
        self.hist = [np.concatenate([fr[c], f32(ds[c])])[len(fr[c]) + f32(ds[c]).size - (self.K - 1):] for c in range(self.nchan)]
        self.next = first_block + nblocks


def audio_stream(history, calls, taps, D, fmt="f32", scale=1.0):
    """calls: [(first_block, nblocks, [d_c of the call, one float32 array per channel])]; the model's audio of every call, [[a_c]]"""
    out = []
    for first, nb, ds in calls:
        fr = history.front(first)
        out.append([audio32(d, taps, D, fmt, scale, fr[c]) for c, d in enumerate(ds)])
        history.done(first, nb, ds)
    return out
