"""CPU tests of the audio stage behind the channel demodulation, as far as it is built: the numpy model of a decimating FIR
over a demodulated port (tests/audio_model.py: float32 in one stated order, float64, the int16 narrowing, the history over a list of calls) on
hand-made rows, the cut rule on the model, the float32 statement inside its bound on constant-envelope FM rows, and lowpass_taps."""
import numpy as np
import pytest

import gr_fdc_amd as G
import audio_model as A
import demod_model as M

# the filters (D, K) and the run lengths of the bound test: the runs of the example plan at R = 2 and 5 blocks
BOUND_FILTERS = ((8, 64), (4, 33), (1, 256), (64, 1), (2, 2))
BOUND_RUNS = (640, 1280, 2560)
GAIN = float(np.float32(1.0 / (2.0 * np.pi)))


def f32bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32).tolist()


def fm_rows(n, seed, amp=0.75):
    """a constant-envelope FM row of n complex64 samples: |theta| <= 2.4 rad per sample as designed (2.5 after rounding is asserted by the users),
    |y| = amp >= 0.1, so that no sample is near the +-pi cut and none underflows: a band-limited modulation plus steps to both ends of the range"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    th = 1.1 * np.sin(2 * np.pi * 0.013 * t + rng.uniform(0, 6)) + 0.9 * np.sin(2 * np.pi * 0.11 * t) + rng.uniform(-0.4, 0.4, n)
    th[n // 3: n // 3 + 7] = 2.4
    th[n // 2: n // 2 + 5] = -2.4
    return (amp * np.exp(1j * np.cumsum(th))).astype(np.complex64)


def taps_for(D, K, seed=0):
    """the low-pass of the decimation where it has a shape (K >= 3), else seeded taps of both signs"""
    if K >= 3:
        return G.lowpass_taps(D, K)
    return np.random.default_rng(seed + K).uniform(-1, 1, K).astype(np.float32)


def test_models_on_hand_made_rows():
    h = np.array([0.5, -0.25, 2.0, 0.125, 3.0], np.float32)
    # an impulse returns the taps (D = 1), and every D-th of them behind a shifted impulse
    d = np.zeros(12, np.float32); d[0] = 1
    assert A.fir_decim32(d, h, 1)[:5].tolist() == h.tolist() and not A.fir_decim32(d, h, 1)[5:].any()
    d = np.zeros(12, np.float32); d[1] = 1
    assert A.fir_decim32(d, h, 2).tolist() == [0.0, h[1], h[3], 0.0, 0.0, 0.0]
    # a constant returns sum h in the stated order (k ascending from +0), once the filter is full
    h3 = np.array([1.0, 2.0 ** -24, 2.0 ** -24], np.float32)
    want = np.float32(np.float32(np.float32(0) + h3[0]) + h3[1]) + h3[2]          # (1 + 2^-24) + 2^-24 = 1: both ties go to even
    assert want == np.float32(1.0) and np.float32(h3[2] + h3[1]) + h3[0] != want     # the order shows
    assert f32bits(A.fir_decim32(np.ones(8, np.float32), h3, 1)[2:]) == f32bits(np.full(6, want))
    assert f32bits(A.fir_decim32(np.ones(8, np.float32), h3[::-1].copy(), 1)[2:]) == f32bits(np.full(6, np.float32(1.0) + np.float32(2.0 ** -23)))
    # K = 1: a gain and a pick; D = 1: a plain FIR, equal to numpy's convolution where that is exact
    d = np.arange(1, 13, dtype=np.float32)
    assert A.fir_decim32(d, [3.0], 4).tolist() == [3.0, 15.0, 27.0]
    hi = np.array([1, 2, 3], np.float32)
    assert A.fir_decim32(d, hi, 1).tolist() == np.convolve(d, hi)[:12].tolist()
    assert A.fir_decim64(d, hi, 3).tolist() == np.convolve(d.astype(np.float64), hi)[:12:3].tolist()
    # the history stands in front: a call behind one equals the tail of one call of both
    both = A.fir_decim32(d, h, 2)
    assert f32bits(np.concatenate([A.fir_decim32(d[:4], h, 2), A.fir_decim32(d[4:], h, 2, hist=d[:4])])) == f32bits(both)
    # K - 1 longer than a call: a call of 2 samples under 5 taps; the new history is the old one's tail and the call's d
    st = A.History(1, 5)
    st.done(0, 1, [d[:2]])
    assert st.hist[0].tolist() == [0.0, 0.0, 1.0, 2.0] and st.next == 1
    st.done(1, 1, [d[2:4]])
    assert st.hist[0].tolist() == [1.0, 2.0, 3.0, 4.0]
    st.done(5, 1, [d[4:6]])                                         # a call elsewhere: zeros stood in front of it
    assert st.hist[0].tolist() == [0.0, 0.0, 5.0, 6.0] and st.front(5)[0].tolist() == [0.0] * 4 and st.front(6)[0].tolist() == [0.0, 0.0, 5.0, 6.0]
    assert A.History(2, 1).front(0)[1].size == 0
    # NaN and +-Inf by IEEE rules: a NaN reaches the outputs whose window holds it; Inf times a zero tap is NaN; Inf - Inf is NaN
    d = np.ones(12, np.float32); d[5] = np.nan
    assert np.isnan(A.fir_decim32(d, h, 1)).tolist() == [False] * 5 + [True] * 5 + [False] * 2
    d = np.ones(6, np.float32); d[2] = np.inf
    assert np.isnan(A.fir_decim32(d, [1.0, 0.0], 1)).tolist() == [False, False, False, True, False, False]
    assert A.fir_decim32(d, [1.0, 0.5], 1)[2:4].tolist() == [np.inf, np.inf] and np.isnan(A.fir_decim32(d, [1.0, -1.0], 1)[3]) == False
    assert np.isnan(A.fir_decim32(np.array([np.inf, np.inf], np.float32), [1.0, -1.0], 1)[1])
    # S16: ties to even, saturation, NaN -> 0, Inf -> the limits, the product rounded once in float32
    a = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e9, -1e9, np.nan, np.inf, -np.inf, 32767.5, -32768.5, 32767.4], np.float32)
    assert A.s16(a, 1.0).tolist() == [0, 2, 2, 0, -2, 32767, -32768, 0, 32767, -32768, 32767, -32768, 32767]
    assert A.s16(a, 1.0).dtype == np.int16
    third = np.float32(1.0) / np.float32(3.0)
    assert A.s16([4.5], third).tolist() == [int(np.rint(np.float32(4.5) * third))] and A.s16([3.0], 0.5).tolist() == [2] and A.s16([5.0], 0.5).tolist() == [2]
    assert A.audio32(np.ones(4, np.float32), [100.0], 2, "s16", 2.5).tolist() == [250, 250]


def test_the_cut_rule():
    """however a stream is cut into calls that continue one another, the model gives the bits of one call; a call elsewhere starts anew"""
    rng = np.random.default_rng(5)
    lout, nch, D = [8, 24], 2, 4
    h = rng.standard_normal(33).astype(np.float32)                  # K - 1 = 32 spans four blocks of 8
    d = [rng.standard_normal(7 * lo).astype(np.float32) for lo in lout]
    for fmt, scale in (("f32", 1.0), ("s16", 300.0)):
        one = A.audio_stream(A.History(nch, h.size), [(0, 7, d)], h, D, fmt, scale)[0]
        assert [o.size for o in one] == [14, 42] and one[0].dtype == (np.int16 if fmt == "s16" else np.float32)
        for cut in ((1,) * 7, (3, 4), (1, 1, 5)):
            calls, b = [], 0
            for n in cut:
                calls.append((b, n, [d[c][b * lout[c]:(b + n) * lout[c]] for c in range(nch)]))
                b += n
            got = A.audio_stream(A.History(nch, h.size), calls, h, D, fmt, scale)
            for c in range(nch):
                assert np.concatenate([g[c] for g in got]).tobytes() == one[c].tobytes(), (fmt, cut, c)
        # a call elsewhere: zeros stand in front of it
        st = A.History(nch, h.size)
        got = A.audio_stream(st, [(0, 3, [d[c][:3 * lout[c]] for c in range(nch)]), (4, 3, [d[c][4 * lout[c]:] for c in range(nch)])], h, D, fmt, scale)
        for c in range(nch):
            assert got[1][c].tobytes() == A.audio32(d[c][4 * lout[c]:], h, D, fmt, scale).tobytes()
            assert got[1][c].tobytes() != one[c][4 * lout[c] // D:].tobytes()
        assert st.next == 7


@pytest.mark.parametrize("n", BOUND_RUNS)
@pytest.mark.parametrize("D,K", BOUND_FILTERS)
def test_the_float32_restatement_is_inside_the_bound(D, K, n):
    """constant-envelope FM rows through numpy's float32 FM statement (demod_model.fm32) and fir_decim32: every sample within
        sum |h[k]| |gain| (5 + 13 |theta64[mD-k]|) 2^-24 + 1.01 K 2^-24 sum |h[k] d64[mD-k]|
    of the float64 FIR of gain theta64 (demod's documented bound through the filter, and sequential float32 summation), no sample left out, and the
    rows are what the bound asks for (|theta| <= 2.5, |y| >= 0.1)"""
    y = fm_rows(n, n + D)
    th = M.theta64(y)
    assert np.abs(th).max() <= 2.5 and np.abs(y).min() >= 0.1 and th[0] == 0
    d = M.fm32(y, 0, GAIN)
    assert not M.fm_ratio(d, y, 0, GAIN)[1].any()
    h = taps_for(D, K)
    a, a64, lim = A.fir_decim32(d, h, D), A.fir_decim64(GAIN * th, h, D), A.fir_bound(th, GAIN, h, D)
    assert a.size == n // D and (lim > 0).all()
    r = np.abs(a.astype(np.float64) - a64) / lim
    print("D = %d, K = %d, %d samples: largest error %.3g of the bound" % (D, K, n, r.max()))
    assert (r <= 1.0).all(), (D, K, n, r.max())
    # the summation alone, against the float64 sum of the same float32 d
    rs = np.abs(a.astype(np.float64) - A.fir_decim64(d, h, D)) / np.maximum(A.sum_bound(d, h, D), 1e-300)
    assert (rs <= 1.0).all(), rs.max()


@pytest.mark.parametrize("D,K", [(1, 1), (2, 2), (8, 64), (8, 65), (3, 31), (64, 256), (4, 33)])
def test_lowpass_taps(D, K):
    h = G.lowpass_taps(D, K)
    assert h.dtype == np.float32 and h.shape == (K,)
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= K * 2.0 ** -24           # unit DC gain, up to the rounding of the taps
    assert np.array_equal(h, h[::-1])                                              # symmetric: linear phase
    if K >= 8 * D and D > 1:
        # a low-pass: the response at the output rate's Nyquist frequency is about a half, far above it small
        w = np.exp(-2j * np.pi * np.arange(K) * 0.5 / D)
        assert 0.3 < abs((h * w).sum()) < 0.7
        assert abs((h * np.exp(-2j * np.pi * np.arange(K) * min(0.5, 1.5 / D))).sum()) < 0.05
    assert np.array_equal(G.lowpass_taps(D, K, cutoff=0.5 / D), h)
    for bad in ((0, 8), (65, 8), (8, 0), (8, 257), (1.5, 8)):
        with pytest.raises(ValueError):
            G.lowpass_taps(*bad)
    with pytest.raises(ValueError):
        G.lowpass_taps(8, 64, cutoff=0.6)
