"""CPU tests of the audio resampler's definition (tests/resample_model.py; no GPU): the float32 model against float64 upsample / convolve / decimate
within the bound of the summation, the L = 1 identity with the decimating form in bytes, cut invariance, the block counts (the model's and the
library's host function against Python integers), and the zero-padding rule.  The device pass is held to the model, in bits, by
tests/test_resample_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import gr_fdc_amd as G
import audio_model as A
import resample_model as RS

F32 = np.float32
RATIOS = ((8, 25, 64), (48, 25, 192), (3, 2, 13), (1, 8, 64), (64, 1, 128), (1, 1, 1), (5, 128, 15), (32, 125, 507), (2, 3, 512))


def taps_of(up, down, ntaps):
    return np.random.default_rng(1000 * up + 10 * down + ntaps).uniform(-1, 1, ntaps).astype(F32)


def upfirdn64(d, taps, up, down):
    """upsample by `up` (zeros between the samples), filter with the taps, keep every `down`-th sample, all in float64 from sample 0"""
    z = np.zeros(d.size * up, np.float64)
    z[::up] = d
    return np.convolve(z, np.asarray(taps, np.float64))[:z.size][::down]


@pytest.mark.parametrize("up,down,ntaps", RATIOS, ids=["%d/%d K%d" % r for r in RATIOS])
def test_the_model_against_float64_upsample_convolve_decimate(up, down, ntaps):
    """|a32 - a64| <= 1.01 Kp 2^-24 sum |h d| (audio_model's bound with K = Kp: the padded zero taps add exact zeros), and the float64 form of the
    model is upsample / np.convolve / decimate to float64 rounding"""
    lout, nb = 96, 5
    rng = np.random.default_rng(up + down)
    d = rng.standard_normal(nb * lout).astype(F32)
    h = taps_of(up, down, ntaps)
    kp = RS.ceil_div(ntaps, up)
    a32 = RS.resample32(d, h, up, down, lout)
    a64 = RS.resample64(d, h, up, down, lout)
    mag = RS.resample64(d, h, up, down, lout, absolute=True)
    want = upfirdn64(d.astype(np.float64), h, up, down)
    assert a32.dtype == F32 and a32.size == want.size == RS.ceil_div(nb * lout * up, down)
    assert np.abs(a64 - want).max() <= 1e-12 * max(1.0, mag.max())
    bound = 1.01 * kp * 2.0 ** -24 * mag
    worst = float((np.abs(a32.astype(np.float64) - a64) / np.maximum(bound, 1e-300)).max()) if ntaps > 1 else 0.0
    print("worst error / bound: %.3f" % worst)
    assert (np.abs(a32.astype(np.float64) - a64) <= bound).all(), worst


@pytest.mark.parametrize("M,K", [(8, 64), (4, 33), (1, 256), (64, 1), (3, 7)])
def test_up_1_is_the_decimating_form_in_bytes(M, K):
    """with L = 1 the outputs are fir_decim32's with D = M, byte for byte, wherever M divides lout; and the matrix has no pads"""
    lout, nb = 192, 4
    rng = np.random.default_rng(M + K)
    d = rng.standard_normal(nb * lout).astype(F32)
    h = rng.uniform(-1, 1, K).astype(F32)
    hist = rng.standard_normal(K - 1).astype(F32)
    for first in (0, 5):
        for fr in (None, hist):
            assert RS.resample32(d, h, 1, M, lout, first, fr).tobytes() == A.fir_decim32(d, h, M, fr).tobytes()
    assert (RS.block_counts(lout, 1, M, 0, nb) == lout // M).all()
    for fmt, scale in (("f32", 1.0), ("s16", 3000.0)):
        assert RS.audio32(d, h, 1, M, lout, 0, fmt, scale, hist).tobytes() == A.audio32(d, h, M, fmt, scale, hist).tobytes()


@pytest.mark.parametrize("first", (0, 5, 2 ** 40 + 3), ids=["0", "5", "2^40 + 3"])
@pytest.mark.parametrize("up,down,ntaps", RATIOS, ids=["%d/%d K%d" % r for r in RATIOS])
def test_cuts_of_the_stream_give_the_same_bits(up, down, ntaps, first):
    """7 blocks from block `first` on as 7, 3 + 4, 1 + 1 + 5 and 2 + 2 + 3: the matrices of the calls, stacked, are the matrix of the one call.  lout 40
    and 7: under (2, 3, 512) a block brings fewer than Kp - 1 samples"""
    louts, nb = [40, 7], 7
    rng = np.random.default_rng(ntaps)
    d = [rng.standard_normal(nb * lo).astype(F32) for lo in louts]
    h = taps_of(up, down, ntaps)
    kp = RS.ceil_div(ntaps, up)

    def run(cut):
        hist, calls, b = A.History(len(louts), kp), [], 0
        hist.next = first          # (a stream that has run up to `first` with zeros: the same as a start there)
        for n in cut:
            calls.append((first + b, n, [d[c][b * lo:(b + n) * lo] for c, lo in enumerate(louts)]))
            b += n
        return np.concatenate(RS.stream(hist, calls, h, up, down, louts))

    whole = run((7,))
    assert whole.shape == (nb, sum(RS.ceil_div(lo * up, down) for lo in louts))
    for cut in ((3, 4), (1, 1, 5), (2, 2, 3)):
        assert run(cut).tobytes() == whole.tobytes(), cut
    # the valid samples, cut from the matrix by the counts, are the stream's outputs of these blocks
    got = G.audio_resampled_channels(whole, louts, up, down, first)
    for c, lo in enumerate(louts):
        assert got[c].tobytes() == RS.resample32(d[c], h, up, down, lo, first).tobytes()
    if first == 0:
        # ... and at block 0 they are the first outputs of the one-shot stream
        for c, lo in enumerate(louts):
            assert got[c].size == RS.ceil_div(nb * lo * up, down)


@pytest.mark.parametrize("up,down,ntaps", RATIOS, ids=["%d/%d K%d" % r for r in RATIOS])
def test_counts(up, down, ntaps):
    for lout in (1, 2, 7, 128, 24576):
        W = RS.ceil_div(lout * up, down)
        for first in (0, 5, 2 ** 40 + 3):
            cnt = RS.block_counts(lout, up, down, first, 300)
            assert ((cnt == W) | (cnt == W - 1)).all() and cnt.min() >= 0
            assert int(cnt.sum()) == RS.first_output(first + 300, lout, up, down) - RS.first_output(first, lout, up, down)
            assert (G.audio_block_counts(lout, up, down, first, 300) == cnt).all()
        # from block 0 on the counts sum to the stream's output count
        assert int(RS.block_counts(lout, up, down, 0, 300).sum()) == RS.ceil_div(300 * lout * up, down)
    # every output's block is the block of its newest sample
    lout, n = 7, np.arange(2000)
    owner = (n * down // up) // lout
    cnt = RS.block_counts(lout, up, down, 0, int(owner.max()) + 1)
    assert (np.bincount(owner, minlength=cnt.size)[:-1] == cnt[:-1]).all()        # (the 2000 outputs end inside the last block)


def test_the_librarys_counts_against_python_integers():
    lib = G.lib()
    for lout, up, down in ((128, 8, 25), (256, 48, 25), (1, 5, 128), (24576, 64, 1), (7, 1, 1), (100, 3, 128)):
        near = (2 ** 62 // lout) // up - 40          # near the largest index whose output index still fits
        for first in (0, 5, 2 ** 40 + 3, near):
            got = (C.c_int32 * 33)()
            assert lib.fdc_audio_resampler_counts(lout, up, down, first, 33, got) == 0, (lout, up, down, first)
            want = [RS.first_output(first + i + 1, lout, up, down) - RS.first_output(first + i, lout, up, down) for i in range(33)]
            assert list(got) == want, (lout, up, down, first)
    v = (C.c_int32 * 4)(7, 7, 7, 7)
    for args in ((0, 1, 1, 0, 4), (8, 0, 1, 0, 4), (8, 65, 1, 0, 4), (8, 1, 0, 0, 4), (8, 1, 129, 0, 4), (8, 1, 1, -1, 4), (8, 1, 1, 0, -1), (8, 64, 1, 2 ** 62, 4)):
        assert lib.fdc_audio_resampler_counts(*args, v) == -1 and list(v) == [7] * 4, args
    assert lib.fdc_audio_resampler_counts(8, 1, 1, 0, 4, None) == -1 and lib.fdc_audio_resampler_counts(8, 1, 1, 0, 0, None) == 0


def test_the_padded_zero_taps_are_part_of_the_sum():
    """ntaps = 13 at up = 3 is padded to 15: phases 1 and 2 end in a zero tap, and a NaN or Inf under it gives NaN (0 x NaN, 0 x Inf), which a sum over
    the given taps alone would miss"""
    up, down, lout = 3, 2, 30
    h = np.arange(1, 14, dtype=F32)
    kp, hp = RS.phase_taps(h, up)
    assert kp == 5 and hp.shape == (3, 5) and hp[0].tolist() == [1, 4, 7, 10, 13] and hp[1].tolist() == [2, 5, 8, 11, 0] and hp[2].tolist() == [3, 6, 9, 12, 0]
    d = np.ones(lout, F32)
    d[10] = np.nan
    a = RS.resample32(d, h, up, down, lout)
    n = np.arange(a.size)
    newest, ph = n * down // up, n * down % up
    touched = (newest >= 10) & (newest - (kp - 1) <= 10)
    assert (np.isnan(a) == touched).all()
    at_pad = touched & (newest - (kp - 1) == 10) & (ph > 0)         # the NaN stands under the padded tap alone
    assert at_pad.any() and np.isnan(a[at_pad]).all()
    d[10] = np.inf
    a = RS.resample32(d, h, up, down, lout)
    assert np.isnan(a[at_pad]).all() and np.isinf(a[touched & ~at_pad]).all()


def test_the_order_of_the_sum():
    """taps [1, 2^-24, 2^-24] under ones give 1.0, reversed 1 + 2^-23; per phase at up = 2 likewise"""
    h3 = np.array([1.0, 2.0 ** -24, 2.0 ** -24], F32)
    ones = np.ones(64, F32)
    for h, full in ((h3, F32(1.0)), (h3[::-1].copy(), F32(1.0) + F32(2.0 ** -23))):
        two = np.repeat(h, 2)                               # both phases of up = 2 carry h
        a = RS.resample32(ones, two, 2, 1, 64)
        assert (a[4:] == full).all()
