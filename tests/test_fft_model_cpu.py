"""The yardstick of tests/test_transform_accuracy_gpu.py (tests/fft_model.py) on the CPU: that fft32_model (and fft32_model_steps, the same with the
roundings of a radix-16 / two-pass transform) is a sound float32 transform — against the
complex128 reference and against an independent float32 transform (scipy.fft on complex64) — and that the criterion built on it sees one wrong table
entry which the suite's present criterion (relative L2 and max|err| / max|ref| <= 1e-5 on noise, tests/test_parity_gpu.py) cannot.  Nothing on the
GPU is ever broken to see that: the defect is seeded into the model.

Measured here (seeded inputs, 65536 points per size up to n = 65536, one item above):
  noise      relative L2 of fft32_model 2.7e-8 (n = 2) ... 1.7e-7 (n = 2^21): 0.46 - 0.63 x 2^-24 sqrt(log2 n) at every size
  impulses   largest per-sample error 0 (n = 2, 4), 1.7e-8 (n = 8), 2.7e-7 (n = 4096), 4.1e-7 (n = 65536), 5.6e-7 (n = 2^21, two-pass positions)
  scipy.fft  its complex64 transform and fft32_model within 1.03 x of each other in L2 and within 1.26 x in per-sample max, either way, at every size
  one twiddle rotated by 1e-5 rad, n = 4096 and 65536: noise L2 <= 5.2e-6, max <= 7.6e-6 (passes 1e-5); the impulse through the entry is 23 - 84 x
  the per-sample bound."""
import numpy as np
import pytest

import fft_model as M

SIZES = [1 << k for k in range(1, 22)]
U = 2.0 ** -24                      # float32 unit roundoff


def batch(n):
    """items of one size: 65536 points' worth, so that the figures of a small n are not one draw"""
    return max(1, 65536 // n)


def aggregate(y, ref):
    """(relative L2 over all items together, largest per-sample error over max|ref|)"""
    d = np.abs(y.astype(np.complex128) - ref)
    return float(np.sqrt((d * d).sum() / (np.abs(ref) ** 2).sum())), float(d.max() / np.abs(ref).max())


def test_dft64_has_fft_vcc_shift_semantics():
    """forward + shift swaps the output halves, inverse + shift the input halves, unnormalised both ways (tests/test_oracle.py::test_fft_vcc_matches_numpy)"""
    x = M.noise((3, 64), 1)
    xd = x.astype(np.complex128)
    k = np.arange(64)
    F = np.exp(-2j * np.pi * np.outer(k, k) / 64)
    assert np.allclose(M.dft64(x), xd @ F.T, rtol=0, atol=1e-11)
    assert np.allclose(M.dft64(x, shift=True), np.roll(xd @ F.T, 32, axis=1), rtol=0, atol=1e-11)
    assert np.allclose(M.dft64(x, inverse=True), xd @ F.conj().T, rtol=0, atol=1e-11)
    assert np.allclose(M.dft64(x, inverse=True, shift=True), np.roll(xd, 32, axis=1) @ F.conj().T, rtol=0, atol=1e-11)
    assert M.dft64(x[0]).shape == (64,)


def test_dft64_forms_equal_dft64():
    """the four forms from two transforms (the test of the largest sizes pays for two, not four)"""
    for n in (2, 4, 64, 4096):
        x = M.noise((2, n), n)
        forms = M.dft64_forms(x)
        for inverse in (False, True):
            for shift in (False, True):
                ref = M.dft64(x, inverse, shift)
                assert np.abs(forms[(inverse, shift)] - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("model", M.FLOAT32_MODELS, ids=lambda t: t.__name__)
@pytest.mark.parametrize("n", SIZES)
def test_model_against_dft64(n, model):
    """The model (radix 2; and fft32_model_steps) is a float32 transform: lg = log2 n stages' worth of butterflies, each stage adds an independent
    relative error of at most one unit roundoff (rms) to every point, so the relative L2 error on noise stays under 2^-24 sqrt(lg); an impulse's output bin is a product of lg rounded twiddles, the same walk, and no
    bin of any impulse is further out than four standard deviations of it.  Inverse = the conjugate tables: the same figures."""
    lg = n.bit_length() - 1
    x = M.noise((batch(n), n), n)
    for inverse in (False, True):
        l2, mx = aggregate(model(x, inverse), M.dft64(x, inverse))
        print("n=2^%d inverse=%d noise: L2 %.3g = %.2f u sqrt(lg), max %.3g" % (lg, inverse, l2, l2 / (U * np.sqrt(lg)), mx))
        assert 0 < l2 <= U * np.sqrt(lg)
    pos = M.impulse_positions(n) if n <= 65536 else M.wide_impulse_positions(n)
    xi = M.impulses(n, pos)
    for inverse in (False, True):
        _, mx = aggregate(model(xi, inverse), M.dft64(xi, inverse))
        print("n=2^%d inverse=%d impulses: max %.3g" % (lg, inverse, mx))
        assert mx <= 4 * U * np.sqrt(lg)
        if n <= 4:
            assert mx <= 1e-15                     # twiddles 1 and -+i only: exact (the criterion's one-ulp floor is for this)
    t = M.tone(n, (3 * n) // 8 + 1 if n > 2 else 1)
    k = (3 * n) // 8 + 1 if n > 2 else 1
    y = model(t)
    assert abs(y[k] - n) <= 4 * U * np.sqrt(lg) * n
    y[k] = 0
    assert np.abs(y).max() <= 4 * U * np.sqrt(lg) * n


@pytest.mark.parametrize("model", M.FLOAT32_MODELS, ids=lambda t: t.__name__)
def test_model_accepts_any_leading_shape(model):
    for n in (32, 16384):
        x = M.noise((2, 3, n), 5)
        y = model(x)
        assert y.shape == x.shape and y.dtype == np.complex64
        assert (y[1, 2] == model(x[1, 2])).all()
    assert (model(x[0, 0, :1]) == x[0, 0, :1]).all()


@pytest.mark.parametrize("model", M.FLOAT32_MODELS, ids=lambda t: t.__name__)
@pytest.mark.parametrize("n", SIZES)
def test_model_against_an_independent_float32_transform(n, model):
    """scipy.fft computes a complex64 transform in float32 (pocketfft: radix 4 / 2 passes, its own twiddles): the two agree within 1.5 x in L2 and
    2 x in per-sample max, in either direction — where the factors 2 and 3 of the criterion come from."""
    S = pytest.importorskip("scipy.fft")
    x = M.noise((batch(n), n), n + 1)
    ys = S.fft(x, axis=-1)
    if ys.dtype != np.complex64:
        pytest.skip("this scipy.fft does not compute complex64 in float32")
    ref = M.dft64(x)
    l2m, mxm = aggregate(model(x), ref)
    l2s, mxs = aggregate(ys, ref)
    print("n=2^%d model L2 %.3g max %.3g, scipy L2 %.3g max %.3g: ratios %.2f %.2f" % (n.bit_length() - 1, l2m, mxm, l2s, mxs, l2m / l2s, mxm / mxs))
    assert l2m <= 1.5 * l2s and l2s <= 1.5 * l2m
    assert mxm <= 2 * mxs and mxs <= 2 * mxm


def test_channel_stage_is_the_composition_of_the_blocks(oracle):
    """channel_stage64 / channel_stage32 against the oracle's own blocks composed as tests/test_oracle.py::test_chain_blockwise_equals_composed_blocks
    composes them, first_block and an odd f included."""
    N, R, wt = 1024, 4, 2
    f, l, p, s = 301, 64, 0.6, 0.85
    spec = M.noise((7, N), 3)
    win = oracle.window(wt, l, np.float32(p), np.float32(s), R)
    pw = oracle.PhaseWindow(l, R, f, p, s, wt)
    pw.work(np.zeros(5 * l, np.complex64))                          # the counter stands at block 5
    c = oracle.vector_cut(8, N, f, l, spec)
    t = oracle.fft_vcc(l, False, True, pw.work(c))
    lout = l - l // R
    z = (oracle.vector_cut(8, l, l - lout, lout, t) * np.float32(l)).reshape(7, lout)
    r64 = M.channel_stage64(spec, N, R, (f, l), win, first_block=5)
    r32 = M.channel_stage32(spec, N, R, (f, l), win, first_block=5)
    assert r64.shape == r32.shape == (7, lout) and r32.dtype == np.complex64
    for y in (z, r32):
        l2, mx = M.relative_errors(y, r64)
        assert l2.max() <= 2e-7 and mx.max() <= 4e-7
    assert M.relative_errors(M.channel_stage64(spec, N, R, (f, l), win, first_block=4), r64)[0].min() > 1e-2     # the window row matters


@pytest.mark.parametrize("n", [4096, 65536])
def test_seeded_defect_passes_the_old_criterion_and_fails_the_new(n):
    """One twiddle entry rotated by 1e-5 rad.  On noise every output sample averages over every entry: relative L2 and max / max stay under the 1e-5
    of tests/test_parity_gpu.py.  An impulse's output is the bare table products: the impulse whose path runs through the entry shows the whole 1e-5 at
    the affected bins, at least 10 x the per-sample bound of the new criterion (3 x the clean models' error on the same item, one ulp at least)."""
    lg = n.bit_length() - 1
    xn = M.noise((3, n), n)
    rn = M.dft64(xn)
    xi = M.impulses(n, M.impulse_positions(n))
    ri = M.dft64(xi)
    clean = M.transform_model_error(xi, ri)                          # the criterion's E_model: the larger of the two models' errors per item
    r_l2, r_max = M.ratios(M.fft32_model(xi), ri, clean)
    assert r_l2.max() <= 1.0 and r_max.max() <= 1.0                 # (the clean model against its own error: the method's zero point)
    for stage, index in ((lg - 1, 1), (lg - 1, n // 4 + 3), (lg // 2, 1), (1, 1), (lg - 2, 5)):
        defect = (stage, index, 1e-5)
        l2, mx = M.relative_errors(M.fft32_model(xn, defect=defect), rn)
        assert l2.max() <= 1e-5 and mx.max() <= 1e-5, (defect, l2.max(), mx.max())          # the suite's present criterion: passes
        r_l2, r_max = M.ratios(M.fft32_model(xi, defect=defect), ri, clean)
        worst = r_max.max() / M.MAX_FACTOR
        print("n=%d defect %s: noise L2 %.3g max %.3g; impulses: worst item %.1f x its per-sample bound, %.1f x its L2 bound" % (
            n, defect, l2.max(), mx.max(), worst, r_l2.max() / M.L2_FACTOR))
        assert worst >= 10, (defect, worst)                                                 # the new one: fails, by 10 x at least
