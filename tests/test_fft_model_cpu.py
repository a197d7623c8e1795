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


# ================================================================ the chain: block -> forward N -> shift, 1/N -> channel stage
# The yardstick of an end-to-end criterion for the kernels that never write a spectrum (fft_model.chain64 / chain32 over the plans and inputs of
# tests/block_accuracy_cases.py).  What is established here: it is the oracle's chain; a wrong inverse-table entry and a wrong early forward entry
# that pass 1e-5 on noise end to end stand far above E on the tone and impulse rows.  What could not be established: factors for a per-row bound
# (block_accuracy_cases.chain_K, profiles/accuracy/README.md).
import functools                           # noqa: E402

import block_accuracy_cases as BC          # noqa: E402


def test_chain_is_the_oracles_chain(oracle):
    """stream_blocks + chain64 against the oracle's own chain (its double-precision transforms, rounded to float between the blocks) on a stream with
    a first_block, channel by channel and as one bank call; the four chain32 combinations at float32 grade."""
    N, R, wt, first = 1024, 4, 2, 7
    H = N - N // R
    chans = [(64 * c + 33, 64, 0.6, 0.85) for c in range(15)]
    x = M.noise(6 * H, 9)
    outs, _ = oracle.channelizer(N, R, wt, chans, x, first_block=first)
    win = oracle.window(wt, 64, np.float32(0.6), np.float32(0.85), R)
    blocks = M.stream_blocks(x, N, R)
    assert blocks.shape == (6, N) and not blocks[0, :N // R].any() and (blocks[1, :N // R] == x[H - N // R:H]).all()
    fs = np.array([f for (f, _, _, _) in chans])
    bank = M.chain64(blocks, N, R, (fs, 64), win, first)
    assert bank.shape == (6, 15, 48)
    for c, (f, l, _, _) in enumerate(chans):
        one = M.chain64(blocks, N, R, (f, l), win, first)
        assert np.array_equal(one, bank[:, c])
        l2, mx = M.relative_errors(outs[c].reshape(6, 48), one)
        assert l2.max() <= 2e-7 and mx.max() <= 4e-7
    for fwd, inv in M.CHAIN_COMBINATIONS:
        y = M.chain32(blocks, N, R, (fs, 64), win, first, fwd, inv)
        assert y.dtype == np.complex64 and y.shape == bank.shape
        l2, mx = M.relative_errors(y, bank)
        assert l2.max() <= 4e-7 and mx.max() <= 8e-7
    e = M.chain_model_error(blocks, N, R, (fs, 64), win, first, bank)
    assert e[0].shape == e[1].shape == (6, 15) and (e[1] >= e[0]).all() and e[1].max() <= 8e-7
    assert M.relative_errors(M.chain64(blocks, N, R, (fs, 64), win, first + 1), bank)[0].min() > 1e-2          # the window row matters


def test_chain_streams():
    """the impulse stream puts block m + 1's impulse at impulse_positions(N)[m]; a tone stream's blocks behind the first transform to one impulse per
    slice; every slice position meets every residue of c mod 16 within chain_tone_calls calls; quantise is exact on its own grid"""
    N, R = 4096, 4
    pos = M.impulse_positions(N)
    blocks = M.stream_blocks(M.chain_impulse_stream(N, R), N, R)
    assert blocks.shape[0] == len(pos) + 1
    for m, p in enumerate(pos):
        assert blocks[m + 1, p] == 1.0
        assert np.count_nonzero(blocks[m + 1]) <= 3                      # its own, and a neighbour's on either side when that lies in the overlap
    cut = [(256 * c + 37, 256) for c in range(15)]
    calls = M.chain_tone_calls(cut)
    seen = set()
    for j in range(calls):
        spec = M.forward64(M.stream_blocks(M.chain_tone_stream(N, R, cut, j), N, R), N)
        for c, (f, l) in enumerate(cut):
            k = M.slice_positions(l)[(c + j) % len(M.slice_positions(l))]
            s = np.abs(spec[1:, f:f + l])
            assert np.allclose(s[:, k], 1.0, rtol=0, atol=1e-5)
            s[:, k] = 0
            assert s.max() <= 1e-5
            seen.add((k, c % 16))
    assert seen == set((k, c % 16) for k in M.slice_positions(256) for c in range(15))
    q, scale = M.quantise(M.noise(1000, 3))
    assert q.dtype == np.int16 and np.abs(q).max() > 8192
    again, scale2 = M.quantise((q[:, 0] + 1j * q[:, 1]) * scale)
    assert scale2 == scale and np.array_equal(again, q)


def _worst_over_E(ref_, runs, fwd, inv):
    """per input kind: (largest relative L2, largest max / max: the suite's present figures; largest rms error / E_rms and largest per-sample error /
    E_max over the rows more than one ulp off) of the chain with the transforms (fwd, inv)"""
    out = {}
    for run in runs:
        for idx, ref, e, ys in ref_.rows(run, extra=[(fwd, inv)]):
            l2, mx = M.relative_errors(ys[(fwd, inv)], ref)
            r_l2, r_max = BC.k_ratios(ys[(fwd, inv)], ref, e)
            w = out.setdefault(run.kind, [0.0] * 4)
            out[run.kind] = [max(a, float(b.max())) for a, b in zip(w, (l2, mx, r_l2, r_max))]
    return out


def _fmt(w):
    return "; ".join("%s: L2 %.2g max %.2g, rms %.1f x E, per sample %.1f x E" % ((k,) + tuple(v)) for k, v in w.items())


@pytest.mark.parametrize("which", ["k_blk256 N=65536", "k_f4096 full band"])
def test_seeded_defect_in_the_chain(oracle, which):
    """One twiddle entry rotated, in the forward or in the inverse model, end to end over a plan of the block-kernel tests (all channels, every input).
    Inverse entries (any stage) at 1e-5 rad: noise stays under the suite's 1e-5; the tone rows — one window value times the bare inverse tables —
    stand at least 16 x above E per sample, twice the largest factor a float32-grade criterion could have (8).
    Forward entries: only those of the EARLY stages show, the ones that reach many bins of one slice — (stage 1, index 1) at 3e-6 rad passes 1e-5 on
    noise and is at least 16 x E on an impulse row; an entry of a late stage reaches one bin in 2**stage, at most one per slice, and its 1e-5 arrives in
    the channel's output divided by about l: it stays within a few E (printed, not asserted: a limit of ANY end-to-end criterion)."""
    case = {"k_blk256 N=65536": BC.blk256_cases()[8], "k_f4096 full band": BC.fused_cases()[8]}[which]
    lgN, lgl = case.N.bit_length() - 1, case.chans[0][1].bit_length() - 1
    ref_ = BC.Reference(case, oracle)
    runs = list(ref_.runs())
    for stage, index in ((lgl - 1, 1), (lgl - 1, (1 << lgl) // 4 + 3), (lgl // 2, 1), (1, 1), (lgl - 2, 5)):
        w = _worst_over_E(ref_, runs, M.fft32_model, functools.partial(M.fft32_model, defect=(stage, index, 1e-5)))
        print("%s inverse defect %s 1e-5: %s" % (case.id, (stage, index), _fmt(w)))
        assert w["noise"][0] <= 1e-5 and w["noise"][1] <= 1e-5, (stage, index, w)
        assert w["tones"][3] >= 16, (stage, index, w)
    w = _worst_over_E(ref_, runs, functools.partial(M.fft32_model, defect=(1, 1, 3e-6)), M.fft32_model)
    print("%s forward defect (1, 1) 3e-6: %s" % (case.id, _fmt(w)))
    assert w["noise"][0] <= 1e-5 and w["noise"][1] <= 1e-5, w
    assert w["impulses"][3] >= 16, w
    for stage, index in ((lgN - 1, 1), (lgN // 2, 1)):
        w = _worst_over_E(ref_, runs, functools.partial(M.fft32_model, defect=(stage, index, 1e-5)), M.fft32_model)
        print("%s forward defect %s 1e-5 (late stage: diluted by l): %s" % (case.id, (stage, index), _fmt(w)))
        assert w["noise"][0] <= 1e-5 and w["noise"][1] <= 1e-5, w


def test_chain_K_measurement_runs(oracle):
    """block_accuracy_cases.chain_K (what profiles/accuracy/chain_factors.py prints for every case) on one small plan: it names a row for both figures.
    The figures themselves are a record, not a bound: see profiles/accuracy/README.md for why no factor follows from them."""
    pytest.importorskip("scipy.fft")
    k_rms, row_rms, k_max, row_max = BC.chain_K(BC.fused_cases()[0], oracle)
    print("CHAIN_K K_rms=%.3f (%s) K_max=%.3f (%s)" % (k_rms, row_rms, k_max, row_max))
    assert np.isfinite([k_rms, k_max]).all() and k_rms > 0 and k_max > 0 and "block" in row_rms and "block" in row_max
