"""GPU tests (-m gpu): the generic LDS transform core (fft_cols, csrc/fdc_kernels.hip) and everything wrapped around it, held to float32-grade error.

One property: the error against a complex128 evaluation of the same operation (tests/fft_model.py: dft64, channel_stage64), per item or per (block,
channel) row, is at most a multiple of the error of a textbook float32 radix-2 transform (fft32_model, channel_stage32) on the same input:
    rms error <= 2 x the model's,  largest per-sample error <= 3 x the model's,  each at least 2**-23 * max|ref| (one float32 ulp at the output's scale).
The factors are those of two independent CPU float32 transforms against each other (tests/test_fft_model_cpu.py), not tuned to the device.  "The
model's" error on a row is the larger of two: the radix-2 model's and that of fft32_model_steps, which takes the roundings a radix-16 / two-pass
transform legitimately takes (two table products per input, W16 constants, the W_n product between the passes; tests/fft_model.py says why).  Inputs:
noise, unit impulses (the output is the bare table products: one wrong entry or one mis-folded twiddle index shows in full, where noise averages it
under 1e-5) and exact-bin tones.

Part A  the fdc_fft_vcc face: every n = 2 ... 2^24 in its four (forward, shift) forms — k_fft_small (n <= 2048 and 8192), k_fft4096, k_fft_pass_a/b
        (every split N1 x N2, the odd powers' N1 = 2 N2 included) — with item counts that fill two tiles and a ragged third.
Part B  the channel stage on its own, through Pipeline.work_spectrum (items in, 1/N — exact — and the channel kernels only):
        B1 k_channels<1> at every l = 1 ... 4096, B2 k_c256, B3 k_c512 / k_c1024 (from the spectrum work() itself returns), B4 the task-addressed
        two-pass inverse transform of the widths above 4096.
(k_channels<2> has no caller: every entry sends l > 4096 to the two-pass tasks — run_channel_groups, fdc_enqueue.hip, and fdc_pipeline_work_spectrum.)

Every test prints its largest ratios to the model ("ACCURACY ..." lines, pytest -s): DESIGN.md §6 and profiles/accuracy/README.md hold the table."""
import numpy as np
import pytest

import fft_model as M
import gr_fdc_amd as G
from gr_fdc_amd import _lib

pytestmark = pytest.mark.gpu

FORMS = [(inverse, shift) for inverse in (False, True) for shift in (False, True)]


def report(kernel, what, r_l2, r_max):
    print("ACCURACY kernel=%s %s l2_ratio=%.3f max_ratio=%.3f" % (kernel, what, float(np.max(r_l2)), float(np.max(r_max))))


def check(kernel, what, y, ref, e_model):
    """the criterion on every row of y; returns the two largest ratios"""
    r_l2, r_max = M.ratios(y, ref, e_model)
    report(kernel, what, r_l2, r_max)
    i, j = int(np.argmax(r_l2)), int(np.argmax(r_max))
    assert r_l2.max() <= M.L2_FACTOR, "%s %s: row %d rms error %.2f x the model's (bound %g)" % (kernel, what, i, r_l2.max(), M.L2_FACTOR)
    assert r_max.max() <= M.MAX_FACTOR, "%s %s: row %d largest error %.2f x the model's (bound %g)" % (kernel, what, j, r_max.max(), M.MAX_FACTOR)
    return float(r_l2.max()), float(r_max.max())


# ================================================================ part A: fdc_fft_vcc
SIZES = [1 << k for k in range(1, 25)]


def face_kernel(n):
    return "k_fft4096" if n == 4096 else "k_fft_small" if n <= 8192 else "k_fft_pass_a/b"


def item_counts(n):
    """items per call: a lone item, and two full tiles and a ragged third of the TC = min(32, 4096 / n) items a workgroup of k_fft_small takes"""
    if n <= 2048:
        return (1, 2 * min(32, 4096 // n) + 3)
    if n == 4096:
        return (1, 9)
    if n == 8192:
        return (3,)                      # k_fft_small<., 2>, one item per workgroup
    return (2,) if n <= 1 << 20 else (1,)


def face_input(n, kind):
    """(rows, items per call of every call to make): all rows go through the face in calls of the listed sizes"""
    counts = item_counts(n)
    if kind == "noise":
        return M.noise((max(counts), n), n), counts
    if kind == "tone":
        ks = [(3 * n) // 8 + 1, n - 1, 1][:min(counts)] if n > 2 else [1]
        return np.stack([M.tone(n, k % n) for k in ks]), (len(ks),)
    if n <= 1 << 16:
        pos = M.impulse_positions(n)                 # one impulse per item
    else:
        pos = M.wide_impulse_positions(n, 4 if n <= 1 << 22 else 2)
    per = max(counts)
    pos = (pos * per)[:-(-len(pos) // per) * per]    # whole calls: the walk starts over
    return M.impulses(n, pos), (per,)


_model_errors = {}


def face_model_error(n, kind, x, fwd_ref):
    """E_model of (n, input): once, on the forward unshifted transform, for all four forms; kept for the process above 2^20 (seconds per item there)"""
    if (n, kind) in _model_errors:
        return _model_errors[(n, kind)]
    e = M.transform_model_error(x, fwd_ref)
    if n > 1 << 20:
        _model_errors[(n, kind)] = e
    return e


@pytest.mark.parametrize("kind", ["noise", "impulse", "tone"])
@pytest.mark.parametrize("n", SIZES)
def test_fft_vcc_against_the_float32_model(n, kind):
    x, counts = face_input(n, kind)
    refs = M.dft64_forms(x)
    e_model = face_model_error(n, kind, x, refs[(False, False)])
    for inverse, shift in FORMS:
        ref = refs[(inverse, shift)]
        for c in counts:
            for r0 in (range(0, x.shape[0], c) if c == max(counts) else [0]):
                y = G.fft_vcc(n, not inverse, shift, x[r0:r0 + c])
                assert y.shape == (c, n) and y.dtype == np.complex64
                check(face_kernel(n), "n=%d %s inverse=%d shift=%d items=%d row0=%d" % (n, kind, inverse, shift, c, r0), y, ref[r0:r0 + c],
                      (e_model[0][r0:r0 + c], e_model[1][r0:r0 + c]))


# ================================================================ part B: the channel stage
BANDWIDTHS = [(0.6, 0.85), (0.88, 1.0), (1.0, 1.0), (0.3, 0.5)]      # (passband, stopband); 1.0 / 1.0: the rectangular window


class ChannelCase:
    """One plan: the references of its channels from the ORACLE's window tables (never the product's), block counter included."""

    def __init__(self, oracle, N, R, wintype, chans):
        self.N, self.R, self.chans = N, R, chans
        self.cut = [(f, l) for (f, l, _, _) in chans]
        self.wins = [oracle.window(wintype, l, np.float32(p), np.float32(s), R) for (_, l, p, s) in chans]

    def check(self, kernel, what, spec, outs, first_block):
        """spec: the (nb, N) complex64 array the channel kernels read (1/N applied); outs: the device's channel streams of this call"""
        nb = spec.shape[0]
        worst = [0.0, 0.0]
        for c, (f, l) in enumerate(self.cut):
            ref = M.channel_stage64(spec, self.N, self.R, (f, l), self.wins[c], first_block)
            e_model = M.channel_model_error(spec, self.N, self.R, (f, l), self.wins[c], first_block, ref)
            y = outs[c].reshape(nb, l - l // self.R)
            r = check(kernel, "%s R=%d ch%d f=%d l=%d first_block=%d" % (what, self.R, c, f, l, first_block), y, ref, e_model)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
        return worst


def run_work_spectrum(oracle, kernel, N, R, wintype, chans, nb, calls, flags=None):
    """noise, then (after a reset) impulses through work_spectrum: `calls` calls of nb items each on one handle, the block counter running on"""
    case = ChannelCase(oracle, N, R, wintype, chans)
    p = G.Pipeline(N, R, chans, windowtype=wintype, max_blocks=nb, flags=flags)
    inv_n = np.float32(1.0 / N)                                 # multiply_const(1/N): a power of two, exact
    for kind in ("noise", "impulse"):
        p.reset()
        for k in range(calls):
            first = k * nb
            items = M.channel_noise_items(N, first, nb, N + R + first) if kind == "noise" else M.channel_impulse_items(N, case.cut, first, nb)
            outs = p.work_spectrum(items)
            case.check(kernel, "N=%d %s" % (N, kind), items * inv_n, outs, first)
    p.close()


@pytest.mark.parametrize("R", [2, 4, 8, 16])
def test_k_channels_every_width(oracle, R):
    """B1: k_channels<1> (FDC_PIPE_FORCE_GENERIC: 256 goes the generic way too) at every l = 1 ... 4096 — all four log2 l mod 4 tails of fft_cols,
    every TC from 32 down to 1 — three channels per width (f = 0, f = N - l, an odd f whose f mod R differs from width to width), the widths l < R
    where nothing is discarded, the window types rotated over the widths, 11 blocks (33 transforms: two tiles and a ragged one at TC = 32) and a
    second call whose counter continues at 11, so that every window row occurs for every R."""
    N = 4096
    for i in range(13):
        l = 1 << i
        fs = [0] if l == N else [0, N - l, (2 * i + 1) + 32 * (i + 1)]
        chans = [(f, l) + BANDWIDTHS[(i + c) % 4] for c, f in enumerate(fs)]
        run_work_spectrum(oracle, "k_channels<1>", N, R, (i + R.bit_length()) % 3, chans, 11, 2, flags=_lib.FDC_PIPE_FORCE_GENERIC)


@pytest.mark.parametrize("R", [2, 4, 8, 16])
def test_k_c256(oracle, R):
    """B2: l = 256 with default flags (fdc_pipeline_work_spectrum sends it to k_c256): five channels, 7 blocks (35 rows over workgroups of 32), three
    calls on one handle (every window row for R = 16)."""
    N = 4096
    chans = [(f, 256) + BANDWIDTHS[c % 4] for c, f in enumerate([0, 1, 255, N - 256, 1365])]
    run_work_spectrum(oracle, "k_c256", N, R, R.bit_length() % 3, chans, 7, 3)


@pytest.mark.parametrize("R", [2, 4])
def test_k_c512_k_c1024(oracle, R):
    """B3: k_c512 / k_c1024 are not reachable through work_spectrum; work(x, want_spectrum=True) of a plan without block, uniform or fused kernels runs
    them on the spectrum it returns.  The reference is computed from THAT spectrum, so the forward transform's own error is outside the comparison:
    with a spectrum asked for, process_device_impl (fdc_enqueue.hip) has launch_fft write it — fftshift and 1/N in its store — into the call's
    whole-call buffer, run_channel_groups reads that very buffer (l = 512 / 1024 -> launch_channels_wide), and pipeline_work_impl (fdc_work.hip)
    copies the same buffer to the host behind them.  6 blocks x 3 channels: 18 rows against 16 (k_c512) and 8 (k_c1024) per workgroup."""
    N, nb = 4096, 6
    H = N - N // R
    chans = [(f, l) + BANDWIDTHS[(c + k) % 4] for k, l in enumerate((512, 1024)) for c, f in enumerate([0, N - l, 1365 + 2 * k])]
    wintype = R.bit_length() % 3
    case = ChannelCase(oracle, N, R, wintype, chans)
    flags = _lib.FDC_PIPE_NO_POLY | _lib.FDC_PIPE_NO_FUSED | _lib.FDC_PIPE_FULL_SPECTRUM
    t = np.arange(nb * H)
    tones = np.zeros(nb * H, dtype=np.complex128)
    for c, (f, l) in enumerate(case.cut):                       # one exact-bin tone inside every slice: the spectrum is impulses (and the forward
        k = f + M.slice_positions(l)[2 + c]                     # transform's rounding elsewhere), each output row nearly a pure exponential
        tones += np.exp(2j * np.pi * (((k - N // 2) * t) % N) / N)
    seg = np.repeat(M.block_scale(np.arange(nb)), H)            # the samples block m brings, times block_scale(m)
    for kind, x in (("noise", M.noise(nb * H, N + R) * seg), ("tones", tones.astype(np.complex64))):
        p = G.Pipeline(N, R, chans, windowtype=wintype, max_blocks=nb, keep_spectrum=True, flags=flags)
        outs, spec = p.work(x, want_spectrum=True)
        d = p.describe()
        # describe() names the route, not each channel kernel: "a spectrum in memory + channel kernels" is run_channel_groups, which without
        # FDC_PIPE_FORCE_GENERIC sends l = 512 and l = 1024 (<= N) to launch_channels_wide, that is k_c512 and k_c1024, and nothing else of this plan
        assert "channel kernels" in d and "k_f4096" not in d and "k_blk" not in d and "two launches" not in d, d
        case.check("k_c512/k_c1024", "N=%d %s" % (N, kind), spec.reshape(nb, N), outs, 0)
        p.close()


def test_wide_two_pass_tasks(oracle):
    """B4: the widths above 4096 (k_wide_tasks + k_fft_pass_a/b<true, 1, TASK>): 8192 (128 x 64) twice, 16384, 32768 and 65536 at the band's edges
    and the whole band 131072 (512 x 256: an odd power).  2 blocks per call, five calls on one handle: ten steps of the impulse walk."""
    N, R = 131072, 2
    chans = [(0, 8192), (12345, 8192), (N - 16384, 16384), (0, 32768), (N - 65536, 65536), (0, N)]
    chans = [c + BANDWIDTHS[i % 4] for i, c in enumerate(chans)]
    run_work_spectrum(oracle, "two-pass tasks", N, R, 1, chans, 2, 5)
