"""TEST INFRASTRUCTURE — the plans, inputs and references of an end-to-end accuracy criterion for the kernels that never write a spectrum (k_blk256 /
512 / 1024, k_blknar, k_f4096, the two-launch forms): every form the block-kernel tests name, as data.  tests/test_fft_model_cpu.py uses it for the
seeded-defect demonstrations, profiles/accuracy/chain_factors.py to measure what factors a per-row bound on E would need (chain_K below; the answer,
in profiles/accuracy/README.md, is why no GPU test asserts on it yet).  Plain numpy and the oracle's window tables; nothing of the product in it
(flags are named; a GPU test would look the names up).

A Case is one plan and the kernel form it must run.  Reference(case, oracle) makes its runs — noise, impulses, exact-bin tones; quantised for the
integer-input forms — and, per run, the complex128 chain and E of every (block, channel) row, one model call per combination and channel group
(channels of one width, one window and one f mod R: a uniform bank is one group)."""
import numpy as np

import fft_model as M

WIN = (0.88, 1.0)           # (passband, stopband) of every bank
WINTYPE = 1


class Case:
    def __init__(self, kernel, name, N, R, chans, expect, path=3, flags=None, fmt=None, first_block=0, wintype=WINTYPE):
        self.kernel, self.name, self.N, self.R, self.chans = kernel, name, N, R, [tuple(c) for c in chans]
        self.expect, self.path, self.flags, self.fmt, self.first_block, self.wintype = expect, path, flags, fmt, first_block, wintype
        self.id = ("%s-%s" % (kernel, name)).replace(" ", "_")
        self.cut = [(f, l) for (f, l, _, _) in self.chans]

    def groups(self):
        """[(indices of the channels, (array of f, l), (passband, stopband))]: what one model call serves"""
        g = {}
        for c, (f, l, p, s) in enumerate(self.chans):
            g.setdefault((l, p, s, f % self.R), []).append(c)
        return [(idx, (np.array([self.chans[c][0] for c in idx]), key[0]), key[1:3]) for key, idx in g.items()]


def bank(N, l, r):
    """every slot of the l-bin raster moved up by r bins (the last slot would leave the band when r > 0)"""
    return [(l * c + r, l) + WIN for c in range(N // l - (1 if r else 0))]


def blk256_cases():
    out = []
    for N in (16384, 32768, 65536):                     # P = 2, 4, 8 passes: another table scheme each
        for form, R, r in (("grid", 2, 0), ("half", 2, 128), ("off37", 2, 37), ("grid", 4, 0)):
            out.append(Case("k_blk256", "N%d-%s-R%d" % (N, form, R), N, R, bank(N, 256, r), "k_blk256, 1 tiling (r = %d)" % r))
    out.append(Case("k_blk256", "N65536-grid-R2-sc16", 65536, 2, bank(65536, 256, 0), "k_blk256, 1 tiling (r = 0)", fmt="sc16"))     # the scalar-row form
    out.append(Case("k_blk256", "N32768-grid-R2-sc16", 32768, 2, bank(32768, 256, 0), "k_blk256, 1 tiling (r = 0)", fmt="sc16"))
    out.append(Case("k_blk256", "N65536-off37-R2-first1000001", 65536, 2, bank(65536, 256, 37), "k_blk256, 1 tiling (r = 37)", first_block=1000001))
    return out


def wide_cases():
    out = []
    for L in (512, 1024):
        for N in (16384, 32768, 65536):
            for form, R, r in (("grid", 2, 0), ("half", 2, L // 2)) + ((("grid", 4, 0),) if N == 65536 else ()):
                where = "half a channel off the grid" if r else "on the grid"
                out.append(Case("k_blk%d" % L, "N%d-%s-R%d" % (N, form, R), N, R, bank(N, L, r), ("k_blk%d" % L, where)))
    return out


def narrow_cases():
    out = []
    for L in (64, 128):
        for N in (65536, 16384):
            for form, r, where in (("grid", 0, "on the grid"), ("half", L // 2, "half a channel off the grid"),
                                   ("quarter", L // 4, "a quarter of a channel off the grid"),
                                   ("three-quarters", 3 * L // 4, "three quarters of a channel off the grid")):
                out.append(Case("k_blknar", "l%d-N%d-%s-R2" % (L, N, form), N, 2, bank(N, L, r), ("k_blknar", where)))
    return out


def fused_cases():
    """every plan of tests/test_fused4096_gpu.py at R = 2 and 4 (fine tuning off: that is another operation)"""
    from test_fused4096_gpu import plans
    out = []
    for i, (name, chans) in enumerate(plans().items()):
        for R in (2, 4):
            out.append(Case("k_f4096", "plan%02d-R%d" % (i, R), 4096, R, chans, "k_f4096", path=5))
    return out


def two_launch_cases():
    full = bank(65536, 256, 0)
    return [Case("k_p1+k_p2", "N65536-R2", 65536, 2, full, "two launches (stage 1 + stage 2), l = 256", path=2, flags=("NO_BLOCK",)),
            Case("k_a256+k_b256", "N65536-R2", 65536, 2, full, "forward transform to a spectrum in memory", path=1, flags=("NO_BLOCK", "NO_POLY"))]


def all_cases():
    return blk256_cases() + wide_cases() + narrow_cases() + fused_cases() + two_launch_cases()


# ---------------------------------------------------------------- runs and references
_forward = {}        # one entry: the spectra of the last (N, R, kind, format) whose stream does not depend on the channels


def _spectra(key, blocks, N, transforms):
    """{64: forward64, fwd: forward32 for fwd in transforms} of `blocks`; kept for the next case when key is not None"""
    if key is not None and _forward.get("key") == key:
        sp = _forward["spectra"]
    else:
        sp = {64: M.forward64(blocks, N)}
        if key is not None:
            _forward.clear()
            _forward.update(key=key, spectra=sp)
    for t in transforms:
        if t not in sp:
            sp[t] = M.forward32(blocks, N, t)
    return sp


class Run:
    """One call: the stream as the entry takes it (complex64, or integers and their scale), the samples it stands for, and the references"""

    def __init__(self, case, kind, j, stream, key):
        self.case, self.kind, self.j = case, kind, j
        if case.fmt:
            self.ints, self.scale = M.quantise(stream, 16 if case.fmt == "sc16" else 8)
            stream = ((self.ints[:, 0] * np.float32(self.scale)) + 1j * (self.ints[:, 1] * np.float32(self.scale))).astype(np.complex64)   # the widened samples
        self.stream = stream
        self.blocks = M.stream_blocks(stream, case.N, case.R)
        self.nb = self.blocks.shape[0]
        self.key = key
        self.what = "%s %s%s" % (case.name, kind, "" if j is None else " call %d" % j)

    def spectra(self, transforms=M.FLOAT32_MODELS):
        return _spectra(self.key, self.blocks, self.case.N, transforms)


class Reference:
    def __init__(self, case, oracle):
        self.case = case
        self.groups = case.groups()
        self.wins = [oracle.window(case.wintype, l, np.float32(p), np.float32(s), case.R) for (_, (_, l), (p, s)) in self.groups]

    def runs(self):
        c = self.case
        N, R = c.N, c.R
        yield Run(c, "noise", None, M.chain_noise_stream(N, R, N + R), (N, R, "noise", c.fmt))
        yield Run(c, "impulses", None, M.chain_impulse_stream(N, R), (N, R, "impulses", c.fmt))
        for j in range(M.chain_tone_calls(c.cut)):
            yield Run(c, "tones", j, M.chain_tone_stream(N, R, c.cut, j), None)

    def rows(self, run, extra=()):
        """per channel group: (channel indices, ref (nb, C, lout), E = (e_rms, e_max), {(fwd, inv): the float32 chain} for the model combinations
        and for every further (fwd, inv) pair of complex64 transforms in `extra`)"""
        c = self.case
        sp = run.spectra(tuple(M.FLOAT32_MODELS) + tuple(f for f, _ in extra))
        for (idx, chan, _), win in zip(self.groups, self.wins):
            ref = M.channel_stage64(sp[64], c.N, c.R, chan, win, c.first_block)
            ys = {}
            for fwd, inv in tuple(M.CHAIN_COMBINATIONS) + tuple(extra):
                ys[(fwd, inv)] = M.channel_stage32(sp[fwd], c.N, c.R, chan, win, c.first_block, transform=inv)
            es = [M.model_error(ys[k], ref) for k in M.CHAIN_COMBINATIONS]
            e = (np.max([a for a, _ in es], axis=0), np.max([b for _, b in es], axis=0))
            yield idx, ref, e, ys


# ---------------------------------------------------------------- what factors would a per-row criterion on E need?
def k_ratios(y, ref, e, floor_ulps=1.0):
    """error / E per row, (rms, max); 0 where the error is within one float32 ulp of the row's scale: a bound max(factor x E, ulp) passes such a row
    under ANY factor, so it says nothing about the factor."""
    rms, mx, top = M.item_errors(y, ref)
    one = np.where(top > 0, top, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.where(rms / one > floor_ulps * M.ULP, (rms / one) / e[0], 0.0),
                np.where(mx / one > floor_ulps * M.ULP, (mx / one) / e[1], 0.0))


def scipy_c64(x, inverse=False):
    """scipy.fft on complex64 (pocketfft in float32) with the signature of the float32 models: unnormalised both ways"""
    import scipy.fft as S
    x = np.asarray(x, dtype=np.complex64)
    y = S.ifft(x, axis=-1, norm="forward") if inverse else S.fft(x, axis=-1)
    assert y.dtype == np.complex64
    return y


def chain_K(case, oracle, floor_ulps=1.0):
    """(K_rms, its row, K_max, its row) of one case: the largest ratio of an independent correct float32 chain's error to E on any row —
    each of the four model combinations against the envelope of the other three; the scipy.fft complex64 chain and its mixtures with the models, and
    the oracle's compiled float32 chain (channelizer(use_float=True)), against the envelope of the four.  All channels, every run of the case."""
    ref_ = Reference(case, oracle)
    mixtures = [(scipy_c64, scipy_c64)] + [(scipy_c64, t) for t in M.FLOAT32_MODELS] + [(t, scipy_c64) for t in M.FLOAT32_MODELS]
    best = [0.0, "", 0.0, ""]

    def note(name, run, idx, r_l2, r_max):
        for i, r in ((0, r_l2), (2, r_max)):
            if r.max() > best[i]:
                m, c = np.unravel_index(int(np.argmax(r)), r.shape)
                best[i], best[i + 1] = float(r.max()), "%s %s block %d channel %d: %s" % (case.id, run.what, m, idx[c], name)

    for run in ref_.runs():
        outs, _ = oracle.channelizer(case.N, case.R, case.wintype, case.chans, run.stream, first_block=case.first_block, use_float=True, nthreads=8)
        for idx, ref, e, ys in ref_.rows(run, extra=mixtures):
            errs = {k: M.model_error(ys[k], ref) for k in M.CHAIN_COMBINATIONS}
            for k in M.CHAIN_COMBINATIONS:                                   # one against the envelope of the other three
                others = [errs[o] for o in M.CHAIN_COMBINATIONS if o != k]
                env = (np.max([a for a, _ in others], axis=0), np.max([b for _, b in others], axis=0))
                note("%s / %s against the other three" % (k[0].__name__, k[1].__name__), run, idx, *k_ratios(ys[k], ref, env, floor_ulps))
            for k in mixtures:
                note("%s / %s" % (k[0].__name__, k[1].__name__), run, idx, *k_ratios(ys[k], ref, e, floor_ulps))
            y = np.stack([outs[c].reshape(run.nb, ref.shape[-1]) for c in idx], axis=1)
            note("the oracle's float32 chain", run, idx, *k_ratios(y, ref, e, floor_ulps))
    return tuple(best)
