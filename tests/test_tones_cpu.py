"""CPU tests of the channel tones' DEFINITION (tests/tones_model.py) and of the library's reference table: the vectorised model against a plain triple
loop, every cut of a stream, the phase beyond the 2^32 group wrap, values that are not finite, the extreme group lengths, and what the numbers mean
(a CTCSS tone's amplitude recovered, the right tone found in noise)."""
import itertools

import numpy as np
import pytest

import gr_fdc_amd as G
import tones_model as M


def same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "%s: %d of %d values differ" % (what, int(np.count_nonzero(a != b)), a.size)


def same_but_nan(a, b, what):
    """byte for byte, except that a NaN is a NaN: the sign and payload of a generated NaN are the platform's, not the definition's"""
    fa, fb = a.view(np.float32), b.view(np.float32)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert (np.isnan(fa) == np.isnan(fb)).all(), what
    same_bytes(np.where(np.isnan(fa), np.float32(0), fa), np.where(np.isnan(fb), np.float32(0), fb), what)


def lib_table():
    return G.tone_table()


def seeded(nb, lout, T, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(nb * lout).astype(np.float32), rng.integers(0, 1 << 32, T, dtype=np.uint64).astype(np.uint32)


def compositions(n):
    """every way to cut n blocks into calls, in order"""
    for k in range(n):
        for bars in itertools.combinations(range(1, n), k):
            edges = (0,) + bars + (n,)
            yield tuple(b - a for a, b in zip(edges, edges[1:]))


# ---- the library's table ------------------------------------------------------------------------------------------------------------------------------

def test_the_librarys_table():
    tab = lib_table()
    assert tab.shape == (1024, 2) and tab.dtype == np.float32
    assert tab[0].tolist() == [1, 0] and tab[256].tolist() == [0, 1] and tab[512].tolist() == [-1, 0] and tab[768].tolist() == [0, -1]
    assert not np.signbit(tab[[0, 256, 512, 768]][tab[[0, 256, 512, 768]] == 0]).any()            # (the zeros are +0)
    a = 2.0 * np.pi * np.arange(1024, dtype=np.float64) / 1024
    for col, ref in ((0, np.cos(a)), (1, np.sin(a))):
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        axis = np.arange(1024) % 256 == 0
        assert (np.abs(tab[:, col].astype(np.float64) - ref)[~axis] <= ulp[~axis]).all()
        assert (np.abs(tab[:, col].astype(np.float64) - ref)[axis] <= 1e-15).all()                # (exact: float64 cos(pi / 2) is 6e-17, not 0)
    assert _lib_null_refused()


def _lib_null_refused():
    from gr_fdc_amd import _lib
    return _lib.lib().fdc_tone_table(None) != 0


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lout,S,W,T,nb,first,fill", [(24, 4, 3, 5, 7, 0, 0), (16, 1, 2, 3, 5, 11, 1), (12, 12, 4, 2, 9, 3, 3), (40, 8, 1, 64, 3, 0, 0)])
def test_vectorised_equals_the_triple_loop(lout, S, W, T, nb, first, fill):
    d, inc = seeded(nb, lout, T, 100 * lout + S)
    tab = lib_table()
    rng = np.random.default_rng(5)
    carry = (rng.standard_normal(T) + 1j * rng.standard_normal(T)).astype(np.complex64)
    a = M.tones(d, lout, inc, S, W, tab, first, fill, carry)
    b = M.tones_loops(d, lout, inc, S, W, tab, first, fill, carry)
    same_bytes(a[0], b[0], "the rows")
    assert a[1] == b[1] == (fill + nb) % W and a[0].shape[0] == (fill + nb) // W
    same_bytes(a[2], b[2], "the carry")
    assert np.abs(a[0]).min() > 0 if a[0].size else True


@pytest.mark.parametrize("W", (1, 2, 4, 9, 12))
def test_every_cut_of_a_stream(W):
    """all 256 cuts of a 9-block stream concatenate to the one-call result, rows and final carry, from fill 0 and from a carried fill"""
    lout, S, T, nb = 16, 4, 3, 9
    d, inc = seeded(nb, lout, T, 40 + W)
    tab = lib_table()
    rng = np.random.default_rng(W)
    for first, fill in ((0, 0), (5, W - 1)):
        carry = (rng.standard_normal(T) + 1j * rng.standard_normal(T)).astype(np.complex64)
        whole, wfill, wcarry = M.tones(d, lout, inc, S, W, tab, first, fill, carry)
        assert whole.shape[0] == (fill + nb) // W
        seen_empty = False
        for cut in compositions(nb):
            rows, f, c, b = [], fill, carry, 0
            for n in cut:
                z, f, c = M.tones(d[b * lout:(b + n) * lout], lout, inc, S, W, tab, first + b, f, c)
                seen_empty = seen_empty or z.shape[0] == 0
                rows.append(z)
                b += n
            same_bytes(np.concatenate(rows), whole, "cut %r" % (cut,))
            assert f == wfill
            same_bytes(c, wcarry, "carry behind cut %r" % (cut,))
        assert seen_empty or W == 1


def test_the_phase_beyond_the_group_wrap():
    """first_block * G beyond 2^32 (and a run that crosses a multiple of 2^32): the phase is that of the exact integer product"""
    lout, S, W, T, nb = 8, 2, 2, 4, 4
    G_ = lout // S
    d, inc = seeded(nb, lout, T, 9)
    inc[0] = 0xFFFFFFFF
    inc[1] = 1 << 22
    tab = lib_table()
    for first in ((1 << 32) // G_ + 12345, (1 << 32) // G_ - 2, (1 << 40) + 7):
        g0 = first * G_
        assert g0 + nb * G_ > (1 << 32)
        k = M.phases(inc, g0, nb * G_)
        for j in range(nb * G_):
            for t in range(T):
                assert k[j, t] == ((int(inc[t]) * (g0 + j)) % (1 << 32)) >> 22
        same_bytes(M.tones(d, lout, inc, S, W, tab, first)[0], M.tones_loops(d, lout, inc, S, W, tab, first)[0], "first_block %d" % first)
    # ... and it matters: the rows differ from those at first_block mod 2^32 / G only where inc g wraps differently, never for a 32-bit-periodic phase
    a = M.tones(d, lout, inc, S, W, tab, (1 << 32) // G_ * 3 + 5)[0]
    b = M.tones(d, lout, inc, S, W, tab, 5)[0]
    same_bytes(a, b, "g and g + 3 * 2^32 give the same phase")


def test_values_that_are_not_finite():
    lout, S, W, T, nb = 16, 4, 2, 3, 4
    d, inc = seeded(nb, lout, T, 3)
    inc[0] = 0                                # (cs = 1, sn = +0: re takes the sums as they are, im sees u * 0)
    d[5], d[20], d[21], d[40] = np.nan, np.inf, -np.inf, np.inf
    tab = lib_table()
    a, b = M.tones(d, lout, inc, S, W, tab), M.tones_loops(d, lout, inc, S, W, tab)
    same_but_nan(a[0], b[0], "rows with NaN and Inf")
    assert np.isnan(a[0][0, 0].real) and np.isnan(a[0][0, 0].imag)           # NaN in frame 0; Inf - Inf = NaN in the same frame (blocks 0, 1)
    assert np.isposinf(a[0][1, 0].real) and np.isnan(a[0][1, 0].imag)        # +Inf alone in frame 1: re = Inf, im = 0 - Inf * 0 = NaN
    assert np.isfinite(a[2]).all()


def test_extreme_group_lengths():
    lout, W, T, nb = 24, 2, 4, 4
    d, inc = seeded(nb, lout, T, 77)
    tab = lib_table()
    for S in (1, lout):
        a, b = M.tones(d, lout, inc, S, W, tab), M.tones_loops(d, lout, inc, S, W, tab)
        same_bytes(a[0], b[0], "S = %d" % S)
    # S = lout, inc = 0: the row is the sequential float32 sum of the frame's block sums
    z = M.tones(d, lout, np.zeros(1, np.uint32), lout, W, tab)[0]
    s = [np.float32(0)] * nb
    for m in range(nb):
        for v in d[m * lout:(m + 1) * lout]:
            s[m] = np.float32(s[m] + v)
    assert z[0, 0].real == np.float32(np.float32(np.float32(0) + s[0]) + s[1]) and z[1, 0].real == np.float32(np.float32(np.float32(0) + s[2]) + s[3])
    # the order of the group sum shows: 1 + 2^-24 + 2^-24 + 2^-24 is 1 ascending and more than 1 descending
    row = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], np.float32)
    assert M.group_sums(row, 4)[0] == np.float32(1.0) and M.group_sums(row[::-1].copy(), 4)[0] > np.float32(1.0)


# ---- what the numbers mean ----------------------------------------------------------------------------------------------------------------------------

RATE, LOUT, S_, W_ = 25000.0, 128, 16, 32


def test_a_ctcss_tone_is_recovered():
    """a noise-free tone of amplitude 0.25 at each of the 50 frequencies and four phases: tone_amplitude gives 0.25 within 2 % (the model with numpy's
    table gave 1.35 % at worst; the margin covers the library's table against numpy's)"""
    f = G.ctcss_tones()
    assert f.shape == (50,) and f[0] == 67.0 and f[-1] == 254.1 and (np.diff(f) > 0).all()
    inc = G.tone_increments(f, RATE, S_)
    assert inc.dtype == np.uint32 and inc.shape == (50,)
    tab = lib_table()
    t = np.arange(W_ * LOUT, dtype=np.float64)
    worst = 0.0
    for j, fj in enumerate(f):
        for ph in (0.0, 0.25, 0.5, 0.8):
            d = (0.25 * np.cos(2 * np.pi * (fj * t / RATE + ph))).astype(np.float32)
            Z = M.tones(d, LOUT, inc[j:j + 1], S_, W_, tab)[0]
            a = float(G.tone_amplitude(Z[0, 0], W_ * LOUT, fj, RATE, S_))
            worst = max(worst, abs(a / 0.25 - 1))
    print("worst relative error of the recovered amplitude: %.4f" % worst)
    assert worst <= 0.02


def test_the_right_tone_in_noise():
    """amplitude 0.1 in Gaussian noise of sigma 0.3, tones 0, 12 and 49, four frames each: the strongest of the 50 is the right one in every frame and
    its power is at least 30 x the median tone's (the model alone gave 84 - 223)"""
    f = G.ctcss_tones()
    inc = G.tone_increments(f, RATE, S_)
    tab = lib_table()
    rng = np.random.default_rng(1)
    n = 4 * W_ * LOUT
    t = np.arange(n, dtype=np.float64)
    for j in (0, 12, 49):
        d = (0.1 * np.cos(2 * np.pi * f[j] * t / RATE + 1.0) + 0.3 * rng.standard_normal(n)).astype(np.float32)
        Z = M.tones(d, LOUT, inc, S_, W_, tab)[0]
        assert Z.shape == (4, 50)
        pw = np.abs(Z.astype(np.complex128)) ** 2
        ratio = pw[:, j] / np.median(pw, axis=1)
        print("tone %d: ratios %s" % (j, np.round(ratio, 1).tolist()))
        assert (np.argmax(pw, axis=1) == j).all()
        assert (ratio >= 30).all()
