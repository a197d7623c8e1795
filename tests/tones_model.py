"""THE DEFINITION of the channel tones (fdc_pipeline_set_tones; include/fdc_amd.h), in numpy.  The device is held to this BYTE FOR BYTE.

One channel at a time.  d: the real float32 stream k_chan_demod writes for the channel (the demodulation gain included), lout samples per block; S
the group length (it divides lout), G = lout / S; W the frame length in blocks; inc[T] uint32 phase increments; table[1024][2] float32 (cos, sin).
With b the stream's block index and q = 0 .. G - 1:

    u(b, q) = d[b lout + q S + i] summed over i = 0 .. S - 1, ascending, in float32 from +0, every sum rounded on its own
    g       = b G + q   (a 64-bit integer);   phase = (inc[t] g) mod 2^32;   k = phase >> 22;   (cs, sn) = table[k]
    re = re + float32(u cs);   im = im - float32(u sn)          per group, g ascending, every product and sum rounded on its own

The accumulator (re, im) of a tone runs on over the W blocks of a frame; at the frame's last group it is the frame's row and is reset to (+0, +0).
Frames are counted from the tone stream's start (fill = 0), the phase from the stream's block 0.  A call of nb blocks that finds `fill` blocks in the open
frame completes (fill + nb) div W frames and leaves (fill + nb) mod W blocks in the open one, with their accumulators as the carry.

tones() is vectorised over the tones; tones_loops() is the same rule as a plain triple loop (tests/test_tones_cpu.py holds one to the other)."""
import numpy as np

TABLE = 1024


def table():
    """The reference as numpy designs it: float32 of float64 (cos, sin)(2 pi k / 1024), the four axis entries exact.  The LIBRARY's table
    (fdc_tone_table) is the one the device uses; the tests compare the two and feed the model with the library's."""
    a = 2.0 * np.pi * np.arange(TABLE, dtype=np.float64) / TABLE
    t = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    t[0], t[256], t[512], t[768] = (1, 0), (0, 1), (-1, 0), (0, -1)
    return t


def group_sums(d, S):
    """u of every group of a run d (float32, a multiple of S long): ascending from +0, every sum rounded on its own"""
    d = np.asarray(d, dtype=np.float32).reshape(-1, int(S))
    with np.errstate(all="ignore"):
        # (ufunc.accumulate is sequential: r[i] = r[i - 1] + a[i], every sum rounded to float32; +0 stands in front)
        return np.add.accumulate(np.concatenate([np.zeros((d.shape[0], 1), np.float32), d], axis=1), axis=1, dtype=np.float32)[:, -1].copy()


def phases(inc, g0, n):
    """k[n][T] of the groups g0 .. g0 + n - 1 (g0 any non-negative Python integer): ((inc g) mod 2^32) >> 22, exact"""
    inc = np.asarray(inc, dtype=np.uint64).reshape(-1)
    g = (np.uint64(int(g0) & 0xFFFFFFFF) + np.arange(int(n), dtype=np.uint64)) & np.uint64(0xFFFFFFFF)      # (inc g) mod 2^32 needs g mod 2^32 only
    return (((g[:, None] * inc[None, :]) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)          # (< 2^64: exact in uint64)


def tones(d, lout, inc, S, W, tab, first_block=0, fill=0, carry=None):
    """One channel, one call: d the call's nb * lout samples, blocks first_block .. of the stream, `fill` blocks already in the open frame with the
    accumulators `carry` (complex64 [T]; None: zeros; looked at only where fill > 0).  Returns (Z complex64 [nf][T], new fill, new carry [T])."""
    d = np.asarray(d, dtype=np.float32).reshape(-1)
    lout, S, W = int(lout), int(S), int(W)
    assert lout % S == 0 and d.size % lout == 0 and 0 <= fill < W
    inc = np.asarray(inc, dtype=np.uint32).reshape(-1)
    tab = np.asarray(tab, dtype=np.float32)
    nb, G, T = d.size // lout, lout // S, inc.size
    u = group_sums(d, S)
    k = phases(inc, int(first_block) * G, nb * G)
    re, im = np.zeros(T, np.float32), np.zeros(T, np.float32)
    if fill > 0 and carry is not None:
        c = np.asarray(carry, dtype=np.complex64).reshape(T)
        re, im = c.real.astype(np.float32).copy(), c.imag.astype(np.float32).copy()
    rows, m = [], 0
    with np.errstate(all="ignore"):
        pc = (u[:, None] * tab[k, 0]).astype(np.float32)              # float32(u cs), [group][T]
        ps = (u[:, None] * tab[k, 1]).astype(np.float32)
        while m < nb:
            n = min(W - fill, nb - m)                                 # the blocks of the call inside the open frame
            # ufunc.accumulate is sequential: r[i] = r[i - 1] op a[i], every result rounded to float32; the accumulator stands in front
            re = np.add.accumulate(np.concatenate([re[None, :], pc[m * G:(m + n) * G]]), axis=0, dtype=np.float32)[-1]
            im = np.subtract.accumulate(np.concatenate([im[None, :], ps[m * G:(m + n) * G]]), axis=0, dtype=np.float32)[-1]
            m, fill = m + n, fill + n
            if fill == W:
                rows.append(np.zeros(T, np.complex64))
                rows[-1].real, rows[-1].imag = re, im                 # (bit for bit: no arithmetic on the way)
                re, im, fill = np.zeros(T, np.float32), np.zeros(T, np.float32), 0
    Z = np.array(rows, dtype=np.complex64).reshape(len(rows), T)
    carry_out = np.zeros(T, np.complex64)
    carry_out.real, carry_out.imag = re, im
    return Z, fill, carry_out


def tones_loops(d, lout, inc, S, W, tab, first_block=0, fill=0, carry=None):
    """tones() as a plain triple loop over blocks, groups and tones, one float32 scalar at a time"""
    d = np.asarray(d, dtype=np.float32).reshape(-1)
    inc = [int(v) for v in np.asarray(inc).reshape(-1)]
    nb, G, T = d.size // lout, lout // S, len(inc)
    acc = [[np.float32(0), np.float32(0)] for _ in range(T)]
    if fill > 0 and carry is not None:
        acc = [[np.float32(np.complex64(z).real), np.float32(np.complex64(z).imag)] for z in carry]
    rows = []
    with np.errstate(all="ignore"):
        for m in range(nb):
            for q in range(G):
                u = np.float32(0)
                for i in range(S):
                    u = np.float32(u + d[m * lout + q * S + i])
                g = (int(first_block) + m) * G + q
                for t in range(T):
                    k = ((inc[t] * g) % (1 << 32)) >> 22
                    acc[t][0] = np.float32(acc[t][0] + np.float32(u * tab[k][0]))
                    acc[t][1] = np.float32(acc[t][1] - np.float32(u * tab[k][1]))
            fill += 1
            if fill == W:
                row = np.zeros(T, np.complex64)
                row.real, row.imag = [a[0] for a in acc], [a[1] for a in acc]
                rows.append(row)
                acc, fill = [[np.float32(0), np.float32(0)] for _ in range(T)], 0
    carry_out = np.zeros(T, np.complex64)
    carry_out.real, carry_out.imag = [a[0] for a in acc], [a[1] for a in acc]
    return np.array(rows, dtype=np.complex64).reshape(len(rows), T), fill, carry_out


def call(ports, louts, inc, S, W, tab, first_block=0, fill=0, carry=None):
    """All channels of one call: ports[c] the call's demodulated samples of channel c, inc uint32 [C][T], carry complex64 [C][T] or None.
    Returns (Z complex64 [nf][C][T], new fill, new carry [C][T])."""
    inc = np.asarray(inc, dtype=np.uint32)
    Cn, T = inc.shape
    zs, cs, f = [], [], fill
    for c in range(Cn):
        z, f, co = tones(ports[c], louts[c], inc[c], S, W, tab, first_block, fill, None if carry is None else carry[c])
        zs.append(z)
        cs.append(co)
    nf = zs[0].shape[0] if Cn else 0
    Z = np.zeros((nf, Cn, T), np.complex64)
    for c in range(Cn):
        Z[:, c, :] = zs[c]
    return Z, f, np.array(cs, dtype=np.complex64).reshape(Cn, T)


class Stream:
    """The handle's stream state: a call continues where its first_block is the block after the last call's last, else the stream starts anew"""

    def __init__(self):
        self.next, self.fill, self.carry = -1, 0, None

    def call(self, first_block, ports, louts, inc, S, W, tab):
        if first_block != self.next:
            self.fill, self.carry = 0, None
        nb = len(ports[0]) // louts[0] if len(louts) else 0
        Z, self.fill, self.carry = call(ports, louts, inc, S, W, tab, first_block, self.fill, self.carry)
        self.next = first_block + nb
        return Z
