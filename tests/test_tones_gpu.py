"""GPU tests (-m gpu) of the channel tones (fdc_pipeline_set_tones and its kin; include/fdc_amd.h): the tone bank behind the demodulation.

THE REFERENCE FOR BITS is tests/tones_model.py fed with the demodulated ports of a second handle with the tones off (whose bits do not depend on how the
stream is cut: demod's contract, tests/test_demod_gpu.py) and with the library's own table (fdc_tone_table): the frame rows must equal the model's
BYTE FOR BYTE, so no tolerance appears anywhere.  The model is held to its own properties on the CPU (tests/test_tones_cpu.py); a generated NaN is
compared as a NaN (its sign and payload are the platform's)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
import tones_model as M
from footprint import DeviceBanded, twice
from test_demod_gpu import CYCLES, KW
from test_fine_tuning_gpu import BANK, signal
from test_fine_tuning_routes_gpu import LONG, TINY, DeviceBuffers, by_channel
from test_iq_input_gpu import EXAMPLE, iq, same_bytes
from test_tones_cpu import same_but_nan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = [("path 5", 4096, EXAMPLE, 0), ("example plan, spectrum path", 4096, EXAMPLE, G.FDC_PIPE_NO_FUSED), ("bank", 16384, BANK, 0)]
plan_ids = [f[0] for f in PLANS]
NB = 9
SETTINGS = ((50, 16, 4), (1, 1, 1), (64, 64, 3), (7, 8, 12))          # (T, S, W)
MODES = {"fm": CYCLES, "mag": 0.75}


@functools.lru_cache(maxsize=None)
def table():
    t = G.tone_table()
    t.setflags(write=False)
    return t


def increments(Cn, T, S, seed=0):
    """[C][T] uint32: the CTCSS bank at 25 kHz where T = 50 (every channel the same), else seeded words, with 0 and 2^32 - 1 among them"""
    if T == 50:
        return np.ascontiguousarray(np.broadcast_to(G.tone_increments(G.ctcss_tones(), 25000.0, S), (Cn, 50)))
    inc = np.random.default_rng(1000 * T + S + seed).integers(0, 1 << 32, (Cn, T), dtype=np.uint64).astype(np.uint32)
    inc[0, 0] = 0
    inc[-1, -1] = 0xFFFFFFFF
    return inc


@functools.lru_cache(maxsize=None)
def ports(k, mode):
    """(x, the demodulated ports of NB blocks of plan k with the tones off): computed once and left unchanged"""
    _name, N, chans, flags = PLANS[k]
    x = signal(NB * (N - N // 2), 500 + k)
    p = G.Pipeline(N, 2, chans, max_blocks=NB, flags=flags)
    p.set_demod(mode, MODES[mode])
    d = p.work(x)
    x.setflags(write=False)
    for a in d:
        a.setflags(write=False)
    return x, d


@functools.lru_cache(maxsize=None)
def whole(k, mode, T, S, W):
    """the model's rows of the whole stream of plan k (the rows of its first nb blocks are the first (nb div W) of them: tests/test_tones_cpu.py)"""
    _x, d = ports(k, mode)
    louts = [a.size // NB for a in d]
    Z, fill, carry = M.call(d, louts, increments(len(d), T, S), S, W, table())
    Z.setflags(write=False)
    return Z


def toned(k, mode, T, S, W, nb=NB, **kw):
    _name, N, chans, flags = PLANS[k]
    p = G.Pipeline(N, 2, chans, max_blocks=nb, flags=flags, **kw)
    p.set_demod(mode, MODES[mode])
    p.set_tones(increments(len(chans), T, S), S, W)
    return p


# ---- the rows of a stream ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,S,W", SETTINGS, ids=["T%d S%d W%d" % s for s in SETTINGS])
@pytest.mark.parametrize("k,mode", [(0, "fm"), (1, "fm"), (2, "fm"), (0, "mag")], ids=["path 5 fm", "spectrum path fm", "bank fm", "path 5 mag"])
def test_frames_against_the_model(k, mode, T, S, W):
    """1, 2, 3, 5 and 9 blocks from a stream start: the rows are the model's over the ports of a handle with the tones off"""
    _name, N, chans, _flags = PLANS[k]
    H = N - N // 2
    x, d = ports(k, mode)
    Z = whole(k, mode, T, S, W)
    assert Z.shape == (NB // W, len(chans), T)
    p = toned(k, mode, T, S, W)
    st = p.tones_setting()
    same_bytes(st[0], increments(len(chans), T, S), "the setting's increments")
    assert st[1:] == (S, W)
    for nb in (1, 2, 3, 5, 9):
        p.reset()
        got_ports = p.work(x[:nb * H])
        for c, a in enumerate(got_ports):
            same_bytes(a, d[c][:a.size], "the ports with the tones on, ch%d" % c)         # (the audio off: the ports go home as ever)
        got = p.tones()
        assert got.dtype == np.complex64 and got.shape == (nb // W, len(chans), T)
        same_bytes(got, Z[:nb // W], "%d blocks" % nb)
    assert "tones: pass" in p.describe()
    if NB // W:
        assert np.abs(Z).max() > 0


CUTS = ((9,), (4, 5), (1, 1, 7), (3, 3, 3))


@pytest.mark.parametrize("T,S,W", [(50, 16, 4), (7, 8, 2), (3, 32, 5)], ids=["T50 S16 W4", "T7 S8 W2", "T3 S32 W5"])
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_cuts_of_the_stream_give_the_same_bits(k, T, S, W):
    """9 blocks as 9, 4 + 5, 1 + 1 + 7 and 3 + 3 + 3 (calls shorter than a frame complete none; cuts fall inside frames); host_sub_blocks and chunk_blocks;
    and behind a reset the stream starts anew"""
    _name, N, chans, _flags = PLANS[k]
    H = N - N // 2
    x, d = ports(k, "fm")
    Z = whole(k, "fm", T, S, W)
    empty = 0
    for cut in CUTS:
        p = toned(k, "fm", T, S, W)
        rows, b0 = [], 0
        for n in cut:
            p.work(x[b0 * H:(b0 + n) * H])
            rows.append(p.tones())
            assert rows[-1].shape[0] == (b0 + n) // W - b0 // W, (cut, b0, n)
            empty += rows[-1].shape[0] == 0
            b0 += n
        same_bytes(np.concatenate(rows), Z, "cut %r" % (cut,))
    assert empty > 0 or W == 2
    for kw in (dict(host_sub_blocks=2), dict(chunk_blocks=2), dict(chunk_blocks=2, host_sub_blocks=3)):
        p = toned(k, "fm", T, S, W, **kw)
        p.work(x[:4 * H])
        a = p.tones()
        p.work(x[4 * H:])
        same_bytes(np.concatenate([a, p.tones()]), Z, repr(kw))
        p.work(x)                                                                      # (blocks 9 .. 17 of the handle: its stream goes on, fill 9 mod W)
        p.reset()
        p.work(x)
        same_bytes(p.tones(), Z, "behind a reset, %r" % kw)


# ---- the pass alone, on hand-made samples -----------------------------------------------------------------------------------------------------------------

class Pass:
    """fdc_pipeline_tones_pass_device on a plan: hand-made d per channel in, (rows [nf][C][T], carry_out [C][T]) out"""

    def __init__(self, N=4096, R=2, chans=EXAMPLE, nb=9):
        self.p = G.Pipeline(N, R, chans, max_blocks=nb)
        self.p.set_demod("mag", 1.0)
        self.lout, self.Cn = self.p.lout, len(chans)

    def __call__(self, d, inc, S, W, first=0, fill=0, carry=None, shift=0):
        """shift: d_in is handed over `shift` floats behind a 256-byte boundary (1: no run is 16-byte aligned)"""
        p = self.p
        p.set_tones(inc, S, W)
        nb = d[0].size // self.lout[0]
        T = inc.shape[1]
        nf = (fill + nb) // W
        flat = np.zeros(shift + p.output_samples(nb), np.float32)
        for c, v in enumerate(d):
            flat[shift + p.channel_offset(c, nb):shift + p.channel_offset(c, nb) + nb * self.lout[c]] = v
        with DeviceBuffers() as dev:
            d_in = C.c_void_p(dev.put(flat).value + 4 * shift)
            d_fr = dev.put(np.full(max(1, nf * self.Cn * T), -7 - 7j, np.complex64))
            d_ci = dev.put(np.ascontiguousarray(carry, np.complex64)) if carry is not None else None
            d_co = dev.put(np.full(self.Cn * T, -9 - 9j, np.complex64))
            p.tones_pass_device(d_in, d_fr, nb, first, fill, d_ci, d_co)
            p.synchronize()
            return (dev.get(d_fr, max(1, nf * self.Cn * T), np.complex64)[:nf * self.Cn * T].reshape(nf, self.Cn, T),
                    dev.get(d_co, self.Cn * T, np.complex64).reshape(self.Cn, T))

    def model(self, d, inc, S, W, first=0, fill=0, carry=None):
        Z, _f, c = M.call(d, self.lout, inc, S, W, table(), first, fill, carry)
        return Z, c


def random_rows(lout, nb, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(nb * lo).astype(np.float32) for lo in lout]


def test_the_order_of_the_sums():
    """a group [1, 2^-24, 2^-24, 2^-24] sums to 1 ascending and to more descending; inc = 0 hands the sums through (cs = 1, sn = +0); and random
    mantissas under seeded increments, where a contracted product would show"""
    run = Pass()
    row = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], np.float32)
    inc0 = np.zeros((run.Cn, 1), np.uint32)
    for r, one in ((row, True), (row[::-1].copy(), False)):
        d = [np.resize(r, lo).astype(np.float32) for lo in run.lout]
        got, carry = run(d, inc0, 4, 1)
        want, wcarry = run.model(d, inc0, 4, 1)
        same_bytes(got, want, "the group sums, ascending %r" % one)
        same_bytes(carry, wcarry, "the carry")
        assert (got[0, 0, 0].real == np.float32(run.lout[0] // 4)) == one and (carry == 0).all()
    rng = np.random.default_rng(8)
    d = [(1 + rng.integers(0, 2 ** 23, 2 * lo) * 2.0 ** -23).astype(np.float32) * rng.choice([-1, 1], 2 * lo).astype(np.float32) for lo in run.lout]
    inc = increments(run.Cn, 64, 2, seed=3)
    got, carry = run(d, inc, 2, 2)
    want, wcarry = run.model(d, inc, 2, 2)
    same_bytes(got, want, "products rounded on their own")


def test_samples_that_are_not_finite():
    run = Pass()
    d = random_rows(run.lout, 4, 2)
    d[0][5], d[1][40], d[1][41], d[2][600], d[3][1000] = np.nan, np.inf, -np.inf, np.inf, -np.inf
    inc = increments(run.Cn, 7, 8)
    rng = np.random.default_rng(4)
    carry = (rng.standard_normal((run.Cn, 7)) + 1j * rng.standard_normal((run.Cn, 7))).astype(np.complex64)
    carry[2, 3] = np.nan
    got, co = run(d, inc, 8, 3, fill=1, carry=carry)
    want, wco = run.model(d, inc, 8, 3, fill=1, carry=carry)
    same_but_nan(got, want, "rows with NaN and Inf")
    same_but_nan(co, wco, "the carry")
    assert got.shape[0] == 1 and np.isnan(got[0, 0].real).all() and np.isnan(got[0, 1].real).all() and np.isnan(got[0, 2, 3].real)
    assert np.isinf(got[0, 2].real).any() and not np.isnan(co[0].view(np.float32)).any() and np.isinf(co[3].view(np.float32)).any()


@pytest.mark.parametrize("W", (1, 5))
def test_every_fill_with_a_carry(W):
    """every fill 0 .. W - 1 in front of 1, 4, 5 and 7 blocks, a carry in front (looked at only where fill > 0), at a first_block beyond the group wrap"""
    run = Pass()
    inc = increments(run.Cn, 7, 8)
    rng = np.random.default_rng(W)
    carry = (rng.standard_normal((run.Cn, 7)) + 1j * rng.standard_normal((run.Cn, 7))).astype(np.complex64)
    first = (1 << 32) // (run.lout[0] // 8) + (1 << 20) + 3            # b G beyond 2^32 for every channel
    for nb in (1, 4, 5, 7):
        d = random_rows(run.lout, nb, 10 * W + nb)
        for fill in range(W):
            got, co = run(d, inc, 8, W, first, fill, carry)
            want, wco = run.model(d, inc, 8, W, first, fill, carry)
            assert got.shape[0] == (fill + nb) // W
            same_bytes(got, want, "fill %d, %d blocks" % (fill, nb))
            same_bytes(co, wco, "the carry behind fill %d, %d blocks" % (fill, nb))
            if (fill + nb) % W == 0:
                assert (co.view(np.uint8) == 0).all()                       # no frame open: +0 bits
        got, co = run(d, inc, 8, W, first, 0, None)
        want, wco = run.model(d, inc, 8, W, first, 0, None)
        same_bytes(got, want, "no carry, %d blocks" % nb)
    # where the stream stands matters: the same samples at first_block 3 give other rows
    if W == 1:
        assert run(d, inc, 8, W, 3)[0].tobytes() != got.tobytes()


@pytest.mark.parametrize("S", (1, 2, 16, 128))
def test_row_counts_around_the_trips(S):
    """the wave takes 64 groups per trip: frames of 8 .. 4608 groups, among them 63 / 64 / 65-like seams (G = lout / S of 128, 256, 512, 256)"""
    run = Pass()
    inc = increments(run.Cn, 5, S)
    for nb, W, fill in ((1, 4, 0), (2, 2, 0), (3, 4, 1), (8, 4, 0), (9, 12, 0), (9, 4, 3)):
        d = random_rows(run.lout, nb, 100 * S + nb)
        rng = np.random.default_rng(nb)
        carry = (rng.standard_normal((run.Cn, 5)) + 1j * rng.standard_normal((run.Cn, 5))).astype(np.complex64)
        got, co = run(d, inc, S, W, 17, fill, carry)
        want, wco = run.model(d, inc, S, W, 17, fill, carry)
        same_bytes(got, want, "S %d, %d blocks, W %d, fill %d" % (S, nb, W, fill))
        same_bytes(co, wco, "the carry: S %d, %d blocks, W %d, fill %d" % (S, nb, W, fill))
        if nb in (3, 9):
            got, co = run(d, inc, S, W, 17, fill, carry, shift=1)             # no 16-byte loads: the same bits
            same_bytes(got, want, "4 bytes off: S %d, %d blocks, W %d, fill %d" % (S, nb, W, fill))
            same_bytes(co, wco, "4 bytes off, the carry: S %d, %d blocks, W %d, fill %d" % (S, nb, W, fill))


def test_long_rows_and_odd_widths():
    """rows of 24576 samples (l = 32768 at R = 4), and the R = 4 widths with an odd factor (lout = 3 l / 4: 12, 6, 192, 768, ...; runs that are not
    16-byte aligned take the 4-byte loads)"""
    run = Pass(65536, 4, LONG, nb=3)
    assert max(run.lout) == 24576
    for S, W in ((16, 2), (3, 1), (6144, 2), (1, 3)):
        inc = increments(run.Cn, 3, S)
        d = random_rows(run.lout, 3, S)
        got, co = run(d, inc, S, W, 5)
        want, wco = run.model(d, inc, S, W, 5)
        same_bytes(got, want, "long rows, S %d W %d" % (S, W))
        same_bytes(co, wco, "long rows, the carry, S %d W %d" % (S, W))
    tiny = [c for c in TINY if (c[1] - c[1] // 4) % 3 == 0 and c[1] >= 4]
    run = Pass(8192, 4, tiny, nb=5)
    assert all(lo % 3 == 0 for lo in run.lout) and len(run.lout) >= 3
    for S, W in ((3, 2), (1, 5), (6, 1)):
        inc = increments(run.Cn, 4, S)
        d = random_rows(run.lout, 5, S)
        got, co = run(d, inc, S, W, 2, 1 if W > 1 else 0, None)
        want, wco = run.model(d, inc, S, W, 2, 1 if W > 1 else 0, None)
        same_bytes(got, want, "odd widths, S %d W %d" % (S, W))
        same_bytes(co, wco, "odd widths, the carry, S %d W %d" % (S, W))


FOOT_PLANS = [("example, N = 4096", 4096, 2, EXAMPLE), ("bank, N = 16384", 16384, 2, BANK)]


@pytest.mark.parametrize("k", range(len(FOOT_PLANS)), ids=[f[0] for f in FOOT_PLANS])
def test_footprint_of_the_pass(k):
    """fdc_pipeline_tones_pass_device with the rows, carry_in and carry_out as three payloads between poisoned guards: exactly nf C T 8 and C T 8 bytes
    change, carry_in and every guard byte stay (both poison bytes), the input is untouched; and the handle's own stream goes on unharmed"""
    _name, N, R, chans = FOOT_PLANS[k]
    p = G.Pipeline(N, R, chans, max_blocks=5)
    p.set_demod("mag", 1.0)
    T, S, W = 7, 16, 3
    inc = increments(len(chans), T, S)
    p.set_tones(inc, S, W)
    lout, Cn = p.lout, len(chans)
    row = Cn * T * 8
    rng = np.random.default_rng(k)
    carry = (rng.standard_normal((Cn, T)) + 1j * rng.standard_normal((Cn, T))).astype(np.complex64)
    for nb, fill in ((5, 2), (1, 0), (4, 2)):
        nf = (fill + nb) // W
        d = random_rows(lout, nb, 7 * nb + k)
        want, _f, wco = M.call(d, lout, inc, S, W, table(), 3, fill, carry)
        flat = np.zeros(p.output_samples(nb), np.float32)
        for c, v in enumerate(d):
            flat[p.channel_offset(c, nb):p.channel_offset(c, nb) + nb * lout[c]] = v
        with DeviceBuffers() as dev:
            d_in = dev.put(flat)
            band = DeviceBanded(dev, [nf * row, row, row], row)
            for poison in twice(band):
                assert dev.hip.hipMemcpy(band.ptr(1), C.c_void_p(carry.ctypes.data), C.c_size_t(carry.nbytes), 1) == 0
                p.tones_pass_device(d_in, band.ptr(0), nb, 3, fill, band.ptr(1), band.ptr(2))
                p.synchronize()
                band.check([want, carry, wco], "%d blocks behind fill %d" % (nb, fill))
            same_bytes(dev.get(d_in, flat.size, np.float32), flat, "the input")
    assert p.tones_setting()[1:] == (S, W)
    lib = _lib.lib()
    assert lib.fdc_pipeline_tones_pass_device(p._h, 1, 1, None, None, 0, 0, 1, None) == -1            # no carry to write
    assert lib.fdc_pipeline_tones_pass_device(p._h, 1, 1, 2, 2, 0, 0, 1, None) == -1                  # one buffer for both
    assert lib.fdc_pipeline_tones_pass_device(p._h, None, 1, None, 2, 0, 0, 1, None) == -1
    assert lib.fdc_pipeline_tones_pass_device(p._h, 1, None, None, 2, 0, 0, W, None) == -1            # rows to write and nowhere to
    assert lib.fdc_pipeline_tones_pass_device(p._h, 1, 1, None, 2, 0, W, 1, None) == -1               # fill out of range
    assert lib.fdc_pipeline_tones_pass_device(p._h, 1, 1, None, 2, 0, -1, 1, None) == -1
    assert lib.fdc_pipeline_tones_pass_device(p._h, 1, 1, None, 2, -1, 0, 1, None) == -1
    assert lib.fdc_pipeline_tones_pass_device(p._h, None, None, None, None, 0, 0, 0, None) == 0
    p.set_tones(None)
    assert lib.fdc_pipeline_tones_pass_device(p._h, 1, 1, None, 2, 0, 0, 1, None) == -1               # the tones are off


# ---- the setting ------------------------------------------------------------------------------------------------------------------------------------------

def test_setting_semantics():
    N, R, nb = 4096, 2, 4
    H = N - N // R
    x = signal(3 * nb * H, 21)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    lib, u32 = _lib.lib(), C.POINTER(C.c_uint32)
    T, S, W = 5, 16, 3
    inc = increments(4, T, S)
    ptr = inc.ctypes.data_as(u32)
    assert p.tones_setting() is None and p.tones_device() is None
    # every refusal: the demodulation off; then, with it on, each argument
    with pytest.raises(G.FdcError, match="demodulation"):
        p.set_tones(inc, S, W)
    p.set_demod("fm", CYCLES)
    assert lib.fdc_pipeline_set_tones(p._h, ptr, 3, T, S, W) == -1 and lib.fdc_pipeline_set_tones(p._h, ptr, 4, 0, S, W) == -1
    assert lib.fdc_pipeline_set_tones(p._h, ptr, 4, 65, S, W) == -1 and lib.fdc_pipeline_set_tones(p._h, ptr, 4, T, 0, W) == -1
    assert lib.fdc_pipeline_set_tones(p._h, ptr, 4, T, S, 0) == -1 and lib.fdc_pipeline_set_tones(p._h, ptr, 4, T, S, 4097) == -1
    with pytest.raises(G.FdcError, match="channel 0"):
        p.set_tones(inc, 48, W)                                 # 48 does not divide 128
    assert p.tones_setting() is None
    q = G.Pipeline(8192, 2, [(100, 256, 0.8, 1.0), (5001, 64, 0.6, 0.9)], max_blocks=nb)
    q.set_demod("mag", 1.0)
    with pytest.raises(G.FdcError, match="channel 1"):
        q.set_tones(inc[:2], 64, W)                             # 64 divides 128 and not 32
    q.set_tones(inc[:2], 32, W)
    with pytest.raises(G.FdcError, match="tones"):
        q.set_demod(None)                                       # refused while the tones are on
    q.set_tones(None)
    q.set_demod(None)
    # the rows of the longest call beyond 2^31 bytes: 64 channels x 64 tones x 8 bytes x 70000 frames of one block
    many = [(16 * c + 8, 4, 1.0, 1.0) for c in range(64)]
    q = G.Pipeline(4096, 2, many, max_blocks=70000)
    q.set_demod("mag", 1.0)
    with pytest.raises(G.FdcError, match="2\\^31"):
        q.set_tones(increments(64, 64, 1), 1, 1)
    assert q.tones_setting() is None
    # a pipelined sinks batch inside the handle
    from test_demod_gpu import SINKS_KW
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, lookahead=True, max_blocks=nb, **SINKS_KW)
    p.work(x[:nb * H], sinks=bank)
    with pytest.raises(G.FdcError, match="pipelined"):
        p.set_tones(inc, S, W)
    while p.flush_sinks(bank) > 0:
        pass
    p.set_demod("fm")
    p.set_tones(inc, S, W)                                      # nothing inside any more
    assert p.tones_setting()[1:] == (S, W)


def test_what_resets_the_stream_and_what_keeps_it():
    N, R, nb = 4096, 2, 4
    H = N - N // R
    T, S, W = 5, 16, 3
    x = signal(3 * nb * H, 21)
    inc = increments(4, T, S)
    off = G.Pipeline(N, R, EXAMPLE, max_blocks=3 * nb)
    off.set_demod("fm", CYCLES)
    d = off.work(x)
    lout = off.lout

    def model(b0, b1, first=None):
        return M.call([a[b0 * lo:b1 * lo] for a, lo in zip(d, lout)], lout, inc, S, W, table(), b0 if first is None else first)[0]

    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    p.set_demod("fm", CYCLES)
    p.set_tones(inc, S, W)
    assert p.tones_device() is not None
    p.work(x[:nb * H])
    same_bytes(p.tones(), model(0, 4), "the first call")
    # a new demodulation gain keeps the open frame; the same setting again keeps it; a refused setting and a refused call keep it
    p.set_tones(inc, S, W)
    with pytest.raises(G.FdcError):
        p.set_tones(inc, 48, W)
    with pytest.raises(G.FdcError):
        p.set_demod(None)                                          # refused while the tones are on
    with pytest.raises((G.FdcError, ValueError)):
        p.work(x[:(nb + 1) * H])                                   # above max_blocks: refused
    st = p.tones_setting()
    same_bytes(st[0], inc, "the setting behind the refusals")
    p.work(x[nb * H:2 * nb * H])
    same_bytes(p.tones(), model(0, 8)[1:], "the second call continues (fill 1: rows 1 and 2 of the stream)")
    # another frame length: the stream starts anew at block 8 (frames counted from there, the phase from block 0)
    p.set_tones(inc, S, 2)
    p.work(x[2 * nb * H:])
    want = M.call([a[8 * lo:12 * lo] for a, lo in zip(d, lout)], lout, inc, S, 2, table(), 8)[0]
    same_bytes(p.tones(), want, "behind a new frame length")
    # other increments restart too; so does another demodulation mode; off and on again
    p.set_tones(inc, S, W)
    p.reset()
    p.work(x[:2 * H])
    assert p.tones().shape[0] == 0
    inc2 = inc.copy()
    inc2[1, 1] ^= 1
    p.set_tones(inc2, S, W)
    p.set_tones(inc, S, W)
    p.work(x[2 * H:5 * H])
    same_bytes(p.tones(), model(2, 5), "behind other increments: a new stream at block 2")
    p.reset()
    p.work(x[:2 * H])
    p.set_demod("mag", 1.0)
    p.set_demod("fm", CYCLES)
    p.work(x[2 * H:3 * H])
    assert p.tones().shape[0] == 0                                 # (a new stream of 1 block; the one of 2 continued would have completed a frame)
    p.reset()
    p.work(x[:2 * H])
    p.set_demod("fm", 2 * CYCLES)                                  # a new gain alone keeps the open frame: blocks 2 .. 4 complete stream frame 0
    p.set_demod("fm", CYCLES)
    p.work(x[2 * H:4 * H])
    same_bytes(p.tones(), model(0, 4), "a new gain keeps the state")
    p.set_tones(None)
    assert p.tones_setting() is None
    with pytest.raises(ValueError):
        p.tones()
    p.set_demod(None)


def test_the_getter_takes_the_capacity():
    N, R, nb = 4096, 2, 4
    H = N - N // R
    T, S, W = 5, 16, 2
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    p.set_demod("fm", CYCLES)
    p.set_tones(increments(4, T, S), S, W)
    lib = _lib.lib()
    nf = C.c_int32(-5)
    buf = np.full(2 * 4 * T + 3, -1 - 1j, np.complex64)
    assert lib.fdc_pipeline_tones(p._h, buf.ctypes.data, buf.nbytes, nb, C.byref(nf)) == -1            # no call yet
    p.work(signal(nb * H, 3))
    full = p.tones()
    assert full.shape == (2, 4, T)
    assert lib.fdc_pipeline_tones(p._h, buf.ctypes.data, full.nbytes - 1, nb, C.byref(nf)) == -1 and nf.value == -5
    assert (buf == -1 - 1j).all()
    assert lib.fdc_pipeline_tones(p._h, buf.ctypes.data, buf.nbytes, nb + 1, C.byref(nf)) == -1 and (buf == -1 - 1j).all()
    assert lib.fdc_pipeline_tones(p._h, buf.ctypes.data, full.nbytes, nb, C.byref(nf)) == 0 and nf.value == 2
    same_bytes(buf[:2 * 4 * T].reshape(2, 4, T), full, "exactly the capacity")
    assert (buf[2 * 4 * T:] == -1 - 1j).all()
    p.work(signal(H, 4))                                                                               # one block: no frame completed
    assert lib.fdc_pipeline_tones(p._h, None, 0, 1, C.byref(nf)) == 0 and nf.value == 0 and p.tones().shape == (0, 4, T)


def test_no_channels():
    """C = 0: on is accepted, and a call has nothing to correlate"""
    N, R, nb = 4096, 2, 3
    p = G.Pipeline(N, R, [], max_blocks=nb, keep_spectrum=True)
    p.set_demod("fm")
    p.set_tones(np.zeros((0, 3), np.uint32), 16, 2)
    outs, spec = p.work(signal(nb * (N - N // R), 1), want_spectrum=True)
    assert outs == [] and np.abs(spec).max() > 0 and "tones" not in p.describe()
    assert p.tones_setting()[1:] == (16, 2)
    p.set_tones(None)
    p.set_demod(None)


# ---- the entries ------------------------------------------------------------------------------------------------------------------------------------------

def test_host_entries_with_the_audio_on_and_off():
    """the audio on: the host entries hand home the audio and the rows and accept outs = NULL; the other input forms; the rows are those of the audio off"""
    k, T, S, W, D = 0, 50, 16, 4, 8
    _name, N, chans, _flags = PLANS[k]
    H = N - N // 2
    x, d = ports(k, "fm")
    Z = whole(k, "fm", T, S, W)
    taps = G.lowpass_taps(D, 64)
    ref = G.Pipeline(N, 2, chans, max_blocks=NB)
    ref.set_demod("fm", CYCLES)
    ref.set_audio(D, taps)
    audio = ref.work(x)
    for kw in (dict(), dict(host_sub_blocks=2)):
        p = toned(k, "fm", T, S, W, **kw)
        p.set_audio(D, taps)
        got = p.work(x)
        for c, a in enumerate(got):
            same_bytes(a, audio[c], "the audio beside the tones, ch%d, %r" % (c, kw))
        same_bytes(p.tones(), Z, "the rows beside the audio, %r" % kw)
        assert p.work_raw(x.ctypes.data, 5, None) == 5 and p.tones(5).shape[0] == (9 + 5) // W - 9 // W
    xr = np.ascontiguousarray(x.real)
    xi = iq(NB * H, np.int16, 33)
    for call in (lambda h: h.work_real(xr), lambda h: h.work_iq(xi, scale=2.0 ** -12)):
        q = G.Pipeline(N, 2, chans, max_blocks=NB)
        q.set_demod("mag", 0.75)
        dd = call(q)
        inc = increments(len(chans), T, S)
        q.set_tones(inc, S, W)
        q.reset()
        call(q)
        same_bytes(q.tones(), M.call(dd, q.lout, inc, S, W, table())[0], "another input form")


@pytest.mark.parametrize("k", (0, 2), ids=[plan_ids[0], plan_ids[2]])
def test_device_entries(k):
    """process_device over a ring: d_out is what it is with the tones off; 0..3 then 3..7 continue the stream; 4..7 behind it is a call elsewhere and
    starts a new stream, and the same call again does not continue itself"""
    _name, N, chans, flags = PLANS[k]
    T, S, W = 7, 8, 2
    H, ovl = N - N // 2, N // 2
    x, d = ports(k, "fm")
    ring = np.concatenate([np.zeros(ovl, np.complex64), x])
    inc = increments(len(chans), T, S)
    p = toned(k, "fm", T, S, W)
    lout = p.lout
    stream = M.Stream()
    with DeviceBuffers() as dev:
        for j, (first, n) in enumerate(((0, 3), (3, 4), (4, 3), (4, 3))):
            d_in = dev.put(np.ascontiguousarray(ring[first * H:first * H + ovl + n * H]))
            d_o = dev.put(np.zeros(p.output_samples(n), np.float32))
            p.process_device(d_in, first, n, d_o)
            p.synchronize()
            got_ports = by_channel(p, dev.get(d_o, p.output_samples(n), np.float32), n)
            if j < 2:
                for c, a in enumerate(got_ports):
                    same_bytes(a, d[c][first * lout[c]:(first + n) * lout[c]], "d_out of call %d, ch%d" % (j, c))
            want = stream.call(first, got_ports, lout, inc, S, W, table())
            got = p.tones(n)
            same_bytes(got, want, "the rows of call %d" % j)
            if want.size:
                same_bytes(dev.get(C.c_void_p(p.tones_device()), want.size, np.complex64).reshape(want.shape), want, "tones_device()")
        assert stream.next == 7 and stream.fill == 1


def test_beside_squelch_and_packed_audio():
    """tones, squelch and packed audio on one handle give the bytes each gives alone"""
    from test_squelch_gpu import stream as sq_stream
    k, T, S, W, D = 0, 50, 16, 4, 8
    _name, N, chans, flags = PLANS[k]
    x, _power, thr_o, thr_c = sq_stream(k)
    taps = G.lowpass_taps(D, 64)
    inc = increments(len(chans), T, S)

    def handle(tones, packed):
        p = G.Pipeline(N, 2, chans, max_blocks=NB, flags=flags, host_sub_blocks=4)
        p.set_demod("fm", CYCLES)
        if tones:
            p.set_tones(inc, S, W)
        if packed:
            p.set_levels(True)
            p.set_squelch(thr_o, thr_c, 1)
            p.set_audio(D, taps)
            p.set_audio_packing(True)
        return p

    a, b, both = handle(True, False), handle(False, True), handle(True, True)
    a.work(x)
    pb = b.work(x)
    pboth = both.work(x)
    same_bytes(both.tones(), a.tones(), "the rows")
    assert a.tones().shape[0] == NB // W
    same_bytes(both.squelch(), b.squelch(), "the mask")
    assert 0 < int(b.squelch().sum()) < b.squelch().size
    same_bytes(both.audio_packed(), b.audio_packed(), "the packed audio")
    for c, (u, v) in enumerate(zip(pboth, pb)):
        same_bytes(u, v, "the unpacked audio, ch%d" % c)
    assert "tones: pass" in both.describe() and "packed" in both.describe() and "tones" not in b.describe()


# ---- no allocation in the steady state ------------------------------------------------------------------------------------------------------------------

NO_ALLOC_CHILD = r'''
import ctypes as C, sys
import numpy as np
shim = C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL)
sys.path.insert(0, sys.argv[2])
import gr_fdc_amd as G

def counts():
    v = (C.c_long * 4)()
    shim.fdc_test_alloc_counts(v)
    return list(v)

hip = C.CDLL("libamdhip64.so")
N, R, nb = 4096, 2, 8
H = N - N // R
rng = np.random.default_rng(3)
x = (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H)).astype(np.complex64)
x2 = (rng.standard_normal(nb * 4096) + 1j * rng.standard_normal(nb * 4096)).astype(np.complex64)
EXAMPLE = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]
MIXED = [(100, 256, 0.8, 1.0), (5001, 64, 0.6, 0.9)]
inc = G.tone_increments(G.ctcss_tones(), 25000.0, 16)
inc2 = inc[::-1].copy()
p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pw = G.Pipeline(8192, 2, MIXED, max_blocks=nb, host_sub_blocks=3)
pd = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
for h, mode in ((p, "fm"), (pw, "mag"), (pd, "fm")):
    h.set_demod(mode, 0.5)
    h.set_tones(inc, 16, 3)
d_ring, d_out, d_fr, d_c0, d_c1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(4 * pd.output_samples(nb))) == 0
assert hip.hipMalloc(C.byref(d_fr), C.c_size_t(8 * 4 * 50 * 4)) == 0
assert hip.hipMalloc(C.byref(d_c0), C.c_size_t(8 * 4 * 50)) == 0 and hip.hipMalloc(C.byref(d_c1), C.c_size_t(8 * 4 * 50)) == 0
blk = [0]

def device():
    pd.process_device(d_ring, blk[0], nb, d_out)          # a stream that goes on: the carry is used and swapped, frames straddle the calls
    blk[0] += nb
    pd.synchronize()
    pd.tones(nb)

def the_pass():
    pd.tones_pass_device(d_out, d_fr, nb, 5, 2, d_c0, d_c1)
    pd.synchronize()

entries = {"fdc_pipeline_work (path 5, FM)": lambda: (p.work(x), p.tones()),
           "fdc_pipeline_work (spectrum path, sub-batches, MAG)": lambda: (pw.work(x2), pw.tones()),
           "fdc_pipeline_process_device and fdc_pipeline_tones": device,
           "fdc_pipeline_tones_pass_device": the_pass,
           "other increments of the same count before every call": lambda: (p.set_tones(inc2, 16, 3), p.work(x), p.set_tones(inc, 16, 3), p.work(x)),
           "another frame length before every call": lambda: (p.set_tones(inc, 16, 5), p.work(x), p.set_tones(inc, 16, 3), p.work(x)),
           "fdc_pipeline_set_tones off and on again": lambda: (pw.set_tones(None), pw.set_tones(inc, 16, 3), pw.work(x2))}
bad = []
for name, call in entries.items():
    for _ in range(3):
        call()
    before = counts()
    for _ in range(30):
        call()
    after = counts()
    print(name, [a - b for a, b in zip(after, before)])
    if after != before:
        bad.append((name, [a - b for a, b in zip(after, before)]))
assert "tones: pass" in p.describe() and "tones: pass" in pw.describe() and "tones: pass" in pd.describe(), (p.describe(), pw.describe())
assert not bad, bad
print("OK")
'''


def test_no_allocation_in_the_steady_state(tmp_path):
    shim = str(tmp_path / "libhipcount.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hip_alloc_counter.c"), "-o", shim,
                           "-ldl", "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([sys.executable, "-c", NO_ALLOC_CHILD, shim, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


# ---- the hier block ------------------------------------------------------------------------------------------------------------------------------------

def test_hier_block():
    N, R, nb = 4096, 2, 6
    H = N - N // R
    x = signal(2 * nb * H, 11)
    T, S, W = 50, 16, 4
    off = G.FrequencyDomainChannelizer(inptype=8, demod="fm", demod_gain=CYCLES, **KW)
    da, db = off.work(x[:nb * H]), off.work(x[nb * H:])
    lout = off.pipeline.lout
    inc1 = G.tone_increments(G.ctcss_tones(), 25000.0, S)
    on = G.FrequencyDomainChannelizer(inptype=8, demod="fm", demod_gain=CYCLES, tones=inc1, tone_group=S, tone_frame=W, **KW)
    st = on.pipeline.tones_setting()
    assert st[1:] == (S, W) and st[0].shape == (len(lout), T) and (st[0] == inc1[None, :]).all()
    model = M.Stream()
    for j, (xs, dd) in enumerate(((x[:nb * H], da), (x[nb * H:], db))):
        got_ports = on.work(xs)
        for c, a in enumerate(got_ports):
            same_bytes(a, dd[c], "hier block: the ports, call %d ch%d" % (j, c))
        want = model.call(j * nb, dd, lout, st[0], S, W, table())
        same_bytes(on.tones, want, "hier block: the rows of call %d" % j)
    assert want.shape[0] == (2 * nb) // W - nb // W
    on.work(x[:0])
    assert on.tones.shape == (0, len(lout), T)
    on.set_tones(inc1[:3], 8, 2)
    on.work(x[:nb * H])
    assert on.tones.shape == (nb // 2, len(lout), 3)
    on.set_tones(None)
    assert on.pipeline.tones_setting() is None
    with pytest.raises(ValueError):
        G.FrequencyDomainChannelizer(inptype=8, tones=inc1, **KW)             # tones without demod
