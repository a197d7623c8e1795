"""GPU tests (-m gpu) of the channel audio (fdc_pipeline_set_audio and its kin; include/fdc_amd.h): the decimating FIR behind the demodulation.

THE REFERENCE FOR BITS is the handle's own demodulated ports: the same stream with the audio off gives d_c (whose bits do not depend on how the
stream is cut: demod's contract, tests/test_demod_gpu.py), and tests/audio_model.py over those d must equal the device's audio BYTE FOR BYTE, on every
sample, in both formats and both demodulation modes.  No tolerance: the model is held to its bound on the CPU (tests/test_audio_cpu.py)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
import audio_model as A
from footprint import DeviceBanded, twice
from test_demod_gpu import CYCLES, KW, MODES, PLANS
from test_fine_tuning_gpu import BANK, signal
from test_fine_tuning_routes_gpu import ALIAS_N, LONG, TINY, DeviceBuffers, alias_plan, by_channel
from test_iq_input_gpu import EXAMPLE, iq, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (("f32", 1.0, np.float32), ("s16", 9000.0, np.int16))     # (the s16 scale: FM ports in cycles fill the range and some samples saturate)
FILTERS = ((8, 64), (4, 33), (1, 256), (64, 1), (2, 2), (1, 1))
assert [f[0] for f in PLANS] == ["example, N = 4096", "bank of 64, N = 16384"]


def taps_for(D, K):
    """the low-pass of the decimation at (8, 64), else seeded taps of both signs: a reordered sum shows in the bits"""
    if (D, K) == (8, 64):
        return G.lowpass_taps(D, K)
    return np.random.default_rng(100 * D + K).uniform(-1, 1, K).astype(np.float32)


def cut_calls(d, lout, cut, first=0):
    """the calls (first_block, nblocks, [d_c of the call]) of a stream d (from block `first` on) cut into calls of `cut` blocks"""
    calls, b = [], 0
    for n in cut:
        calls.append((first + b, n, [d[c][b * lo:(b + n) * lo] for c, lo in enumerate(lout)]))
        b += n
    return calls


def model(d, lout, cut, taps, D, fmt, scale, hist=None, first=0):
    return A.audio_stream(hist or A.History(len(lout), len(taps)), cut_calls(d, lout, cut, first), taps, D, fmt, scale)


def same_audio(got, want, what):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        same_bytes(np.ascontiguousarray(g), w, "%s, ch%d" % (what, c))


@functools.lru_cache(maxsize=None)
def example_ports(mode, gain, nb=7):
    """the demodulated ports of the example plan's stream of nb blocks with the audio off, computed once and left unchanged"""
    N, R = 4096, 2
    x = signal(nb * (N - N // R), 77)
    x.setflags(write=False)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    p.set_demod(mode, gain)
    d = p.work(x)
    for a in d:
        a.setflags(write=False)
    return x, d


# ---- the filters ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,gain", MODES, ids=["fm", "mag"])
@pytest.mark.parametrize("D,K", FILTERS, ids=["D%d K%d" % f for f in FILTERS])
def test_filter_sweep(D, K, mode, gain):
    """the example plan (lout 128, 256, 512, 256; path 5) under every filter shape, at 1, 2, 3 and 5 blocks from a stream start, both formats.  K = 256 at
    one block: channel 0 brings 128 < K - 1 samples"""
    N, R = 4096, 2
    H = N - N // R
    x, d = example_ports(mode, gain)
    taps = taps_for(D, K)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=7)
    p.set_demod(mode, gain)
    assert p.lout == [128, 256, 512, 256]
    for fmt, scale, dt in FORMATS:
        p.set_audio(D, taps, fmt, scale)
        got_setting = p.audio_setting()
        assert got_setting[0] == D and got_setting[2] == fmt and got_setting[1].tobytes() == taps.tobytes()
        assert _lib.lib().fdc_pipeline_audio_row(p._h) == sum(p.lout) // D
        for nb in (1, 2, 3, 5):
            p.reset()
            got = p.work(x[:nb * H])
            assert [g.dtype for g in got] == [dt] * 4 and [g.size for g in got] == [nb * lo // D for lo in p.lout]
            same_audio(got, model(d, p.lout, (nb,), taps, D, fmt, scale)[0], "D %d K %d %s %s, %d blocks" % (D, K, mode, fmt, nb))
            # a second call of two blocks behind it: the history of a short call (K - 1 above what channel 0 brought) is the tail of front + d
            if nb == 1:
                more = p.work(x[H:3 * H])
                same_audio(more, model(d, p.lout, (1, 2), taps, D, fmt, scale)[1], "D %d K %d %s %s, 1 + 2 blocks" % (D, K, mode, fmt))
        assert "audio: pass" in p.describe() and ("demod: %s" % mode) in p.describe()
    if fmt == "s16" and mode == "fm" and K > 1:
        flat = np.concatenate(got)
        assert (np.abs(flat.astype(np.int32)) < 32767).any() and flat.any()


CUT_PLANS = [("path 5", 4096, EXAMPLE, 0), ("example plan, spectrum path", 4096, EXAMPLE, G.FDC_PIPE_NO_FUSED), ("bank", 16384, BANK, 0)]


@pytest.mark.parametrize("fmt,scale,dt", FORMATS, ids=["f32", "s16"])
@pytest.mark.parametrize("k", range(len(CUT_PLANS)), ids=[f[0] for f in CUT_PLANS])
def test_cuts_of_the_stream_give_the_same_bits(k, fmt, scale, dt):
    """7 blocks as 7, 3 + 4, 1 + 1 + 5 and 7 x 1; host_sub_blocks = 2 (four enqueue-path calls whose rows append) and chunk_blocks = 2 (launch groups
    inside one enqueue call: one pass over the whole call); FM, D = 8, K = 64"""
    _name, N, chans, flags = CUT_PLANS[k]
    R, nb, D = 2, 7, 8
    H = N - N // R
    taps = G.lowpass_taps(D, 64)
    x = signal(nb * H, 5 + k)
    ref = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    ref.set_demod("fm", CYCLES)
    d = ref.work(x)
    lout = ref.lout
    for cut in ((7,), (3, 4), (1, 1, 5), (1,) * 7):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
        p.set_demod("fm", CYCLES)
        p.set_audio(D, taps, fmt, scale)
        want, b0 = model(d, lout, cut, taps, D, fmt, scale), 0
        for j, n in enumerate(cut):
            same_audio(p.work(x[b0 * H:(b0 + n) * H]), want[j], "cut %r, call %d" % (cut, j))
            b0 += n
    whole = model(d, lout, (7,), taps, D, fmt, scale)[0]
    for kw in (dict(host_sub_blocks=2), dict(chunk_blocks=2), dict(chunk_blocks=2, host_sub_blocks=3)):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags, **kw)
        p.set_demod("fm", CYCLES)
        p.set_audio(D, taps, fmt, scale)
        same_audio(p.work(x), whole, repr(kw))
        # the matrix itself: row m is block m, channel c its own columns
        mat = p.audio()
        assert mat.shape == (nb, sum(lout) // D) and mat.dtype == dt
        at = 0
        for c, lo in enumerate(lout):
            same_bytes(np.ascontiguousarray(mat[:, at:at + lo // D]).reshape(-1), whole[c], "%r: the columns of ch%d" % (kw, c))
            at += lo // D


@pytest.mark.parametrize("R", (4, 16))
def test_tiny_rows(R):
    """rows of 1, 2 and a few samples under K = 5, D = 1 in single-block calls: the history is rebuilt from fewer than K - 1 new samples several calls
    running.  D = 2 is refused there: it does not divide lout = 1"""
    N, nb = 8192, 6
    H = N - N // R
    x = signal(nb * H, 40 + R)
    taps = taps_for(1, 5)
    ref = G.Pipeline(N, R, TINY, max_blocks=nb)
    assert min(ref.lout) == 1 and sorted(ref.lout)[1] == 2
    for mode, gain in MODES:
        ref.set_demod(mode, gain)
        ref.reset()
        d = ref.work(x)
        p = G.Pipeline(N, R, TINY, max_blocks=nb)
        p.set_demod(mode, gain)
        with pytest.raises(G.FdcError) as e:
            p.set_audio(2, taps)
        assert e.value.status == -1 and "channel 0" in str(e.value) and p.audio_setting() is None
        for fmt, scale, _dt in FORMATS:
            p.set_audio(1, taps, fmt, scale)
            p.reset()
            want = model(d, p.lout, (1,) * nb, taps, 1, fmt, scale)
            for j in range(nb):
                same_audio(p.work(x[j * H:(j + 1) * H]), want[j], "R %d %s %s, call %d" % (R, mode, fmt, j))


@pytest.mark.parametrize("D,K", [(64, 256), (1, 2)])
def test_long_rows(D, K):
    """lout = 6144, 12288 and 24576, three blocks: more outputs, and more samples, than one tile of the kernel holds"""
    N, R, nb = 32768, 4, 3
    H = N - N // R
    x = signal(nb * H, 9)
    taps = taps_for(D, K)
    p = G.Pipeline(N, R, LONG, max_blocks=nb)
    assert p.lout == [6144, 12288, 24576]
    p.set_demod("fm", CYCLES)
    d = p.work(x)
    for fmt, scale, _dt in FORMATS:
        p.set_audio(D, taps, fmt, scale)
        p.reset()
        same_audio(p.work(x), model(d, p.lout, (nb,), taps, D, fmt, scale)[0], "D %d K %d %s" % (D, K, fmt))
        p.reset()
        a, b = p.work(x[:H]), p.work(x[H:])
        want = model(d, p.lout, (1, 2), taps, D, fmt, scale)
        same_audio(a, want[0], "D %d K %d %s, first of 1 + 2" % (D, K, fmt))
        same_audio(b, want[1], "D %d K %d %s, second of 1 + 2" % (D, K, fmt))


# ---- the setting ---------------------------------------------------------------------------------------------------------------------------------------

def test_setting_semantics():
    N, R, nb, D = 4096, 2, 2, 4
    H = N - N // R
    x = signal(3 * nb * H, 6)
    xs = [x[j * nb * H:(j + 1) * nb * H] for j in range(3)]
    taps, other = taps_for(D, 33), taps_for(D, 34)
    g1, g2 = CYCLES, 0.25
    q = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    q.set_demod("fm", g1)
    plain = [q.work(v) for v in xs]
    d_plain = q.describe()
    d1 = [np.concatenate([c[i] for c in plain]) for i in range(4)]                 # the ports of the whole stream at gain g1
    q.set_demod("fm", g2)
    q.reset()
    d2 = [np.concatenate(v) for v in zip(*[q.work(v) for v in xs])]
    q.set_demod("mag", g1)
    q.reset()
    dm = [np.concatenate(v) for v in zip(*[q.work(v) for v in xs])]
    lout = q.lout
    part = lambda d, j: [v[j * nb * lo:(j + 1) * nb * lo] for v, lo in zip(d, lout)]
    lib = _lib.lib()

    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    # off by default; refused while the demodulation is off
    assert p.audio_setting() is None and lib.fdc_pipeline_audio_row(p._h) == 0 and p.audio_device() is None and "audio" not in p.describe()
    with pytest.raises(G.FdcError) as e:
        p.set_audio(D, taps)
    assert e.value.status == -1 and "demodulation" in str(e.value) and p.audio_setting() is None
    p.set_demod("fm", g1)
    same_audio(p.work(xs[0]), plain[0], "call 0, audio off")
    # on in the middle of the stream: nothing stands in front of the first call; off again restores bytes and describe string
    p.set_audio(D, taps)
    assert p.audio_device() is not None and lib.fdc_pipeline_audio_row(p._h) == sum(lout) // D
    same_audio(p.work(xs[1]), model(part(d1, 1), lout, (nb,), taps, D, "f32", 1.0, first=nb)[0], "call 1, switched on")
    assert "audio: pass" in p.describe()
    with pytest.raises(G.FdcError) as e:
        p.set_demod(None)
    assert e.value.status == -1 and "audio" in str(e.value) and p.demod() == ("fm", g1) and p.audio_setting()[0] == D
    p.set_audio(None)
    assert p.audio_setting() is None
    same_audio(p.work(xs[2]), plain[2], "call 2, off again")
    assert p.describe() == d_plain, (p.describe(), d_plain)
    # out-of-range arguments at the C entry: refused, the previous setting stays
    p.set_audio(D, taps, "s16", 300.0)
    before = p.audio_setting()
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    nan = np.array([1.0, np.nan], np.float32).ctypes.data_as(C.POINTER(C.c_float))
    for args in ((65, tp, 33, 0, 1.0), (-1, tp, 33, 0, 1.0), (D, tp, 0, 0, 1.0), (D, tp, 257, 0, 1.0), (D, None, 33, 0, 1.0), (D, nan, 2, 0, 1.0),
                 (D, tp, 33, 2, 1.0), (D, tp, 33, 1, 0.0), (D, tp, 33, 1, float("nan")), (3, tp, 33, 0, 1.0)):
        assert lib.fdc_pipeline_set_audio(p._h, *args) == -1, args[0:1] + args[2:]
        now = p.audio_setting()
        assert now[0] == before[0] and now[1].tobytes() == before[1].tobytes() and now[2:] == before[2:]
    # the setting survives reset(), the history does not
    p.set_audio(D, taps)
    p.reset()
    a0, a1 = p.work(xs[0]), p.work(xs[1])
    want = model(d1, lout, (nb, nb, nb), taps, D, "f32", 1.0)
    same_audio(a0, want[0], "first call")
    same_audio(a1, want[1], "a continuing call")
    assert any(a1[c].tobytes() != model(part(d1, 1), lout, (nb,), taps, D, "f32", 1.0, first=nb)[0][c].tobytes() for c in range(4))
    p.reset()
    assert p.audio_setting()[0] == D and "audio" not in p.describe()
    same_audio(p.work(xs[0]), a0, "after reset()")
    # a new format and scale keep the history
    p.set_audio(D, taps, "s16", 9000.0)
    same_audio(p.work(xs[1]), model(d1, lout, (nb, nb), taps, D, "s16", 9000.0)[1], "a new format keeps the history")
    # ... and so does a new demodulation gain: the history holds the samples as they were demodulated
    p.set_demod("fm", g2)
    mixed = [np.concatenate([u[:2 * nb * lo], v[2 * nb * lo:]]) for u, v, lo in zip(d1, d2, lout)]
    same_audio(p.work(xs[2]), model(mixed, lout, (nb, nb, nb), taps, D, "s16", 9000.0)[2], "a new demodulation gain keeps the history")
    # a refused call leaves the stream continuing: above max_blocks, and an entry that is refused while the demodulation is on
    p.set_demod("fm", g1)
    p.set_audio(D, taps)
    p.reset()
    p.work(xs[0])
    with pytest.raises(G.FdcError):
        p.work(x[:(nb + 1) * H])
    with pytest.raises(G.FdcError):
        p.work_spectrum(np.zeros(nb * N, np.complex64))
    same_audio(p.work(xs[1]), want[1], "behind two refused calls")
    # new taps, a new decimation or a new demodulation mode: the stream starts anew
    p.set_audio(D, other)
    same_audio(p.work(xs[2]), model(part(d1, 2), lout, (nb,), other, D, "f32", 1.0, first=2 * nb)[0], "new taps")
    p.reset()
    p.work(xs[0])
    p.set_audio(2 * D, other)
    same_audio(p.work(xs[1]), model(part(d1, 1), lout, (nb,), other, 2 * D, "f32", 1.0, first=nb)[0], "a new decimation")
    p.set_demod("mag", g1)
    same_audio(p.work(xs[2]), model(part(dm, 2), lout, (nb,), other, 2 * D, "f32", 1.0, first=2 * nb)[0], "a new demodulation mode")
    # MAG continues too: the audio keeps a position of its own
    p.reset()
    wm = model(dm, lout, (nb, nb), other, 2 * D, "f32", 1.0)
    same_audio(p.work(xs[0]), wm[0], "MAG, first call")
    same_audio(p.work(xs[1]), wm[1], "MAG, a continuing call")


def test_the_getter_takes_the_capacity():
    N, R, nb, D = 4096, 2, 3, 8
    H = N - N // R
    x, d = example_ports("fm", CYCLES)
    taps = G.lowpass_taps(D, 64)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    p.set_demod("fm", CYCLES)
    lib = _lib.lib()
    for fmt, scale, dt in FORMATS:
        p.set_audio(D, taps, fmt, scale)
        need = nb * (sum(p.lout) // D) * np.dtype(dt).itemsize
        buf = np.full(need + 64, 0xA5, np.uint8)
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need, nb) == -1 and (buf == 0xA5).all()      # no call since the format changed
        p.reset()
        got = p.work(x[:nb * H])
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need - 1, nb) == -1 and (buf == 0xA5).all()
        assert "bytes" in lib.fdc_last_error().decode()
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, 0, nb) == -1 and (buf == 0xA5).all()
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need + 64, nb - 1) == -1 and (buf == 0xA5).all()
        assert lib.fdc_pipeline_audio(p._h, None, need, nb) == -1
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need, nb) == 0
        assert (buf[need:] == 0xA5).all()
        same_bytes(buf[:need].view(dt).reshape(nb, -1), p.audio(), "the raw getter against audio(), %s" % fmt)
        same_audio(G.audio_channels(buf[:need].view(dt).reshape(nb, -1), p.lout, D), got, "the raw getter against work(), %s" % fmt)
    p.set_audio(None)
    assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need, nb) == -1
    with pytest.raises(ValueError):
        p.audio()


def test_no_channels():
    """C = 0: on is accepted, and a call has nothing to filter"""
    N, R, nb = 4096, 2, 3
    H = N - N // R
    p = G.Pipeline(N, R, [], max_blocks=nb, keep_spectrum=True)
    p.set_demod("fm")
    p.set_audio(2, [0.5, 0.5])
    outs, spec = p.work(signal(nb * H, 1), want_spectrum=True)
    assert outs == [] and np.abs(spec).max() > 0 and p.audio_setting()[0] == 2 and "audio" not in p.describe()
    assert _lib.lib().fdc_pipeline_audio_row(p._h) == 0 and p.audio().shape == (nb, 0)
    p.set_audio(None)
    p.set_demod(None)


# ---- the entries ---------------------------------------------------------------------------------------------------------------------------------------

def test_host_entries_write_nothing_to_outs():
    """while the audio is on the host entries leave outs alone (poisoned arrays stay poisoned) and accept outs = NULL; work_real and work_iq likewise"""
    N, R, nb, D = 4096, 2, 3, 8
    H = N - N // R
    x, d = example_ports("fm", CYCLES)
    taps = G.lowpass_taps(D, 64)
    want = model(d, [128, 256, 512, 256], (nb, 2), taps, D, "f32", 1.0)
    for kw in (dict(), dict(host_sub_blocks=2)):
        p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, **kw)
        p.set_demod("fm", CYCLES)
        p.set_audio(D, taps)
        outs = [np.full(nb * lo, np.float32(-7.5), np.float32) for lo in p.lout]        # (room for the demodulated ports, were they written)
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        assert p.work_raw(x.ctypes.data, nb, ptrs) == nb
        assert all((o == np.float32(-7.5)).all() for o in outs)
        same_audio(G.audio_channels(p.audio(nb), p.lout, D), want[0], "work_raw with poisoned outs, %r" % kw)
        assert p.work_raw(x[nb * H:].ctypes.data, 2, None) == 2
        same_audio(G.audio_channels(p.audio(2), p.lout, D), want[1], "work_raw with outs = NULL, %r" % kw)
        with pytest.raises(ValueError):
            p.work(x[:nb * H], outs=outs)
    # the other input forms: their own ports with the audio off are the reference
    xr = x.real.copy()
    xi = iq(nb * H, np.int16, 33)
    for call in (lambda h: h.work_real(xr[:nb * H]), lambda h: h.work_iq(xi, scale=2.0 ** -12)):
        p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
        p.set_demod("mag", 0.75)
        dd = call(p)
        p.set_audio(D, taps, "s16", 50.0)
        p.reset()
        same_audio(call(p), model(dd, p.lout, (nb,), taps, D, "s16", 50.0)[0], "another input form")


@pytest.mark.parametrize("k", range(len(PLANS)), ids=[f[0] for f in PLANS])
def test_device_entries(k):
    """process_device over a ring of 7 blocks: d_out is, byte for byte, what it is with the audio off; the audio goes to the handle's buffer.  0..3 then
    3..7 continue the stream; 4..7 behind it is a call elsewhere and starts from zeros, and the same call again does not continue itself"""
    _name, N, chans = PLANS[k]
    R, nb, D = 2, 7, 8
    H, ovl = N - N // R, N // R
    x = signal(nb * H, 340 + k)
    ring = np.concatenate([np.zeros(ovl, np.complex64), x])
    taps = G.lowpass_taps(D, 64)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    lout, row = p.lout, sum(p.lout) // D
    with DeviceBuffers() as dev:
        def run(first, n):
            d_in = dev.put(np.ascontiguousarray(ring[first * H:first * H + ovl + n * H]))
            d_o = dev.put(np.zeros(p.output_samples(n), np.float32))
            p.process_device(d_in, first, n, d_o)
            p.synchronize()
            return by_channel(p, dev.get(d_o, p.output_samples(n), np.float32), n)

        for mode, gain in MODES:
            for fmt, scale, dt in FORMATS:
                p.set_audio(None)
                p.set_demod(None)
                p.set_demod(mode, gain)
                off = [run(0, 3), run(3, 4), run(4, 3)]
                p.set_demod(None)
                p.set_demod(mode, gain)
                p.set_audio(D, taps, fmt, scale)
                hist = A.History(len(lout), 64)
                for j, (first, n) in enumerate(((0, 3), (3, 4), (4, 3), (4, 3))):
                    ports = run(first, n)
                    same_audio(ports, off[min(j, 2)], "%s %s: d_out of call %d against the audio-off ports" % (mode, fmt, j))
                    want = A.audio_stream(hist, [(first, n, ports)], taps, D, fmt, scale)[0]
                    mat = p.audio(n)
                    same_audio(G.audio_channels(mat, lout, D), want, "%s %s: the audio of call %d" % (mode, fmt, j))
                    same_bytes(dev.get(C.c_void_p(p.audio_device()), n * row, dt).reshape(n, row), mat, "audio_device()")
                    if j == 1:
                        assert hist.front(7)[0].any()                        # (the model continued: the history stood in front of call 1)
                assert hist.next == 7
        # above max_blocks: refused, nothing enqueued, and the stream goes on
        big = dev.put(np.zeros(ovl + 2 * nb * H, np.complex64))
        d_big = dev.put(np.full(p.output_samples(2 * nb), 7, np.float32))
        with pytest.raises(G.FdcError):
            p.process_device(big, 0, 2 * nb, d_big)
        p.synchronize()
        assert (dev.get(d_big, p.output_samples(2 * nb), np.float32) == 7).all()


# ---- the pass alone, on hand-made samples -----------------------------------------------------------------------------------------------------------------

class Pass:
    """fdc_pipeline_audio_pass_device on the example plan: hand-made d per channel in, the audio per channel and the new history out"""

    def __init__(self, nb=1):
        self.p = G.Pipeline(4096, 2, EXAMPLE, max_blocks=nb)
        self.p.set_demod("mag", 1.0)
        self.nb, self.lout = nb, self.p.lout

    def __call__(self, d, D, taps, fmt="f32", scale=1.0, hist=None):
        p, nb, K = self.p, self.nb, len(taps)
        p.set_audio(D, taps, fmt, scale)
        dt = np.int16 if fmt == "s16" else np.float32
        flat = np.zeros(p.output_samples(nb), np.float32)
        for c, v in enumerate(d):
            flat[p.channel_offset(c, nb):p.channel_offset(c, nb) + nb * self.lout[c]] = v
        row = sum(self.lout) // D
        with DeviceBuffers() as dev:
            d_in, d_out = dev.put(flat), dev.put(np.zeros(nb * row, dt))
            d_hi = dev.put(np.concatenate(hist).astype(np.float32)) if hist is not None and K > 1 else None
            d_ho = dev.put(np.zeros(max(1, 4 * (K - 1)), np.float32)) if K > 1 else None
            p.audio_pass_device(d_in, d_out, nb, d_hi, d_ho)
            p.synchronize()
            mat = dev.get(d_out, nb * row, dt).reshape(nb, row)
            new = dev.get(d_ho, 4 * (K - 1), np.float32).reshape(4, K - 1) if K > 1 else np.zeros((4, 0), np.float32)
        return G.audio_channels(mat, self.lout, D), new


def test_the_order_of_the_sum():
    """d = ones under taps [1, 2^-24, 2^-24] gives 1.0, under their reverse 1 + 2^-23 (tests/test_audio_cpu.py): a contracted or reordered sum fails"""
    run = Pass()
    ones = [np.ones(lo, np.float32) for lo in run.lout]
    h3 = np.array([1.0, 2.0 ** -24, 2.0 ** -24], np.float32)
    for taps, full in ((h3, np.float32(1.0)), (h3[::-1].copy(), np.float32(1.0) + np.float32(2.0 ** -23))):
        got, new = run(ones, 1, taps)
        for c, g in enumerate(got):
            same_bytes(g, A.fir_decim32(ones[c], taps, 1), "ch%d" % c)
            assert (g[2:] == full).all() and g[2:].size > 0
        assert (new == 1).all()
    # a product that a fused multiply-add would not round: h d with 24 + 24 significant bits, added to a value it nearly cancels
    rng = np.random.default_rng(8)
    d = [(1 + rng.integers(0, 2 ** 23, lo) * 2.0 ** -23).astype(np.float32) for lo in run.lout]
    taps = np.array([1 + 2.0 ** -23, -(1 + 3 * 2.0 ** -23), 1 + 5 * 2.0 ** -23], np.float32)
    got, _new = run(d, 2, taps)
    for c, g in enumerate(got):
        same_bytes(g, A.fir_decim32(d[c], taps, 2), "products rounded on their own, ch%d" % c)


def test_samples_that_are_not_finite():
    """NaN and +-Inf reach exactly the outputs the model says, in both formats; the history in front counts"""
    run = Pass()
    rng = np.random.default_rng(2)
    d = [rng.standard_normal(lo).astype(np.float32) for lo in run.lout]
    hist = [rng.standard_normal(4).astype(np.float32) for _ in run.lout]
    d[0][5], d[1][40], d[1][41], d[2][100], d[3][255] = np.nan, np.inf, -np.inf, np.inf, -np.inf
    hist[2][3], hist[3][0] = np.nan, np.inf
    taps = np.array([0.5, 0.0, -0.25, 1.0, 0.0], np.float32)
    for fmt, scale in (("f32", 1.0), ("s16", 100.0)):
        got, new = run(d, 2, taps, fmt, scale, hist=hist)
        for c, g in enumerate(got):
            want = A.audio32(d[c], taps, 2, fmt, scale, hist[c])
            same_bytes(g, want, "%s ch%d" % (fmt, c))
            same_bytes(new[c], d[c][-4:], "the new history, ch%d" % c)
        if fmt == "f32":
            assert np.isnan(got[0]).sum() >= 2 and np.isnan(got[1]).any() and np.isinf(got[2]).any() and np.isnan(got[2][:2]).any()


def test_the_s16_edges():
    """ties to even, saturation, NaN -> 0, +-Inf -> the limits, the product with the scale rounded once (the edge list of tests/test_audio_cpu.py)"""
    run = Pass()
    a = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e9, -1e9, np.nan, np.inf, -np.inf, 32767.5, -32768.5, 32767.4, 4.5, 3.0, 5.0], np.float32)
    d = [np.resize(a, lo).astype(np.float32) for lo in run.lout]
    third = float(np.float32(1.0) / np.float32(3.0))
    for scale in (1.0, third, 0.5, -1.0):
        got, _new = run(d, 1, [1.0], "s16", scale)
        for c, g in enumerate(got):
            same_bytes(g, A.s16(d[c], scale), "scale %r ch%d" % (scale, c))
    got, _new = run(d, 1, [1.0], "s16", 1.0)
    assert got[0][:13].tolist() == [0, 2, 2, 0, -2, 32767, -32768, 0, 32767, -32768, 32767, -32768, 32767]


FOOT_PLANS = [("example, N = 4096", 4096, 2, lambda: EXAMPLE), ("ragged runs, N = 8192", 8192, 4, lambda: TINY),
              ("aliased channels, N = 16384", ALIAS_N, 2, lambda: alias_plan(ALIAS_N))]


@pytest.mark.parametrize("k", range(len(FOOT_PLANS)), ids=[f[0] for f in FOOT_PLANS])
def test_footprint_of_the_pass(k):
    """fdc_pipeline_audio_pass_device with d_out, d_hist_in and d_hist_out as three payloads between poisoned guards: exactly nblocks A elements and
    C (K - 1) floats change, d_hist_in and every guard byte stay (both poison bytes), and the handle's own history and position stay: its stream goes
    on behind the first call, in bits.  The input is the second of two calls of a stream, the history in front of it the model's"""
    _name, N, R, plan = FOOT_PLANS[k]
    chans = plan()
    H = N - N // R
    D, K = (1, 5) if k == 1 else (8, 64)
    taps = taps_for(D, K)
    for n1, n2 in ((5, 3), (1, 4)):
        x = signal((n1 + n2) * H, 60 + k)
        p = G.Pipeline(N, R, chans, max_blocks=max(n1, n2))
        p.set_demod("fm", CYCLES)
        d1, d2 = p.work(x[:n1 * H]), p.work(x[n1 * H:])
        lout, C_ = p.lout, len(p.lout)
        row = sum(lout) // D
        n_out = p.output_samples(n2)
        flat = np.zeros(n_out, np.float32)
        for c, w in enumerate(d2):
            flat[p.channel_offset(c, n2):p.channel_offset(c, n2) + n2 * lout[c]] = w
        for fmt, scale, dt in FORMATS:
            hist = A.History(C_, K)
            want1, want2 = A.audio_stream(hist, [(0, n1, d1), (n1, n2, d2)], taps, D, fmt, scale)
            h_in = A.History(C_, K)
            h_in.done(0, n1, d1)
            hist_in, hist_out = np.concatenate(h_in.hist).astype(np.float32), np.concatenate(hist.hist).astype(np.float32)
            mat = np.empty((n2, row), dt)
            at = 0
            for c, lo in enumerate(lout):
                mat[:, at:at + lo // D] = want2[c].reshape(n2, lo // D)
                at += lo // D
            p.set_audio(D, taps, fmt, scale)
            p.reset()
            same_audio(p.work(x[:n1 * H]), want1, "the handle's own first call")     # (the handle now stands behind the first call)
            isz = np.dtype(dt).itemsize
            with DeviceBuffers() as dev:
                d_in = dev.put(flat)
                band = DeviceBanded(dev, [n2 * row * isz, C_ * (K - 1) * 4, C_ * (K - 1) * 4], row * isz)
                for poison in twice(band):
                    untouched = np.full(C_ * (K - 1) * 4, poison, np.uint8)
                    assert dev.hip.hipMemcpy(band.ptr(1), C.c_void_p(hist_in.ctypes.data), C.c_size_t(hist_in.nbytes), 1) == 0
                    p.audio_pass_device(d_in, band.ptr(0), n2, band.ptr(1), band.ptr(2))
                    p.synchronize()
                    band.check([mat, hist_in, hist_out], "%s behind a history, %d blocks" % (fmt, n2))
                    band.fill(poison)
                    p.audio_pass_device(d_in, band.ptr(0), n2, None, band.ptr(2))
                    p.synchronize()
                    fresh = A.History(C_, K)
                    start = A.audio_stream(fresh, [(n1, n2, d2)], taps, D, fmt, scale)[0]
                    got = dev.get(band.ptr(0), n2 * row, dt).reshape(n2, row)
                    same_audio(G.audio_channels(got, lout, D), start, "%s at a stream start" % fmt)
                    band.check([got, untouched, np.concatenate(fresh.hist).astype(np.float32)], "%s at a stream start, %d blocks" % (fmt, n2))
                same_bytes(dev.get(d_in, n_out, np.float32), flat, "the input")
            same_audio(p.work(x[n1 * H:]), want2, "the handle's own second call, %s" % fmt)
    lib = _lib.lib()
    assert lib.fdc_pipeline_audio_pass_device(p._h, 1, 1, None, None, 1, None) == -1          # K > 1 without a history to write
    assert lib.fdc_pipeline_audio_pass_device(p._h, 1, 1, 2, 2, 1, None) == -1                # one buffer for both
    assert lib.fdc_pipeline_audio_pass_device(p._h, None, 1, None, 2, 1, None) == -1 and lib.fdc_pipeline_audio_pass_device(p._h, 1, None, None, 2, 1, None) == -1
    assert lib.fdc_pipeline_audio_pass_device(p._h, None, None, None, None, 0, None) == 0 and lib.fdc_pipeline_audio_pass_device(p._h, 1, 1, None, 2, -1, None) == -1
    p.set_audio(None)
    assert lib.fdc_pipeline_audio_pass_device(p._h, 1, 1, None, 2, 1, None) == -1             # the audio is off


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
taps, taps2 = G.lowpass_taps(8, 64), G.lowpass_taps(8, 64, cutoff=0.05)
p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pw = G.Pipeline(8192, 2, MIXED, max_blocks=nb, host_sub_blocks=3)
pd = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
for h, mode in ((p, "fm"), (pw, "mag"), (pd, "fm")):
    h.set_demod(mode, 0.5)
    h.set_audio(8, taps)
d_ring, d_out, d_aud, d_h0, d_h1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(4 * pd.output_samples(nb))) == 0
assert hip.hipMalloc(C.byref(d_aud), C.c_size_t(4 * pd.output_samples(nb))) == 0
assert hip.hipMalloc(C.byref(d_h0), C.c_size_t(4 * 4 * 63)) == 0 and hip.hipMalloc(C.byref(d_h1), C.c_size_t(4 * 4 * 63)) == 0
blk = [0]

def device():
    pd.process_device(d_ring, blk[0], nb, d_out)          # a stream that goes on: the history is used and swapped
    blk[0] += nb
    pd.synchronize()
    pd.audio(nb)

def the_pass():
    pd.audio_pass_device(d_out, d_aud, nb, d_h0, d_h1)
    pd.synchronize()

entries = {"fdc_pipeline_work (path 5, FM)": lambda: p.work(x),
           "fdc_pipeline_work (spectrum path, sub-batches, MAG)": lambda: (pw.work(x2), pw.audio()),
           "fdc_pipeline_process_device and fdc_pipeline_audio": device,
           "fdc_pipeline_audio_pass_device": the_pass,
           "a new format and scale before every call": lambda: (p.set_audio(8, taps, "s16", 100.0), p.work(x), p.set_audio(8, taps, "f32"), p.work(x)),
           "other taps of the same count before every call": lambda: (p.set_audio(8, taps2), p.work(x), p.set_audio(8, taps), p.work(x)),
           "fdc_pipeline_set_audio off and on again": lambda: (pw.set_audio(None), pw.set_audio(8, taps), pw.work(x2))}
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
assert "audio: pass" in p.describe() and "audio: pass" in pw.describe() and "audio: pass" in pd.describe(), (p.describe(), pw.describe())
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
    N, R, nb, D = 4096, 2, 6, 4
    H = N - N // R
    x = signal(2 * nb * H, 11)
    taps = G.lowpass_taps(D, 33)
    for mode, gain in MODES:
        off = G.FrequencyDomainChannelizer(inptype=8, demod=mode, demod_gain=gain, **KW)
        da, db = off.work(x[:nb * H]), off.work(x[nb * H:])
        lout = off.pipeline.lout
        assert all(lo % D == 0 for lo in lout)
        d = [np.concatenate([u, v]) for u, v in zip(da, db)]
        for fmt, scale, dt in FORMATS:
            on = G.FrequencyDomainChannelizer(inptype=8, demod=mode, demod_gain=gain, audio_decim=D, audio_taps=taps, audio_format=fmt, audio_scale=scale, **KW)
            st = on.pipeline.audio_setting()
            assert st[0] == D and st[2] == fmt and st[1].tobytes() == taps.tobytes() and (fmt == "f32" or st[3] == scale)
            want = model(d, lout, (nb, nb), taps, D, fmt, scale)
            same_audio(on.work(x[:nb * H]), want[0], "hier block %s %s, first call" % (mode, fmt))
            same_audio(on.work(x[nb * H:]), want[1], "hier block %s %s, second call" % (mode, fmt))
            assert [(o.shape, o.dtype) for o in on.work(x[:0])] == [((0,), dt)] * 3
    # together with fine tuning, levels, gains and lag1: levels and lag1 are those of the block without the audio
    kw = dict(KW, fine_tuning=True, levels=True, lag1=True, gains=[2.0, 0.5, -1.0], demod="fm", demod_gain=CYCLES)
    both = G.FrequencyDomainChannelizer(inptype=8, audio_decim=D, audio_taps=taps, **kw)
    ref = G.FrequencyDomainChannelizer(inptype=8, **kw)
    a, dd = both.work(x[:nb * H]), ref.work(x[:nb * H])
    same_audio(a, model(dd, ref.pipeline.lout, (nb,), taps, D, "f32", 1.0)[0], "hier block with fine tuning, levels, gains and lag1")
    same_bytes(both.levels, ref.levels, "levels")
    same_bytes(both.lag1, ref.lag1, "lag1")
