"""GPU tests (-m gpu) of the audio resampler (fdc_pipeline_set_audio_resampler and its kin; include/fdc_amd.h): the polyphase FIR with interpolation `up`
and decimation `down` behind the demodulation.

THE REFERENCE FOR BITS is the handle's own demodulated ports: the same stream with the audio off gives d_c, and tests/resample_model.py over those d
must equal the device's matrix BYTE FOR BYTE, pads included, in both formats.  No tolerance: the model is held to its bound on the CPU
(tests/test_resample_cpu.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
import audio_model as A
import resample_model as RS
import squelch_model as S
import test_squelch_gpu as SQ
import test_tone_squelch_gpu as TSQ
from footprint import DeviceBanded, twice
from test_audio_gpu import CUT_PLANS, FOOT_PLANS, FORMATS, cut_calls, example_ports
from test_demod_gpu import CYCLES, KW, MODES
from test_fine_tuning_gpu import BANK, signal
from test_fine_tuning_routes_gpu import LONG, TINY, DeviceBuffers, by_channel
from test_iq_input_gpu import EXAMPLE, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = ((8, 25, 64), (48, 25, 192), (3, 2, 13), (1, 8, 64), (64, 1, 128), (1, 1, 1), (5, 128, 15), (32, 125, 507), (2, 3, 512))
BOTH_MODES = ((8, 25, 64), (3, 2, 13))
F32 = np.float32


def taps_for(up, down, ntaps):
    """the designed low-pass where the count is the designer's, else seeded taps of both signs: a reordered sum shows in the bits"""
    if ntaps == 16 * up:
        return G.resampler_taps(up, down)
    return np.random.default_rng(1000 * up + 10 * down + ntaps).uniform(-1, 1, ntaps).astype(F32)


def widths(lout, up, down):
    return [RS.ceil_div(lo * up, down) for lo in lout]


def model(d, lout, cut, taps, up, down, fmt, scale, first=0, hist=None, masks=None):
    """the model's matrix of every call of the stream d (from block `first` on) cut into calls of `cut` blocks"""
    return RS.stream(hist or A.History(len(lout), RS.ceil_div(len(taps), up)), cut_calls(d, lout, cut, first), taps, up, down, lout, fmt, scale, masks)


def valid(mat, lout, up, down, first):
    return G.audio_resampled_channels(mat, lout, up, down, first)


def same_channels(got, want, what):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        same_bytes(np.ascontiguousarray(g), w, "%s, ch%d" % (what, c))


# ---- the ratios ----------------------------------------------------------------------------------------------------------------------------------------

RATIO_CASES = [r + m for r in RATIOS for m in (MODES if r in BOTH_MODES else MODES[:1])]


@pytest.mark.parametrize("up,down,ntaps,mode,gain", RATIO_CASES, ids=["%d/%d K%d %s" % (c[0], c[1], c[2], c[3]) for c in RATIO_CASES])
def test_ratio_sweep(up, down, ntaps, mode, gain):
    """the example plan (lout 128, 256, 512, 256; path 5) under every ratio, at 1, 2, 3 and 5 blocks from a stream start, both formats.  Kp = 256 at one
    block: channel 0 brings 128 < Kp - 1 samples, and a second call follows it"""
    N, R = 4096, 2
    H = N - N // R
    x, d = example_ports(mode, gain)
    taps = taps_for(up, down, ntaps)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=7)
    p.set_demod(mode, gain)
    lout = p.lout
    assert lout == [128, 256, 512, 256]
    for fmt, scale, dt in FORMATS:
        p.set_audio_resampler(up, down, taps, fmt, scale)
        st = p.audio_resampler_setting()
        assert st[:2] == (up, down) and st[3] == fmt and st[2].tobytes() == taps.tobytes() and p.audio_setting() is None
        assert _lib.lib().fdc_pipeline_audio_row(p._h) == sum(widths(lout, up, down))
        for nb in (1, 2, 3, 5):
            p.reset()
            got = p.work(x[:nb * H])
            want = model(d, lout, (nb,), taps, up, down, fmt, scale)[0]
            what = "%d/%d K %d %s %s, %d blocks" % (up, down, ntaps, mode, fmt, nb)
            same_bytes(p.audio(), want, what)
            assert p.audio_first_block() == 0 and [g.dtype for g in got] == [dt] * 4
            assert [g.size for g in got] == [RS.ceil_div(nb * lo * up, down) for lo in lout]
            same_channels(got, valid(want, lout, up, down, 0), what)
            if nb == 1:
                more = p.work(x[H:3 * H])
                want2 = model(d, lout, (1, 2), taps, up, down, fmt, scale)[1]
                same_bytes(p.audio(), want2, what + ", 1 + 2 blocks")
                assert p.audio_first_block() == 1
                same_channels(more, valid(want2, lout, up, down, 1), what + ", 1 + 2 blocks")
        assert "audio: resampled" in p.describe() and "gated" not in p.describe() and ("demod: %s" % mode) in p.describe()
    if up == 1:
        # up = 1 is the decimating form: a second handle under set_audio(down, ...) gives the same bytes
        q = G.Pipeline(N, R, EXAMPLE, max_blocks=7)
        q.set_demod(mode, gain)
        for fmt, scale, dt in FORMATS:
            q.set_audio(down, taps, fmt, scale)
            p.set_audio_resampler(up, down, taps, fmt, scale)
            for h in (p, q):
                h.reset()
                h.work(x[:3 * H])
                h.work(x[3 * H:5 * H])
            same_bytes(p.audio(), q.audio(), "up = 1 against set_audio(%d), %s" % (down, fmt))


CUT_RATIOS = ((8, 25, 64), (48, 25, 192), (3, 2, 13))


@pytest.mark.parametrize("fmt,scale,dt", FORMATS, ids=["f32", "s16"])
@pytest.mark.parametrize("k", range(len(CUT_PLANS)), ids=[f[0] for f in CUT_PLANS])
def test_cuts_of_the_stream_give_the_same_bits(k, fmt, scale, dt):
    """7 blocks as 7, 3 + 4, 1 + 1 + 5 and 2 + 2 + 3; host_sub_blocks (enqueue-path calls whose rows append, each with its own first block) and
    chunk_blocks (launch groups inside one enqueue call: one pass over the whole call); FM"""
    _name, N, chans, flags = CUT_PLANS[k]
    up, down, ntaps = CUT_RATIOS[k]
    R, nb = 2, 7
    H = N - N // R
    taps = taps_for(up, down, ntaps)
    x = signal(nb * H, 5 + k)
    ref = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    ref.set_demod("fm", CYCLES)
    d = ref.work(x)
    lout = ref.lout
    whole = model(d, lout, (7,), taps, up, down, fmt, scale)[0]
    for cut in ((7,), (3, 4), (1, 1, 5), (2, 2, 3)):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
        p.set_demod("fm", CYCLES)
        p.set_audio_resampler(up, down, taps, fmt, scale)
        want, b0 = model(d, lout, cut, taps, up, down, fmt, scale), 0
        assert np.concatenate(want).tobytes() == whole.tobytes()
        for j, n in enumerate(cut):
            outs = p.work(x[b0 * H:(b0 + n) * H])
            same_bytes(p.audio(), want[j], "cut %r, call %d" % (cut, j))
            assert p.audio_first_block() == b0
            same_channels(outs, valid(want[j], lout, up, down, b0), "cut %r, call %d: what work() returns" % (cut, j))
            b0 += n
    for kw in (dict(host_sub_blocks=2), dict(chunk_blocks=2), dict(chunk_blocks=2, host_sub_blocks=3)):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags, **kw)
        p.set_demod("fm", CYCLES)
        p.set_audio_resampler(up, down, taps, fmt, scale)
        outs = p.work(x)
        mat = p.audio()
        assert mat.shape == whole.shape and mat.dtype == dt
        same_bytes(mat, whole, repr(kw))
        same_channels(outs, valid(whole, lout, up, down, 0), repr(kw))


@pytest.mark.parametrize("first", (5, 2 ** 40 + 3), ids=["5", "2^40 + 3"])
def test_a_start_elsewhere_in_the_stream(first):
    """the device entry at first_block 5 and 2^40 + 3: phase and counts are the absolute index's although zeros stand in front; the call behind it
    continues the stream, a call elsewhere starts from zeros again and the same call again does not continue itself.  d_out is, byte for byte, what it is with the audio off"""
    N, R, nb = 4096, 2, 7
    H, ovl = N - N // R, N // R
    x = signal(nb * H, 340)
    ring = np.concatenate([np.zeros(ovl, np.complex64), x])
    up, down, ntaps = 8, 25, 64
    taps = taps_for(up, down, ntaps)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    p.set_demod("fm", CYCLES)
    lout, W = p.lout, widths(p.lout, up, down)
    lib = _lib.lib()
    with DeviceBuffers() as dev:
        def run(b0, at, n):
            d_in = dev.put(np.ascontiguousarray(ring[at * H:at * H + ovl + n * H]))
            d_o = dev.put(np.zeros(p.output_samples(n), np.float32))
            p.process_device(d_in, b0, n, d_o)
            p.synchronize()
            return by_channel(p, dev.get(d_o, p.output_samples(n), np.float32), n)

        off = [run(first, 0, 3), run(first + 3, 3, 4), run(first + 4, 4, 3)]
        for fmt, scale, dt in FORMATS:
            p.set_demod(None)
            p.set_demod("fm", CYCLES)
            p.set_audio_resampler(up, down, taps, fmt, scale)
            hist = A.History(len(lout), RS.ceil_div(ntaps, up))
            for j, (b0, at, n) in enumerate(((first, 0, 3), (first + 3, 3, 4), (first + 4, 4, 3), (first + 4, 4, 3))):
                ports = run(b0, at, n)
                same_channels(ports, off[min(j, 2)], "%s: d_out of call %d against the audio-off ports" % (fmt, j))
                want = RS.stream(hist, [(b0, n, ports)], taps, up, down, lout, fmt, scale)[0]
                mat = p.audio(n)
                same_bytes(mat, want, "%s: the matrix of call %d at block %d" % (fmt, j, b0))
                same_bytes(dev.get(C.c_void_p(p.audio_device()), n * sum(W), dt).reshape(n, sum(W)), mat, "audio_device()")
                assert p.audio_first_block() == b0
                # the row counts are the formula's at that index: the library's host function, the Python helper and the pads of the matrix agree
                for c, lo in enumerate(lout):
                    cnt = (C.c_int32 * n)()
                    assert lib.fdc_audio_resampler_counts(lo, up, down, b0, n, cnt) == 0
                    want_cnt = [RS.first_output(b0 + i + 1, lo, up, down) - RS.first_output(b0 + i, lo, up, down) for i in range(n)]
                    assert list(cnt) == want_cnt == G.audio_block_counts(lo, up, down, b0, n).tolist()
            p.set_audio_resampler(None)
        # the counts differ between the two starts somewhere, so a pass that took the call's own index 0 would fail above
        assert any(G.audio_block_counts(lo, up, down, first, 7).tolist() != G.audio_block_counts(lo, up, down, 0, 7).tolist() for lo in lout)


# ---- the edges -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", (4, 16))
def test_tiny_rows(R):
    """rows of 1, 2 and a few samples under (5, 128, 15) in single-block calls: most blocks own no output at all, some one; and under (3, 2, 13), where
    the history is rebuilt from fewer than Kp - 1 new samples several calls running"""
    N, nb = 8192, 6
    H = N - N // R
    x = signal(nb * H, 40 + R)
    ref = G.Pipeline(N, R, TINY, max_blocks=nb)
    assert min(ref.lout) == 1 and sorted(ref.lout)[1] == 2
    assert set(G.audio_block_counts(1, 5, 128, 0, 128).tolist()) == {0, 1}
    for mode, gain in MODES:
        ref.set_demod(mode, gain)
        ref.reset()
        d = ref.work(x)
        p = G.Pipeline(N, R, TINY, max_blocks=nb)
        p.set_demod(mode, gain)
        for up, down, ntaps in ((5, 128, 15), (3, 2, 13)):
            taps = taps_for(up, down, ntaps)
            for fmt, scale, _dt in FORMATS:
                p.set_audio_resampler(up, down, taps, fmt, scale)
                p.reset()
                want = model(d, p.lout, (1,) * nb, taps, up, down, fmt, scale)
                for j in range(nb):
                    outs = p.work(x[j * H:(j + 1) * H])
                    same_bytes(p.audio(), want[j], "R %d %s %s %d/%d, call %d" % (R, mode, fmt, up, down, j))
                    same_channels(outs, valid(want[j], p.lout, up, down, j), "R %d %s %s %d/%d, call %d" % (R, mode, fmt, up, down, j))


@pytest.mark.parametrize("up,down,ntaps", [(48, 25, 192), (2, 3, 512)], ids=["48/25 K192", "2/3 K512"])
def test_long_rows(up, down, ntaps):
    """lout = 6144, 12288 and 24576, three blocks: more outputs, and more samples, than one tile of the kernel holds"""
    N, R, nb = 32768, 4, 3
    H = N - N // R
    x = signal(nb * H, 9)
    taps = taps_for(up, down, ntaps)
    p = G.Pipeline(N, R, LONG, max_blocks=nb)
    assert p.lout == [6144, 12288, 24576]
    p.set_demod("fm", CYCLES)
    d = p.work(x)
    for fmt, scale, _dt in FORMATS:
        p.set_audio_resampler(up, down, taps, fmt, scale)
        p.reset()
        p.work(x)
        same_bytes(p.audio(), model(d, p.lout, (nb,), taps, up, down, fmt, scale)[0], "%d/%d %s" % (up, down, fmt))
        p.reset()
        want = model(d, p.lout, (1, 2), taps, up, down, fmt, scale)
        p.work(x[:H])
        same_bytes(p.audio(), want[0], "%d/%d %s, first of 1 + 2" % (up, down, fmt))
        p.work(x[H:])
        same_bytes(p.audio(), want[1], "%d/%d %s, second of 1 + 2" % (up, down, fmt))


def test_no_channels():
    """C = 0: on is accepted, and a call has nothing to filter"""
    N, R, nb = 4096, 2, 3
    H = N - N // R
    p = G.Pipeline(N, R, [], max_blocks=nb, keep_spectrum=True)
    p.set_demod("fm")
    p.set_audio_resampler(3, 2, [0.5, 0.5, 0.25])
    outs, spec = p.work(signal(nb * H, 1), want_spectrum=True)
    assert outs == [] and np.abs(spec).max() > 0 and p.audio_resampler_setting()[:2] == (3, 2) and "audio" not in p.describe()
    assert _lib.lib().fdc_pipeline_audio_row(p._h) == 0 and p.audio().shape == (nb, 0)
    p.set_audio_resampler(None)
    p.set_demod(None)


# ---- the gate ------------------------------------------------------------------------------------------------------------------------------------------

def gate(mat, mask, W):
    """the ungated matrix with every element of a closed (row, channel) cell replaced by zero bits"""
    out, at = mat.copy(), 0
    for c, w in enumerate(W):
        out[mask[:, c] == 0, at:at + w] = 0
        at += w
    return out


@pytest.mark.parametrize("hang", (0, 3))
@pytest.mark.parametrize("k", (0, 2), ids=[SQ.plan_ids[0], SQ.plan_ids[2]])
def test_gated(k, hang):
    """the same stream through a handle with the squelch and one without: open cells have the ungated handle's bits, closed cells and pads are zero, in
    both formats.  The stream is cut 6 + 3 and channels reopen in the second call: behind the opening the audio has the bits of the ungated pass, so the
    history ran on through the closed blocks"""
    _name, N, chans, flags = SQ.PLANS[k]
    H = N - N // 2
    x, power, thr_o, thr_c = SQ.stream(k)
    up, down, ntaps = (8, 25, 64) if k == 0 else (3, 2, 13)
    taps = taps_for(up, down, ntaps)
    whole, _s = S.squelch(power, None, thr_o, thr_c, hang)
    assert whole.min() == 0 and whole.max() == 1 and (np.diff(whole[5:].astype(int), axis=0) == 1).any()       # something reopens in the second call
    for fmt, scale, dt in FORMATS:
        un = G.Pipeline(N, 2, chans, max_blocks=SQ.NB, flags=flags)
        un.set_levels(True)
        on = SQ.squelched(N, chans, thr_o, thr_c, hang, flags=flags)
        for h in (un, on):
            h.set_demod("fm", CYCLES)
            h.set_audio_resampler(up, down, taps, fmt, scale)
        W = widths(on.lout, up, down)
        b0 = 0
        for n in (6, 3):
            un.work(x[b0 * H:(b0 + n) * H])
            outs = on.work(x[b0 * H:(b0 + n) * H])
            mask = on.squelch()
            same_bytes(mask, whole[b0:b0 + n], "the mask, call at %d" % b0)
            plain = un.audio()
            assert plain.dtype == dt and np.count_nonzero(plain) > plain.size // 2
            want = gate(plain, mask, W)
            same_bytes(on.audio(), want, "%s %d/%d hang %d, call at %d" % (fmt, up, down, hang, b0))
            same_channels(outs, valid(want, on.lout, up, down, b0), "what work() returns")
            b0 += n
        assert "audio: resampled, gated" in on.describe() and "squelch: pass" in on.describe() and "gated" not in un.describe()
    # the demodulated ports of a device entry are not gated
    ring = np.concatenate([np.zeros(N // 2, np.complex64), x])
    with DeviceBuffers() as dev:
        d_in = dev.put(ring)
        res = []
        for h in (un, on):
            d_o = dev.put(np.zeros(h.output_samples(SQ.NB), np.float32))
            h.process_device(d_in, 0, SQ.NB, d_o)
            h.synchronize()
            res.append(dev.get(d_o, h.output_samples(SQ.NB), np.float32))
        same_bytes(res[1], res[0], "d_out of a device entry")
        same_bytes(on.audio(SQ.NB), gate(un.audio(SQ.NB), whole, W), "the audio of a device entry")


def test_gated_under_the_tone_squelch():
    """the matrix is the ungated matrix of a second handle with the cells the model's COMBINED mask (carrier AND tone) closes replaced by zero bits"""
    k = 0
    T, S_, W_ = TSQ.SETTINGS[1]
    _name, N, chans, flags = TSQ.PLANS[k]
    H = N - N // 2
    x = TSQ.base(k, T, S_, W_)[0]
    _dec, mask = TSQ.whole(k, T, S_, W_, 1)
    up, down, ntaps = 8, 25, 64
    taps = taps_for(up, down, ntaps)
    for fmt, scale, dt in FORMATS:
        un = TSQ.plain(k, T, S_, W_, tones=False)
        gated = TSQ.toned(k, T, S_, W_, 1)
        for h in (un, gated):
            h.set_audio_resampler(up, down, taps, fmt, scale)
        W = widths(un.lout, up, down)
        b0 = 0
        for n in (4, 5):
            xs = x[b0 * H:(b0 + n) * H]
            un.work(xs)
            mat = un.audio()
            assert mat.dtype == dt and np.count_nonzero(mat) > mat.size // 2
            gated.work(xs)
            same_bytes(gated.squelch(), mask[b0:b0 + n], "the combined mask, call at %d" % b0)
            same_bytes(gated.audio(), gate(mat, mask[b0:b0 + n], W), "%s: the gated matrix, call at %d" % (fmt, b0))
            b0 += n
        assert "audio: resampled, gated" in gated.describe() and "tone squelch: pass" in gated.describe()


# ---- the pass alone, on hand-made samples -----------------------------------------------------------------------------------------------------------------

class Pass:
    """fdc_pipeline_audio_resampler_pass_device on the example plan: hand-made d per channel in, the matrix and the new history out"""

    def __init__(self, nb=1):
        self.p = G.Pipeline(4096, 2, EXAMPLE, max_blocks=nb)
        self.p.set_demod("mag", 1.0)
        self.nb, self.lout = nb, self.p.lout

    def __call__(self, d, up, down, taps, fmt="f32", scale=1.0, hist=None, first=0, mask=None):
        p, nb, K = self.p, self.nb, RS.ceil_div(len(taps), up)
        p.set_audio_resampler(up, down, taps, fmt, scale)
        dt = np.int16 if fmt == "s16" else np.float32
        flat = np.zeros(p.output_samples(nb), np.float32)
        for c, v in enumerate(d):
            flat[p.channel_offset(c, nb):p.channel_offset(c, nb) + nb * self.lout[c]] = v
        row = sum(widths(self.lout, up, down))
        with DeviceBuffers() as dev:
            d_in, d_out = dev.put(flat), dev.put(np.full(nb * row, 77, dt))
            d_hi = dev.put(np.concatenate(hist).astype(np.float32)) if hist is not None and K > 1 else None
            d_ho = dev.put(np.zeros(max(1, 4 * (K - 1)), np.float32)) if K > 1 else None
            d_m = dev.put(np.ascontiguousarray(mask, np.uint8)) if mask is not None else None
            p.audio_resampler_pass_device(d_in, d_out, first, nb, d_hi, d_ho, d_m)
            p.synchronize()
            mat = dev.get(d_out, nb * row, dt).reshape(nb, row)
            new = dev.get(d_ho, 4 * (K - 1), np.float32).reshape(4, K - 1) if K > 1 else np.zeros((4, 0), np.float32)
        return mat, new

    def want(self, d, up, down, taps, fmt="f32", scale=1.0, hist=None, first=0, mask=None):
        a = [RS.audio32(d[c], taps, up, down, lo, first, fmt, scale, None if hist is None else hist[c]) for c, lo in enumerate(self.lout)]
        return RS.matrix(a, self.lout, up, down, first, self.nb, mask)


def test_the_order_of_the_sum():
    """d = ones under taps [1, 2^-24, 2^-24] in every phase gives 1.0, under their reverse 1 + 2^-23: a contracted or reordered sum fails"""
    run = Pass()
    ones = [np.ones(lo, np.float32) for lo in run.lout]
    h3 = np.array([1.0, 2.0 ** -24, 2.0 ** -24], np.float32)
    for h, full in ((h3, np.float32(1.0)), (h3[::-1].copy(), np.float32(1.0) + np.float32(2.0 ** -23))):
        taps = np.repeat(h, 3)                              # up = 3: all three phases carry h
        mat, new = run(ones, 3, 2, taps)
        same_bytes(mat, run.want(ones, 3, 2, taps), "ones under %r" % h.tolist())
        got = valid(mat, run.lout, 3, 2, 0)
        assert all((g[6:] == full).all() and g[6:].size > 0 for g in got)
        assert (new == 1).all()
    # a product that a fused multiply-add would not round: h d with 24 + 24 significant bits, added to a value it nearly cancels
    rng = np.random.default_rng(8)
    d = [(1 + rng.integers(0, 2 ** 23, lo) * 2.0 ** -23).astype(np.float32) for lo in run.lout]
    taps = np.array([1 + 2.0 ** -23, -(1 + 3 * 2.0 ** -23), 1 + 5 * 2.0 ** -23, -(1 + 7 * 2.0 ** -23), 1 + 9 * 2.0 ** -23, -1.0], np.float32)
    mat, _new = run(d, 2, 3, taps, first=5)
    same_bytes(mat, run.want(d, 2, 3, taps, first=5), "products rounded on their own")


def test_samples_that_are_not_finite():
    """NaN and +-Inf reach exactly the outputs the model says, through the padded zero taps too, in both formats; the history in front counts; and a
    mask of the caller's gates the pass alone"""
    run = Pass()
    rng = np.random.default_rng(2)
    d = [rng.standard_normal(lo).astype(np.float32) for lo in run.lout]
    hist = [rng.standard_normal(4).astype(np.float32) for _ in run.lout]
    d[0][5], d[1][40], d[1][41], d[2][100], d[3][255] = np.nan, np.inf, -np.inf, np.inf, -np.inf
    hist[2][3], hist[3][0] = np.nan, np.inf
    taps = np.random.default_rng(3).uniform(-1, 1, 13).astype(np.float32)          # up = 3: Kp = 5, two phases end in a padded zero
    taps[4] = 0.0
    for fmt, scale in (("f32", 1.0), ("s16", 100.0)):
        mat, new = run(d, 3, 2, taps, fmt, scale, hist=hist, first=7)
        same_bytes(mat, run.want(d, 3, 2, taps, fmt, scale, hist, 7), fmt)
        for c in range(4):
            same_bytes(new[c], d[c][-4:], "the new history, ch%d" % c)
        if fmt == "f32":
            assert np.isnan(mat).any() and np.isinf(mat).any()
        mask = np.array([[1, 0, 1, 0]], np.uint8)
        mat, new = run(d, 3, 2, taps, fmt, scale, hist=hist, first=7, mask=mask)
        same_bytes(mat, run.want(d, 3, 2, taps, fmt, scale, hist, 7, mask), fmt + ", gated by the caller's mask")
        for c in range(4):
            same_bytes(new[c], d[c][-4:], "the new history of the gated pass, ch%d" % c)


def test_the_s16_edges():
    """ties to even, saturation, NaN -> 0, +-Inf -> the limits, the product with the scale rounded once (the edge list of tests/test_audio_cpu.py)"""
    run = Pass()
    a = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e9, -1e9, np.nan, np.inf, -np.inf, 32767.5, -32768.5, 32767.4, 4.5, 3.0, 5.0], np.float32)
    d = [np.resize(a, lo).astype(np.float32) for lo in run.lout]
    third = float(np.float32(1.0) / np.float32(3.0))
    for scale in (1.0, third, 0.5, -1.0):
        mat, _new = run(d, 1, 1, [1.0], "s16", scale)
        for c, g in enumerate(valid(mat, run.lout, 1, 1, 0)):
            same_bytes(g, A.s16(d[c], scale), "scale %r ch%d" % (scale, c))
    mat, _new = run(d, 1, 1, [1.0], "s16", 1.0)
    assert mat[0, :13].tolist() == [0, 2, 2, 0, -2, 32767, -32768, 0, 32767, -32768, 32767, -32768, 32767]


@pytest.mark.parametrize("k", range(len(FOOT_PLANS)), ids=[f[0] for f in FOOT_PLANS])
def test_footprint_of_the_pass(k):
    """fdc_pipeline_audio_resampler_pass_device with d_out, d_hist_in and d_hist_out as three payloads between poisoned guards: exactly nblocks A
    elements and C (Kp - 1) floats change, d_hist_in and every guard byte stay (both poison bytes), and the handle's own history and position stay.
    The input is the second of two calls of a stream, the history in front of it the model's"""
    _name, N, R, plan = FOOT_PLANS[k]
    chans = plan()
    H = N - N // R
    up, down, ntaps = (5, 128, 15) if k == 1 else (8, 25, 64) if k == 0 else (3, 2, 13)
    taps = taps_for(up, down, ntaps)
    K = RS.ceil_div(ntaps, up)
    for n1, n2 in ((5, 3), (1, 4)):
        x = signal((n1 + n2) * H, 60 + k)
        p = G.Pipeline(N, R, chans, max_blocks=max(n1, n2))
        p.set_demod("fm", CYCLES)
        d1, d2 = p.work(x[:n1 * H]), p.work(x[n1 * H:])
        lout, C_ = p.lout, len(p.lout)
        row = sum(widths(lout, up, down))
        n_out = p.output_samples(n2)
        flat = np.zeros(n_out, np.float32)
        for c, w in enumerate(d2):
            flat[p.channel_offset(c, n2):p.channel_offset(c, n2) + n2 * lout[c]] = w
        for fmt, scale, dt in FORMATS:
            hist = A.History(C_, K)
            want1, want2 = RS.stream(hist, [(0, n1, d1), (n1, n2, d2)], taps, up, down, lout, fmt, scale)
            h_in = A.History(C_, K)
            h_in.done(0, n1, d1)
            hist_in, hist_out = np.concatenate(h_in.hist).astype(np.float32), np.concatenate(hist.hist).astype(np.float32)
            p.set_audio_resampler(up, down, taps, fmt, scale)
            p.reset()
            p.work(x[:n1 * H])
            same_bytes(p.audio(), want1, "the handle's own first call")             # (the handle now stands behind the first call)
            isz = np.dtype(dt).itemsize
            with DeviceBuffers() as dev:
                d_in = dev.put(flat)
                band = DeviceBanded(dev, [n2 * row * isz, C_ * (K - 1) * 4, C_ * (K - 1) * 4], row * isz)
                for poison in twice(band):
                    untouched = np.full(C_ * (K - 1) * 4, poison, np.uint8)
                    assert dev.hip.hipMemcpy(band.ptr(1), C.c_void_p(hist_in.ctypes.data), C.c_size_t(hist_in.nbytes), 1) == 0
                    p.audio_resampler_pass_device(d_in, band.ptr(0), n1, n2, band.ptr(1), band.ptr(2))
                    p.synchronize()
                    band.check([want2, hist_in, hist_out], "%s behind a history, %d blocks" % (fmt, n2))
                    band.fill(poison)
                    p.audio_resampler_pass_device(d_in, band.ptr(0), n1, n2, None, band.ptr(2))
                    p.synchronize()
                    fresh = A.History(C_, K)
                    start = RS.stream(fresh, [(n1, n2, d2)], taps, up, down, lout, fmt, scale)[0]
                    band.check([start, untouched, np.concatenate(fresh.hist).astype(np.float32)], "%s at a stream start, %d blocks" % (fmt, n2))
                same_bytes(dev.get(d_in, n_out, np.float32), flat, "the input")
            p.work(x[n1 * H:])
            same_bytes(p.audio(), want2, "the handle's own second call, %s" % fmt)
    lib = _lib.lib()
    f = lib.fdc_pipeline_audio_resampler_pass_device
    assert f(p._h, 1, 1, None, None, 0, 1, None, None) == -1              # Kp > 1 without a history to write
    assert f(p._h, 1, 1, 2, 2, 0, 1, None, None) == -1                    # one buffer for both
    assert f(p._h, None, 1, None, 2, 0, 1, None, None) == -1 and f(p._h, 1, None, None, 2, 0, 1, None, None) == -1
    assert f(p._h, None, None, None, None, 0, 0, None, None) == 0 and f(p._h, 1, 1, None, 2, 0, -1, None, None) == -1 and f(p._h, 1, 1, None, 2, -1, 1, None, None) == -1
    assert lib.fdc_pipeline_audio_pass_device(p._h, 1, 1, None, 2, 1, None) == -1 and "resampler" in lib.fdc_last_error().decode()
    p.set_audio_resampler(None)
    assert f(p._h, 1, 1, None, 2, 0, 1, None, None) == -1                 # the resampler is off


# ---- the setting ---------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_and_getters():
    N, R, nb = 4096, 2, 2
    H = N - N // R
    x = signal(3 * nb * H, 6)
    xs = [x[j * nb * H:(j + 1) * nb * H] for j in range(3)]
    up, down = 8, 25
    taps, other = taps_for(up, down, 64), taps_for(up, down, 65)
    lib = _lib.lib()
    q = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    q.set_demod("fm", CYCLES)
    plain = [q.work(v) for v in xs]
    d_plain = q.describe()
    d1 = [np.concatenate([c[i] for c in plain]) for i in range(4)]
    lout = q.lout
    part = lambda j: [v[j * nb * lo:(j + 1) * nb * lo] for v, lo in zip(d1, lout)]

    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    # off by default; refused while the demodulation is off
    assert p.audio_resampler_setting() is None and lib.fdc_pipeline_audio_row(p._h) == 0 and p.audio_device() is None and p.audio_first_block() == -1
    with pytest.raises(G.FdcError) as e:
        p.set_audio_resampler(up, down, taps)
    assert e.value.status == -1 and "demodulation" in str(e.value) and p.audio_resampler_setting() is None
    p.set_demod("fm", CYCLES)
    p.set_audio_resampler(None)                                 # off while off: accepted
    # on in the middle of the stream: nothing stands in front of the first call, and the phase is the absolute index's
    p.work(xs[0])
    p.set_audio_resampler(up, down, taps)
    assert p.audio_device() is not None and p.audio_first_block() == -1
    p.work(xs[1])
    same_bytes(p.audio(), model(part(1), lout, (nb,), taps, up, down, "f32", 1.0, first=nb)[0], "switched on at block %d" % nb)
    assert p.audio_first_block() == nb and "audio: resampled" in p.describe()
    with pytest.raises(G.FdcError) as e:
        p.set_demod(None)
    assert e.value.status == -1 and "resampler" in str(e.value) and p.demod() == ("fm", CYCLES) and p.audio_resampler_setting()[:2] == (up, down)
    p.set_audio_resampler(None)
    assert p.audio_resampler_setting() is None and p.audio_first_block() == -1
    same_channels(p.work(xs[2]), plain[2], "off again")
    assert p.describe() == d_plain, (p.describe(), d_plain)
    # every range at the C entry: refused, the previous setting stays
    p.set_audio_resampler(up, down, taps, "s16", 300.0)
    before = p.audio_resampler_setting()
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    nan = np.array([1.0, np.nan], np.float32).ctypes.data_as(C.POINTER(C.c_float))
    big = np.ones(2 * 256 + 1, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    for args in ((65, 1, tp, 64, 0, 1.0), (-1, 1, tp, 64, 0, 1.0), (1, 0, tp, 64, 0, 1.0), (1, 129, tp, 64, 0, 1.0), (1, -3, tp, 64, 0, 1.0),
                 (up, down, tp, 0, 0, 1.0), (up, down, None, 64, 0, 1.0), (2, 1, big, 513, 0, 1.0), (up, down, nan, 2, 0, 1.0), (up, down, tp, 64, 2, 1.0),
                 (up, down, tp, 64, 1, 0.0), (up, down, tp, 64, 1, float("nan")), (16, 50, tp, 64, 0, 1.0), (64, 128, tp, 64, 0, 1.0)):
        assert lib.fdc_pipeline_set_audio_resampler(p._h, *args) == -1, args[0:2] + args[3:]
        now = p.audio_resampler_setting()
        assert now[:2] == before[:2] and now[2].tobytes() == before[2].tobytes() and now[3:] == before[3:]
    assert lib.fdc_pipeline_set_audio_resampler(p._h, 16, 50, tp, 64, 0, 1.0) == -1 and "8 / 25" in lib.fdc_last_error().decode()
    # the getter copies the taps only where the capacity holds them
    buf = np.full(80, 7, np.float32)
    k = C.c_int32(0)
    bp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.fdc_pipeline_audio_resampler_setting(p._h, None, None, C.byref(k), None, None, bp, 63) == 0 and k.value == 64 and (buf == 7).all()
    assert lib.fdc_pipeline_audio_resampler_setting(p._h, None, None, None, None, None, bp, -1) == 0 and (buf == 7).all()
    assert lib.fdc_pipeline_audio_resampler_setting(p._h, None, None, None, None, None, bp, 64) == 0
    assert buf[:64].tobytes() == taps.tobytes() and (buf[64:] == 7).all()
    # the decimating form's getter says off, and its pass alone is refused
    assert p.audio_setting() is None
    # the setting survives reset(), the history does not; a new format and scale keep the history; new taps or a new ratio restart the stream
    p.set_audio_resampler(up, down, taps)
    p.reset()
    want = model(d1, lout, (nb, nb, nb), taps, up, down, "f32", 1.0)
    p.work(xs[0])
    a0 = p.audio()
    same_bytes(a0, want[0], "first call")
    p.work(xs[1])
    same_bytes(p.audio(), want[1], "a continuing call")
    assert want[1].tobytes() != model(part(1), lout, (nb,), taps, up, down, "f32", 1.0, first=nb)[0].tobytes()
    p.reset()
    assert p.audio_resampler_setting()[:2] == (up, down) and "audio" not in p.describe()
    p.work(xs[0])
    same_bytes(p.audio(), a0, "after reset()")
    p.set_audio_resampler(up, down, taps, "s16", 9000.0)
    with pytest.raises(G.FdcError):
        p.audio(nb)                                             # a new format leaves no rows to fetch
    p.work(xs[1])
    same_bytes(p.audio(), model(d1, lout, (nb, nb), taps, up, down, "s16", 9000.0)[1], "a new format keeps the history")
    p.set_audio_resampler(up, down, taps, "s16", 100.0)
    assert p.audio(nb).shape[0] == nb                           # a new scale alone leaves the rows
    p.set_audio_resampler(up, down, other)
    p.work(xs[2])
    same_bytes(p.audio(), model(part(2), lout, (nb,), other, up, down, "f32", 1.0, first=2 * nb)[0], "new taps")
    p.reset()
    p.work(xs[0])
    p.set_audio_resampler(3, 2, other)
    with pytest.raises(G.FdcError):
        p.audio(nb)                                             # a new ratio leaves no rows to fetch
    p.work(xs[1])
    same_bytes(p.audio(), model(part(1), lout, (nb,), other, 3, 2, "f32", 1.0, first=nb)[0], "a new ratio")
    # a refused call leaves the stream continuing
    p.set_audio_resampler(up, down, taps)
    p.reset()
    p.work(xs[0])
    with pytest.raises(G.FdcError):
        p.work(x[:(nb + 1) * H])
    p.work(xs[1])
    same_bytes(p.audio(), want[1], "behind a refused call")


def test_the_two_forms_replace_each_other_and_the_packing_is_refused():
    N, R, nb, D = 4096, 2, 3, 8
    H = N - N // R
    x, d = example_ports("fm", CYCLES)
    up, down = 8, 25
    taps, low = taps_for(up, down, 64), G.lowpass_taps(D, 64)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    p.set_demod("fm", CYCLES)
    lout = p.lout
    p.set_audio(D, low)
    p.work(x[:nb * H])
    p.set_audio_resampler(up, down, taps)
    assert p.audio_setting() is None and p.audio_resampler_setting()[:2] == (up, down)
    with pytest.raises(G.FdcError):
        p.audio(nb)                                             # the rows of the other form are not served
    p.work(x[nb * H:2 * nb * H])
    same_bytes(p.audio(), model([v[nb * lo:] for v, lo in zip(d, lout)], lout, (nb,), taps, up, down, "f32", 1.0, first=nb)[0], "the resampler in the decimating form's place")
    p.set_audio(D, low)
    assert p.audio_resampler_setting() is None and p.audio_setting()[0] == D
    with pytest.raises(G.FdcError):
        p.audio(nb)
    p.reset()
    outs = p.work(x[:nb * H])
    want = A.audio_stream(A.History(4, 64), cut_calls(d, lout, (nb,)), low, D, "f32", 1.0)[0]
    same_channels(outs, want, "the decimating form in the resampler's place")
    assert "audio: pass" in p.describe() and "resampled" not in p.describe()
    # set_audio(None) switches off whichever is on
    p.set_audio_resampler(up, down, taps)
    p.set_audio(None)
    assert p.audio_resampler_setting() is None and p.audio_setting() is None and p.audio_device() is None
    p.set_demod(None)                                           # nothing holds the demodulation any more
    p.set_demod("fm", CYCLES)
    # a refused set_audio leaves the resampler on
    p.set_audio_resampler(up, down, taps)
    with pytest.raises(G.FdcError):
        p.set_audio(3, low)                                     # 3 does not divide 128
    assert p.audio_resampler_setting()[:2] == (up, down)
    # the packing: refused while the resampler is on, and the resampler while the packing is on
    p.set_levels(True)
    p.set_squelch(np.ones(4, np.float32), np.ones(4, np.float32), 0)
    with pytest.raises(G.FdcError) as e:
        p.set_audio_packing(True)
    assert e.value.status == -1 and "resampler" in str(e.value) and not p.audio_packing()
    p.set_audio(D, low)
    p.set_audio_packing(True)
    with pytest.raises(G.FdcError) as e:
        p.set_audio_resampler(up, down, taps)
    assert e.value.status == -1 and "packing" in str(e.value) and p.audio_resampler_setting() is None and p.audio_setting()[0] == D and p.audio_packing()
    p.set_audio_resampler(None)                                 # off while off stays accepted
    assert p.audio_setting()[0] == D and p.audio_packing()


def test_the_getter_takes_the_capacity():
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x, d = example_ports("fm", CYCLES)
    up, down = 48, 25
    taps = taps_for(up, down, 192)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    p.set_demod("fm", CYCLES)
    lib = _lib.lib()
    for fmt, scale, dt in FORMATS:
        p.set_audio_resampler(up, down, taps, fmt, scale)
        need = nb * sum(widths(p.lout, up, down)) * np.dtype(dt).itemsize
        buf = np.full(need + 64, 0xA5, np.uint8)
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need, nb) == -1 and (buf == 0xA5).all()      # no call since the format changed
        p.reset()
        p.work(x[:nb * H])
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need - 1, nb) == -1 and (buf == 0xA5).all()
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need + 64, nb - 1) == -1 and (buf == 0xA5).all()
        assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, need, nb) == 0
        assert (buf[need:] == 0xA5).all()
        same_bytes(buf[:need].view(dt).reshape(nb, -1), p.audio(), "the raw getter against audio(), %s" % fmt)


# ---- the feature off -----------------------------------------------------------------------------------------------------------------------------------

def test_the_feature_off_changes_nothing():
    """a handle on which the resampler was switched on and off again (or replaced by the decimating form) gives, on the audio, the gated and the packed
    route, the bytes and the describe string of a handle that never saw it"""
    k = 0
    _name, N, chans, flags = SQ.PLANS[k]
    H = N - N // 2
    x, power, thr_o, thr_c = SQ.stream(k)
    D = 8
    low, taps = G.lowpass_taps(D, 64), taps_for(8, 25, 64)

    def handle(touched, squelch, packed):
        p = G.Pipeline(N, 2, chans, max_blocks=SQ.NB, flags=flags)
        p.set_levels(True)
        p.set_demod("fm", CYCLES)
        if touched:
            p.set_audio_resampler(8, 25, taps, "s16", 50.0)
            p.work(x[:2 * H])
            p.reset()
            if touched == 1:
                p.set_audio_resampler(None)
        if squelch:
            p.set_squelch(thr_o, thr_c, 1)
        p.set_audio(D, low)
        if packed:
            p.set_audio_packing(True)
        return p

    for squelch, packed in ((False, False), (True, False), (True, True)):
        ref = handle(0, squelch, packed)
        a = [ref.work(x[:6 * H]), ref.work(x[6 * H:])]
        for touched in (1, 2):
            p = handle(touched, squelch, packed)
            b = [p.work(x[:6 * H]), p.work(x[6 * H:])]
            for u, v in zip(a, b):
                same_channels(v, u, "squelch %r packed %r touched %d" % (squelch, packed, touched))
            assert p.describe() == ref.describe(), (p.describe(), ref.describe())
            assert "resampled" not in p.describe()
            if not packed:
                same_bytes(p.audio(), ref.audio(), "the matrix")


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
taps, taps2 = G.resampler_taps(8, 25), G.resampler_taps(8, 25, cutoff=0.01)
p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pw = G.Pipeline(8192, 2, MIXED, max_blocks=nb, host_sub_blocks=3)
pd = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
for h, mode in ((p, "fm"), (pw, "mag"), (pd, "fm")):
    h.set_demod(mode, 0.5)
    h.set_audio_resampler(8, 25, taps)
pw.set_levels(True)
pw.set_squelch(np.zeros(2, np.float32), np.zeros(2, np.float32), 0)      # the gated form on one of them
d_ring, d_out, d_aud, d_h0, d_h1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(4 * pd.output_samples(nb))) == 0
assert hip.hipMalloc(C.byref(d_aud), C.c_size_t(4 * nb * G.lib().fdc_pipeline_audio_row(pd._h))) == 0
assert hip.hipMalloc(C.byref(d_h0), C.c_size_t(4 * 4 * 15)) == 0 and hip.hipMalloc(C.byref(d_h1), C.c_size_t(4 * 4 * 15)) == 0
blk = [0]

def device():
    pd.process_device(d_ring, blk[0], nb, d_out)          # a stream that goes on: the history is used and swapped
    blk[0] += nb
    pd.synchronize()
    pd.audio(nb)

def the_pass():
    pd.audio_resampler_pass_device(d_out, d_aud, blk[0], nb, d_h0, d_h1)
    pd.synchronize()

entries = {"fdc_pipeline_work (path 5, FM)": lambda: p.work(x),
           "fdc_pipeline_work (spectrum path, sub-batches, MAG, gated)": lambda: (pw.work(x2), pw.audio()),
           "fdc_pipeline_process_device and fdc_pipeline_audio": device,
           "fdc_pipeline_audio_resampler_pass_device": the_pass,
           "a new format and scale before every call": lambda: (p.set_audio_resampler(8, 25, taps, "s16", 100.0), p.work(x),
                                                                p.set_audio_resampler(8, 25, taps, "f32"), p.work(x)),
           "other taps of the same count before every call": lambda: (p.set_audio_resampler(8, 25, taps2), p.work(x), p.set_audio_resampler(8, 25, taps), p.work(x)),
           "the two forms in turn": lambda: (p.set_audio(8, G.lowpass_taps(8, 64)), p.work(x), p.set_audio_resampler(8, 25, taps), p.work(x)),
           "off and on again": lambda: (pd.set_audio_resampler(None), pd.set_audio_resampler(8, 25, taps), device())}
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
assert "audio: resampled" in p.describe() and "audio: resampled, gated" in pw.describe() and "audio: resampled" in pd.describe(), (p.describe(), pw.describe())
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
    up, down = 8, 25
    for mode, gain in MODES:
        off = G.FrequencyDomainChannelizer(inptype=8, demod=mode, demod_gain=gain, **KW)
        da, db = off.work(x[:nb * H]), off.work(x[nb * H:])
        lout = off.pipeline.lout
        d = [np.concatenate([u, v]) for u, v in zip(da, db)]
        for fmt, scale, dt in FORMATS:
            for taps in (None, taps_for(up, down, 40)):
                on = G.FrequencyDomainChannelizer(inptype=8, demod=mode, demod_gain=gain, audio_up=up, audio_down=down, audio_taps=taps, audio_format=fmt,
                                                  audio_scale=scale, **KW)
                h = G.resampler_taps(up, down) if taps is None else taps
                st = on.pipeline.audio_resampler_setting()
                assert st[:2] == (up, down) and st[3] == fmt and st[2].tobytes() == h.tobytes() and (fmt == "f32" or st[4] == scale)
                want = model(d, lout, (nb, nb), h, up, down, fmt, scale)
                same_channels(on.work(x[:nb * H]), valid(want[0], lout, up, down, 0), "hier block %s %s, first call" % (mode, fmt))
                same_channels(on.work(x[nb * H:]), valid(want[1], lout, up, down, nb), "hier block %s %s, second call" % (mode, fmt))
                assert [(o.shape, o.dtype) for o in on.work(x[:0])] == [((0,), dt)] * len(lout)
