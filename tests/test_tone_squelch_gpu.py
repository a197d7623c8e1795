"""GPU tests (-m gpu) of the tone squelch (fdc_pipeline_set_tone_squelch and its kin; include/fdc_amd.h): the decision on the tones' frame rows and the
causal gate of the carrier mask, on the device.

THE REFERENCE FOR BITS is tests/tone_squelch_model.py fed with the frame rows and the carrier mask of a SECOND handle that has the tones and the
squelch on and the tone squelch off (both are independent of how the stream is cut: tests/test_tones_gpu.py, tests/test_squelch_gpu.py): dec and the
combined mask must equal the model's BYTE FOR BYTE, so no tolerance appears anywhere.

THE STREAM: per channel a carrier at the channel's centre, keyed in amplitude per block as tests/test_squelch_gpu.py keys it (every channel carries a
carrier), and phase-modulated by the channel's selected tone with an index that is keyed per block too: on in the stream's second half for even
channels, in its first half for odd ones.  The open threshold of a channel is the median of the model's own e over the stream's frames and the close
threshold half of it; every parametrisation asserts on the model alone that dec holds both 0 and 1 before anything of the device is compared."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
import audio_pack_model as APM
import squelch_model as SQ
import tone_squelch_model as M
from footprint import DeviceBanded, twice
from test_demod_gpu import CYCLES, KW, SINKS_KW
from test_fine_tuning_routes_gpu import DeviceBuffers
from test_iq_input_gpu import EXAMPLE, same_bytes
from test_squelch_gpu import AMP, SEQS, gate as gate_audio
from test_tones_gpu import NB, PLANS, increments, plan_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ((50, 16, 1), (7, 8, 2), (64, 64, 4))                     # (T, S, W)
setting_ids = ["T%d S%d W%d" % s for s in SETTINGS]
HANGS = (0, 1, 3)
BETA_ON = (0, 0, 0, 0, 1, 1, 1, 1, 1), (1, 1, 1, 1, 1, 0, 0, 0, 0)    # the modulation index per block: even channels, odd channels
GUARD = 1


def selected(k, T, S):
    """the tone every channel of plan k selects: the one of its row whose phase advance per group is nearest a quarter turn (far from the boxcar's nulls
    and from DC); the last channel of a plan of four is not tone-gated.  From the setting alone, nothing of the device"""
    inc = increments(len(PLANS[k][2]), T, S)
    x = inc.astype(np.float64) / 2.0 ** 32
    tone = np.argmin(np.abs(x - 0.25), axis=1).astype(np.int32)
    if len(tone) == 4:
        tone[3] = -1
    return tone


@functools.lru_cache(maxsize=None)
def stream(k, T, S):
    _name, N, chans, _flags = PLANS[k]
    H = N - N // 2
    inc = increments(len(chans), T, S)
    tone = selected(k, T, S)
    rng = np.random.default_rng(40 + k)
    t = np.arange(NB * H, dtype=np.float64)
    x = 1e-3 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    for c, (f, l, _p, _s) in enumerate(chans):
        amp = np.repeat(np.array([AMP[j] for j in np.resize(SEQS[c % 3], NB)]), H)
        beta = 0.5 * np.repeat(np.array(BETA_ON[c % 2], np.float64), H)
        # the tone's frequency in cycles per INPUT sample: inc / 2^32 per group of S output samples, l / N output samples per input sample
        fm = inc[c, max(int(tone[c]), 0)] / 2.0 ** 32 / S * l / N
        x += amp * np.exp(1j * (2 * np.pi * (((f + 0.501 * l) / N - 0.5) * t + rng.uniform()) + beta * np.sin(2 * np.pi * fm * t)))
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def plain(k, T, S, W, nb=NB, tones=True, audio=None, **kw):
    """a handle of plan k with everything the tone squelch needs, and the tone squelch off"""
    _name, N, chans, flags = PLANS[k]
    p = G.Pipeline(N, 2, chans, max_blocks=nb, flags=flags, **kw)
    p.set_levels(True)
    p.set_demod("fm", CYCLES)
    if tones:
        p.set_tones(increments(len(chans), T, S), S, W)
    if audio:
        p.set_audio(*audio)
    return p


@functools.lru_cache(maxsize=None)
def base(k, T, S, W):
    """(x, Z [NB div W][C][T] and carrier mask [NB][C] of a second handle with the tone squelch off, the carrier thresholds, tone, open, close, ratio):
    computed once and left unchanged"""
    x = stream(k, T, S)
    p = plain(k, T, S, W)
    p.work(x)
    power = p.levels()[:, :, 0].copy()
    top = power.max(axis=0)
    thr_o, thr_c = (top * np.float32(10.0 ** -0.5)).astype(np.float32), (top * np.float32(10.0 ** -1.5)).astype(np.float32)
    p.set_squelch(thr_o, thr_c, 1)
    p.reset()
    p.work(x)
    Z, cm = p.tones(), p.squelch()
    assert Z.shape[0] == NB // W and cm.shape == (NB, Z.shape[1])
    tone = selected(k, T, S)
    e = np.array([[M.energies(Z[f, c])[max(int(tone[c]), 0)] for c in range(Z.shape[1])] for f in range(Z.shape[0])], np.float32)
    open_thr = np.median(e.astype(np.float64), axis=0).astype(np.float32)
    close_thr = (open_thr * np.float32(0.5)).astype(np.float32)
    ratio = np.where(np.arange(Z.shape[1]) % 2 == 1, 0.25, 0.0).astype(np.float32)
    for a in (Z, cm, thr_o, thr_c, tone, open_thr, close_thr, ratio):
        a.setflags(write=False)
    return x, Z, cm, thr_o, thr_c, tone, open_thr, close_thr, ratio


@functools.lru_cache(maxsize=None)
def whole(k, T, S, W, hang):
    """the model's (dec, combined mask) of the whole stream, asserted to decide both ways and to gate something the carrier leaves open"""
    x, Z, cm, thr_o, thr_c, tone, o, c, r = base(k, T, S, W)
    dec, mask, fill, _st = M.call(Z, cm, tone, o, c, r, GUARD, hang, W)
    gated = tone >= 0
    assert set(dec[:, gated].ravel().tolist()) == {0, 1}, ("the model's dec must hold both values", k, T, S, W, hang, dec.T.tolist())
    assert (dec[:, ~gated] == 1).all() and (mask[:, ~gated] == cm[:, ~gated]).all()
    assert (mask <= cm).all() and (mask != cm).any() and mask[:, gated].any(), (k, T, S, W, hang)
    assert (mask[:W, gated] == 0).all()                             # the first frame of a fresh stream is closed
    dec.setflags(write=False)
    mask.setflags(write=False)
    return dec, mask


def toned(k, T, S, W, hang, nb=NB, audio=None, packed=False, **kw):
    x, Z, cm, thr_o, thr_c, tone, o, c, r = base(k, T, S, W)
    p = plain(k, T, S, W, nb=nb, audio=audio, **kw)
    p.set_squelch(thr_o, thr_c, 1)
    if packed:
        p.set_audio_packing(True)
    p.set_tone_squelch(tone, o, c, r, GUARD, hang)
    return p


# ---- the decisions and the mask of a stream ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hang", HANGS)
@pytest.mark.parametrize("T,S,W", SETTINGS, ids=setting_ids)
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_stream_against_the_model(k, T, S, W, hang):
    """1, 2, 3, 5 and 9 blocks from a stream start: dec and the combined mask are the model's over a second handle's rows and carrier mask"""
    _name, N, chans, _flags = PLANS[k]
    H = N - N // 2
    x, Z, cm, thr_o, thr_c, tone, o, c, r = base(k, T, S, W)
    dec, mask = whole(k, T, S, W, hang)
    p = toned(k, T, S, W, hang)
    st = p.tone_squelch_setting()
    same_bytes(st[0], np.asarray(tone), "the setting's tones")
    assert st[1].tobytes() == o.tobytes() and st[2].tobytes() == c.tobytes() and st[3].tobytes() == r.tobytes() and st[4:] == (GUARD, hang)
    for nb in (1, 2, 3, 5, 9):
        p.reset()
        p.work(x[:nb * H])
        same_bytes(p.tones(), Z[:nb // W], "the rows beside the tone squelch, %d blocks" % nb)
        got = p.tone_squelch()
        assert got.dtype == np.uint8 and got.shape == (nb // W, len(chans))
        same_bytes(got, dec[:nb // W], "dec, hang %d, %d blocks" % (hang, nb))
        same_bytes(p.squelch(), mask[:nb], "the combined mask, hang %d, %d blocks" % (hang, nb))
    d = p.describe()
    assert "tone squelch: pass" in d and "tones: pass" in d and "squelch: pass" in d


@pytest.mark.parametrize("T,S,W", SETTINGS, ids=setting_ids)
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_cuts_of_the_stream_give_the_same_bits(k, T, S, W):
    """9 blocks as 9, 4 + 5, 1 + 1 + 7 and 3 + 3 + 3 (calls that complete no frame; cuts inside frames); host_sub_blocks and chunk_blocks; and behind a
    reset the stream starts anew"""
    _name, N, chans, _flags = PLANS[k]
    H = N - N // 2
    hang = 1
    x = base(k, T, S, W)[0]
    dec, mask = whole(k, T, S, W, hang)
    for cut in ((9,), (4, 5), (1, 1, 7), (3, 3, 3)):
        p = toned(k, T, S, W, hang)
        decs, masks, b0 = [], [], 0
        for n in cut:
            p.work(x[b0 * H:(b0 + n) * H])
            decs.append(p.tone_squelch())
            masks.append(p.squelch())
            assert decs[-1].shape[0] == (b0 + n) // W - b0 // W, (cut, b0, n)
            b0 += n
        same_bytes(np.concatenate(decs), dec, "dec, cut %r" % (cut,))
        same_bytes(np.concatenate(masks), mask, "the mask, cut %r" % (cut,))
    for kw in (dict(host_sub_blocks=2), dict(chunk_blocks=2), dict(chunk_blocks=2, host_sub_blocks=3)):
        p = toned(k, T, S, W, hang, **kw)
        p.work(x[:4 * H])
        a, ma = p.tone_squelch(), p.squelch()
        p.work(x[4 * H:])
        same_bytes(np.concatenate([a, p.tone_squelch()]), dec, "dec, %r" % kw)
        same_bytes(np.concatenate([ma, p.squelch()]), mask, "the mask, %r" % kw)
        p.work(x)                                                       # (the stream goes on: a carried state and a fill of 9 mod W)
        p.reset()
        p.work(x)
        same_bytes(p.tone_squelch(), dec, "dec behind a reset, %r" % kw)
        same_bytes(p.squelch(), mask, "the mask behind a reset, %r" % kw)


# ---- the pass alone, on hand-made rows and masks ----------------------------------------------------------------------------------------------------------

def narrow_plan(Cn):
    """Cn channels of 4 bins at N = 4096 (lout = 2)"""
    return [(16 * c + 8, 4, 1.0, 1.0) for c in range(Cn)]


class Pass:
    """fdc_pipeline_tone_squelch_pass_device on a plan of Cn narrow channels with T tones and frames of W blocks"""

    def __init__(self, Cn, T, W):
        self.p = G.Pipeline(4096, 2, narrow_plan(Cn), max_blocks=4)
        self.p.set_levels(True)
        self.p.set_squelch(1.0, 1.0, 0)
        self.p.set_demod("mag", 1.0)
        self.p.set_tones(np.arange(1, Cn * T + 1, dtype=np.uint32).reshape(Cn, T), 1, W)
        self.Cn, self.T, self.W = Cn, T, W

    def setting(self, tone, o, c, r, guard, hang):
        self.set = (np.asarray(tone, np.int32), np.asarray(o, np.float32), np.asarray(c, np.float32), np.asarray(r, np.float32), guard, hang)
        self.p.set_tone_squelch(*self.set)

    def __call__(self, dev, Z, nb, fill=0, state=None, cm=None):
        """(dec [nf][C], state [C][2], mask [nb][C] or None) of the device"""
        Cn, T = self.Cn, self.T
        nf = (fill + nb) // self.W
        assert Z.shape == (nf, Cn, T)
        d_fr = dev.put(np.ascontiguousarray(Z, np.complex64)) if nf else None
        d_dec = dev.put(np.full(max(1, nf * Cn), 0xEE, np.uint8)) if nf else None
        d_in = dev.put(np.ascontiguousarray(state, np.int32)) if state is not None else None
        d_out = dev.put(np.full(2 * Cn, -77, np.int32))
        d_mask = dev.put(np.ascontiguousarray(cm, np.uint8)) if cm is not None else None
        self.p.tone_squelch_pass_device(d_fr, d_dec, nb, fill, d_in, d_out, d_mask)
        self.p.synchronize()
        return (dev.get(d_dec, nf * Cn, np.uint8).reshape(nf, Cn) if nf else np.zeros((0, Cn), np.uint8), dev.get(d_out, 2 * Cn, np.int32).reshape(Cn, 2),
                dev.get(d_mask, nb * Cn, np.uint8).reshape(nb, Cn) if cm is not None else None)

    def model(self, Z, nb, fill=0, state=None, cm=None):
        tone, o, c, r, guard, hang = self.set
        dec, st = M.decide(Z, tone, o, c, r, guard, hang, state)
        return dec, st, (M.gate(cm, dec, tone, self.W, fill, state) if cm is not None else None)


OPEN4, CLOSE4 = np.array([16, 36, 64, 100], np.float32), np.array([4, 9, 16, 100], np.float32)       # squares: a row can hit them exactly


def seam_rows(nf, T, tone, hang, seed):
    """Z [nf][4][T]: seeded classes of the selected tone, mostly low; in front of every seam of the trips (64, 128, 192) a strong frame and low frames
    across it, so that a closing run straddles the seam; the other tones small"""
    rng = np.random.default_rng(seed)
    cls = rng.choice(3, size=(nf, 4), p=(0.8, 0.1, 0.1))
    for b in (64, 128, 192):
        for c in range(4):
            s = b - 1 - (hang * (c + 1)) // 4 - c % 2
            if s >= 0 and b + hang + 2 <= nf:
                cls[s, c] = 2
                cls[s + 1:b + hang + 2, c] = 0
    mag = np.where(cls == 2, np.sqrt(1.5 * OPEN4)[None, :], np.where(cls == 1, np.sqrt(0.5 * (OPEN4 + CLOSE4))[None, :], np.sqrt(0.5 * CLOSE4)[None, :]))
    Z = (0.1 * (rng.standard_normal((nf, 4, T)) + 1j * rng.standard_normal((nf, 4, T)))).astype(np.complex64)
    for c in range(4):
        if tone[c] >= 0:
            ph = np.exp(2j * np.pi * rng.uniform(size=nf))
            Z[:, c, tone[c]] = (mag[:, c] * ph).astype(np.complex64)
    return Z


@pytest.mark.parametrize("hang", HANGS)
@pytest.mark.parametrize("T", (1, 7, 64))
def test_frame_counts_around_the_trips(T, hang):
    """1 .. 200 completed frames (a trip takes 64), closing runs across the seams, every carried state (0, 0), (1, 0 .. hang) and states that must be
    read (clipped), and the call continued from the state it wrote: dec and the state are the model's"""
    run = Pass(4, T, 1)
    tone = [0, T - 1, T // 2, -1]
    run.setting(tone, OPEN4, CLOSE4, [0.0, 0.5, 0.0, 0.0], 0, hang)
    states = [None] + [np.array([(1, h), (1, hang - h), (0, 0), (1, h)], np.int32) for h in range(hang + 1)] + [np.array([(5, 99999), (1, -4), (0, 3), (-1, 1)], np.int32)]
    seen = np.zeros(2, bool)
    with DeviceBuffers() as dev:
        for nf in (1, 63, 64, 65, 128, 129, 200):
            Z = seam_rows(nf, T, tone, hang, 1000 * hang + nf + T)
            for state in states:
                want, wst, _m = run.model(Z, nf, 0, state)
                got, gst, _m = run(dev, Z, nf, 0, state)
                what = "T %d, hang %d, %d frames, state %r" % (T, hang, nf, None if state is None else state.tolist())
                same_bytes(got, want, "dec: " + what)
                same_bytes(gst, wst, "the state: " + what)
                seen |= [bool((want[:, :3] == 0).any()), bool((want[:, :3] == 1).any())]
            # continued from the state the device wrote: the two halves are the whole
            if nf >= 64:
                a, sa, _m = run(dev, Z[:61], 61)
                b, sb, _m = run(dev, Z[61:], nf - 61, 0, sa)
                want, wst, _m = run.model(Z, nf)
                same_bytes(np.concatenate([a, b]), want, "cut at 61 of %d" % nf)
                same_bytes(sb, wst, "the state behind the cut")
            if nf == 200:
                d = np.diff(run.model(Z, nf)[0][:, :3].astype(int), axis=0)
                assert (d == -1).any() and (d == 1).any()
    assert seen.all()


def test_rows_that_are_not_finite_and_rows_on_the_thresholds():
    """NaN and +-Inf in the selected and in the other tones, e exactly open, close, one ulp below each, and exactly R: the model's classes"""
    T = 5
    run = Pass(4, T, 1)
    tone = [0, 4, 2, 2]
    ratio = np.array([0.0, 4.0, 1.0, 0.0], np.float32)
    nan, inf = np.nan, np.inf
    rows = []

    def frame(*per_channel):
        rows.append(np.array(per_channel, np.complex64))

    z = [0.0] * T
    sel = lambda c, v, others=0.0: [v if t == tone[c] else others for t in range(T)]
    frame(sel(0, 4.0), sel(1, 6.0, 3.0), sel(2, 8.0, 8.0), sel(3, 10.0))                      # e == open everywhere; ch1: e = 36 = 4 * 9 = R; ch2: e == o
    frame(sel(0, nan), sel(1, 6.0, nan), sel(2, 8.0, inf), sel(3, inf, nan))                  # NaN selected: low; NaN others: never taken; Inf other: R = Inf
    frame(sel(0, 2.0), sel(1, 3.0), sel(2, 4.0), sel(3, 10.0))                                # e == close: hold (ch3: open == close: strong)
    frame(sel(0, np.float32(1.9999999)), sel(1, 3.0, np.float32(1.5000001)), sel(2, inf, inf), sel(3, -inf))   # below close; R just above e; Inf >= Inf
    frame(z, z, z, z)
    frame([complex(0, nan)] + z[1:], sel(1, 6.0, np.float32(3.0000002)), sel(2, 1e30, 1e30), sel(3, 1e-30))    # NaN in im; e just below R; overflow; underflow
    frame(sel(0, 4.0, inf), sel(1, inf, 1.0), sel(2, 8.0, nan), sel(3, 10.0, inf))            # ratio 0 and an Inf other: 0 Inf = NaN, nothing reaches it
    Z = np.array(rows, np.complex64)
    with DeviceBuffers() as dev:
        for hang in (0, 2):
            for guard in (0, 1, 3, 63):
                run.setting(tone, OPEN4, CLOSE4, ratio, guard, hang)
                want, wst, _m = run.model(Z, len(rows))
                got, gst, _m = run(dev, Z, len(rows))
                same_bytes(got, want, "dec, guard %d hang %d" % (guard, hang))
                same_bytes(gst, wst, "the state, guard %d hang %d" % (guard, hang))
        run.setting(tone, OPEN4, CLOSE4, ratio, 0, 0)
        want = run.model(Z, len(rows))[0]
        assert want[0].tolist() == [1, 1, 1, 1] and want[1].tolist() == [0, 1, 0, 1] and want[4].tolist() == [0, 0, 0, 0]
        assert want[6, 0] == 0 and want[6, 1] == 1 and want[3, 2] == 1 and want[5, 1] == 0


@pytest.mark.parametrize("W", (1, 3, 32))
@pytest.mark.parametrize("Cn", (1, 4, 64, 256))
def test_the_gate_at_every_fill(Cn, W):
    """every fill 0 .. W - 1, calls that complete no frame, one and several: the mask is the carrier mask ANDed with the decision in force, the state of
    a call without a frame is the state as read"""
    T = 2
    run = Pass(Cn, T, W)
    rng = np.random.default_rng(100 * Cn + W)
    tone = rng.integers(-1, T, Cn).astype(np.int32)
    tone[0] = 0
    o = np.full(Cn, 4.0, np.float32)
    run.setting(tone, o, o * np.float32(0.25), np.zeros(Cn, np.float32), 0, 1)
    state = np.stack([rng.integers(0, 2, Cn), rng.integers(0, 2, Cn)], axis=1).astype(np.int32)
    with DeviceBuffers() as dev:
        for fill in range(W):
            for nb in sorted({1, W - fill - 1, W - fill, 2 * W + 1} - {0}):
                nf = (fill + nb) // W
                Z = (rng.integers(0, 4, (nf, Cn, T)) * np.float32(1.0)).astype(np.complex64)
                cm = (rng.random((nb, Cn)) < 0.7).astype(np.uint8)
                for st in (state, None):
                    want, wst, wmask = run.model(Z, nb, fill, st, cm)
                    got, gst, gmask = run(dev, Z, nb, fill, st, cm)
                    what = "C %d, W %d, fill %d, %d blocks, state %s" % (Cn, W, fill, nb, "carried" if st is not None else "none")
                    same_bytes(got, want, "dec: " + what)
                    same_bytes(gst, wst, "the state: " + what)
                    same_bytes(gmask, wmask, "the mask: " + what)
                    if nf == 0:
                        same_bytes(gst, SQ.read_state(st, Cn, 1).astype(np.int32) * (tone >= 0)[:, None].astype(np.int32), "no frame: the state as read")


def test_footprint_of_the_pass():
    """dec, the state and the mask as three payloads between poisoned guards: exactly nf C, 8 C and nb C bytes change, every guard byte stays (both
    poison bytes), the rows and the state read are untouched; a NULL mask runs the decision alone"""
    Cn, T, W = 4, 7, 3
    run = Pass(Cn, T, W)
    tone = [0, 6, -1, 3]
    run.setting(tone, OPEN4, CLOSE4, [0.0, 0.5, 0.0, 0.0], 1, 1)
    rng = np.random.default_rng(5)
    state = np.array([(1, 1), (0, 0), (1, 0), (1, 1)], np.int32)
    with DeviceBuffers() as dev:
        for nb, fill in ((200 * W, 0), (5, 2), (1, 0), (4, 2)):
            nf = (fill + nb) // W
            Z = seam_rows(nf, T, tone, 1, nb) if nf else np.zeros((0, Cn, T), np.complex64)
            cm = (rng.random((nb, Cn)) < 0.7).astype(np.uint8)
            want, wst, wmask = run.model(Z, nb, fill, state, cm)
            d_fr = dev.put(np.ascontiguousarray(Z)) if nf else None
            d_in = dev.put(state)
            band = DeviceBanded(dev, [nf * Cn, 8 * Cn, nb * Cn], max(nb, 1) * Cn)
            for _poison in twice(band):
                assert dev.hip.hipMemcpy(band.ptr(2), C.c_void_p(cm.ctypes.data), C.c_size_t(cm.nbytes), 1) == 0
                run.p.tone_squelch_pass_device(d_fr, band.ptr(0) if nf else None, nb, fill, d_in, band.ptr(1), band.ptr(2))
                run.p.synchronize()
                band.check([want, wst, wmask], "%d blocks behind fill %d" % (nb, fill))
            same_bytes(dev.get(d_in, 2 * Cn, np.int32).reshape(Cn, 2), state, "the state read")
            if nf:
                same_bytes(dev.get(d_fr, Z.size, np.complex64).reshape(Z.shape), Z, "the rows")
            # the decision alone
            band = DeviceBanded(dev, [nf * Cn, 8 * Cn], max(nb, 1) * Cn)
            for _poison in twice(band):
                run.p.tone_squelch_pass_device(d_fr, band.ptr(0) if nf else None, nb, fill, d_in, band.ptr(1), None)
                run.p.synchronize()
                band.check([want, wst], "the decision alone, %d blocks behind fill %d" % (nb, fill))
    lib, h = _lib.lib(), run.p._h
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, 1, 1, None, None, None, 0, W, None) == -1          # no state to write
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, 1, 1, 2, 2, None, 0, W, None) == -1                # one buffer for both states
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, None, 1, None, 2, None, 0, W, None) == -1          # frames to decide and no rows
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, 1, None, None, 2, None, 0, W, None) == -1          # ... and nowhere to put them
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, 1, 1, None, 2, None, W, 1, None) == -1             # fill out of range
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, 1, 1, None, 2, None, -1, 1, None) == -1
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, 1, 1, None, 2, None, 0, -1, None) == -1
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, None, None, None, None, None, 0, 0, None) == 0
    run.p.set_tone_squelch(None)
    assert lib.fdc_pipeline_tone_squelch_pass_device(h, 1, 1, None, 2, None, 0, W, None) == -1             # the tone squelch is off


# ---- the gated and the packed audio -----------------------------------------------------------------------------------------------------------------------

FORMATS = (("f32", 1.0, np.float32), ("s16", 9000.0, np.int16))


@pytest.mark.parametrize("D,K", [(8, 64), (64, 1)], ids=["D8 K64", "D64 K1"])
@pytest.mark.parametrize("k", (0, 2), ids=[plan_ids[0], plan_ids[2]])
def test_gated_and_packed_audio(k, D, K):
    """the audio matrix is the ungated matrix of a second handle with the cells the model's COMBINED mask closes replaced by zero bits, and the packed
    audio is audio_pack_model's over that mask, in both formats, the stream cut 4 + 5"""
    T, S, W = SETTINGS[1]
    _name, N, chans, flags = PLANS[k]
    H = N - N // 2
    x = base(k, T, S, W)[0]
    dec, mask = whole(k, T, S, W, 1)
    taps = G.lowpass_taps(D, K) if K > 1 else np.array([0.75], np.float32)
    for fmt, scale, dt in FORMATS:
        un = plain(k, T, S, W, tones=False, audio=(D, taps, fmt, scale))
        gated = toned(k, T, S, W, 1, audio=(D, taps, fmt, scale))
        packed = toned(k, T, S, W, 1, audio=(D, taps, fmt, scale), packed=True)
        npb = APM.npb_of(un.lout, D)
        b0 = 0
        for n in (4, 5):
            xs = x[b0 * H:(b0 + n) * H]
            un.work(xs)
            mat = un.audio()
            assert mat.dtype == dt and np.count_nonzero(mat) > mat.size // 2
            gated.work(xs)
            same_bytes(gated.squelch(), mask[b0:b0 + n], "the mask of the gated handle, call at %d" % b0)
            same_bytes(gated.audio(), gate_audio(mat, mask[b0:b0 + n], un.lout, D), "%s D %d K %d: the gated matrix, call at %d" % (fmt, D, K, b0))
            outs = packed.work(xs)
            same_bytes(packed.squelch(), mask[b0:b0 + n], "the mask of the packed handle, call at %d" % b0)
            want, count = APM.pack(mat, mask[b0:b0 + n], npb)
            got = packed.audio_packed()
            assert got.size == count
            same_bytes(got, want, "%s D %d K %d: the packed audio, call at %d" % (fmt, D, K, b0))
            for c, (u, v) in enumerate(zip(outs, APM.unpack(want, mask[b0:b0 + n], npb))):
                same_bytes(u, v, "what work() returns, ch%d" % c)
            b0 += n
        assert "audio: pass, gated" in gated.describe() and "packed" in packed.describe() and "tone squelch: pass" in packed.describe()


# ---- the setting ------------------------------------------------------------------------------------------------------------------------------------------

def test_every_refusal():
    N, R, nb = 4096, 2, 4
    H = N - N // R
    T, S, W = 5, 16, 2
    lib = _lib.lib()
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    tone, thr, half, ratio = np.array([0, 1, 4, -1], np.int32), np.full(4, 4.0, np.float32), np.full(4, 2.0, np.float32), np.zeros(4, np.float32)
    inc = increments(4, T, S)

    def raw(p, t=tone, o=thr, c=half, r=ratio, n=4, guard=0, hang=0):
        ptr = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
        return lib.fdc_pipeline_set_tone_squelch(p._h, ptr(t, i32), ptr(o, f32), ptr(c, f32), ptr(r, f32), n, guard, hang)

    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    assert p.tone_squelch_setting() is None and p.tone_squelch_device() is None
    with pytest.raises(ValueError):
        p.tone_squelch()
    # the tones off, then the squelch off
    with pytest.raises(G.FdcError, match="tones"):
        p.set_tone_squelch(tone, thr)
    p.set_demod("fm", CYCLES)
    p.set_tones(inc, S, W)
    with pytest.raises(G.FdcError, match="squelch"):
        p.set_tone_squelch(tone, thr)
    p.set_levels(True)
    p.set_squelch(1.0, 0.5, 0)
    # each argument
    assert raw(p, n=3) == -1 and raw(p, n=5) == -1
    assert raw(p, t=np.array([0, 1, 5, -1], np.int32)) == -1 and raw(p, t=np.array([0, -2, 4, -1], np.int32)) == -1
    for bad in (np.nan, np.inf, -1.0):
        v = thr.copy()
        v[2] = bad
        assert raw(p, o=v) == -1 and raw(p, r=v) == -1
        v[2] = bad if bad < 0 or np.isnan(bad) else -np.inf
        assert raw(p, c=v) == -1
    assert raw(p, o=half, c=thr) == -1                                 # close above open
    assert raw(p, o=None) == -1 and raw(p, c=None) == -1 and raw(p, r=None) == -1
    assert raw(p, guard=-1) == -1 and raw(p, guard=64) == -1 and raw(p, hang=-1) == -1 and raw(p, hang=65536) == -1
    assert p.tone_squelch_setting() is None                            # each wrote nothing
    assert raw(p, guard=63, hang=65535) == 0
    st = p.tone_squelch_setting()
    assert st[0].tolist() == tone.tolist() and st[1].tolist() == thr.tolist() and st[2].tolist() == half.tolist() and st[4:] == (63, 65535)
    assert raw(p, t=np.array([0, 1, 5, -1], np.int32)) == -1 and p.tone_squelch_setting()[4:] == (63, 65535)      # a refusal keeps the setting in force
    # while it is on: the tones cannot go or change their shape, the squelch cannot go; other increments and other carrier thresholds may come
    with pytest.raises(G.FdcError, match="tone squelch"):
        p.set_tones(None)
    for other in ((increments(4, 6, S), S, W), (inc, 8, W), (inc, S, 3)):
        with pytest.raises(G.FdcError, match="tone squelch"):
            p.set_tones(*other)
    with pytest.raises(G.FdcError, match="tone squelch"):
        p.set_squelch(None)
    inc2 = inc.copy()
    inc2[0, 0] ^= 1
    p.set_tones(inc2, S, W)
    p.set_squelch(2.0, 1.0, 3)
    assert p.tones_setting()[1:] == (S, W) and p.squelch_setting()[2] == 3
    p.set_tone_squelch(None)
    assert p.tone_squelch_setting() is None and p.tone_squelch_device() is None
    p.set_tones(None)
    p.set_squelch(None)
    # a pipelined sinks batch inside the handle
    from test_fine_tuning_gpu import signal
    q = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, lookahead=True, max_blocks=nb, **SINKS_KW)
    q.work(signal(nb * H, 2), sinks=bank)
    with pytest.raises(G.FdcError, match="pipelined"):
        q.set_tone_squelch(tone, thr)
    while q.flush_sinks(bank) > 0:
        pass
    q.set_levels(True)
    q.set_squelch(1.0, 0.5, 0)
    q.set_demod("fm")
    q.set_tones(inc, S, W)
    assert raw(q) == 0


def test_what_resets_the_stream_and_the_getter():
    """a gap, a reset, a new setting (the state only: the tones' fill goes on), a refused call; the getter takes the capacity"""
    k, (T, S, W), hang = 0, SETTINGS[1], 3
    _name, N, chans, _flags = PLANS[k]
    H = N - N // 2
    x, Z, cm, thr_o, thr_c, tone, o, c, r = base(k, T, S, W)
    p = toned(k, T, S, W, hang)
    lib = _lib.lib()
    buf = np.full(64, 0xAB, np.uint8)
    nf = C.c_int32(-5)
    assert lib.fdc_pipeline_tone_squelch(p._h, buf.ctypes.data, buf.nbytes, 3, C.byref(nf)) == -1                  # no call yet
    model = M.Stream(len(chans), W)
    setting = (tone, o, c, r, GUARD, hang)

    def both(first, b0, n, what):
        p.work(x[b0 * H:(b0 + n) * H])
        fill = model.fill if first == model.next else 0
        f0 = b0 // W if fill == 0 else (b0 - fill) // W
        wd, wm = model.call(first, Z[f0:f0 + (fill + n) // W], cm[b0:b0 + n], *setting)
        same_bytes(p.tone_squelch(), wd, "dec: " + what)
        same_bytes(p.squelch(), wm, "the mask: " + what)
        return wd, wm

    both(0, 0, 5, "the first call")                                    # blocks 0 .. 4: fill 1 behind it
    full = p.tone_squelch()
    assert full.shape == (2, len(chans))
    assert lib.fdc_pipeline_tone_squelch(p._h, buf.ctypes.data, full.size - 1, 5, C.byref(nf)) == -1 and nf.value == -5 and (buf == 0xAB).all()
    assert lib.fdc_pipeline_tone_squelch(p._h, buf.ctypes.data, buf.nbytes, 4, C.byref(nf)) == -1 and (buf == 0xAB).all()
    assert lib.fdc_pipeline_tone_squelch(p._h, buf.ctypes.data, full.size, 5, C.byref(nf)) == 0 and nf.value == 2
    assert buf[:full.size].tobytes() == full.tobytes() and (buf[full.size:] == 0xAB).all()
    with pytest.raises((G.FdcError, ValueError)):
        p.work(np.zeros((NB + 1) * H, np.complex64))                  # above max_blocks: refused, the state stays
    wd, wm = both(5, 5, 2, "the second call continues")                # blocks 5, 6: completes frame 2 (blocks 4, 5)
    assert wd.shape[0] == 1
    # a new setting restarts the state only: fill 1 stays, block 7 completes frame 3 with block 6, in front of it every gated channel is closed
    p.set_tone_squelch(*setting)
    model.restart()
    wd, wm = both(7, 7, 2, "behind a new setting")
    assert wd.shape[0] == 1 and (wm[:1, tone >= 0] == 0).all()
    # a reset: block 0 anew
    p.reset()
    both(0, 0, 4, "behind a reset")
    # one block: no frame completed, nothing to copy
    p.work(x[4 * H:5 * H])
    model.call(4, Z[2:2], cm[4:5], *setting)
    assert lib.fdc_pipeline_tone_squelch(p._h, None, 0, 1, C.byref(nf)) == 0 and nf.value == 0 and p.tone_squelch().shape == (0, len(chans))
    # the same tones again keep both streams (a call elsewhere in the stream: test_device_entries)
    p.reset()
    p.work(x[:3 * H])
    p.set_tones(increments(len(chans), T, S), S, W)
    p.work(x[3 * H:4 * H])
    same_bytes(p.tone_squelch(), whole(k, T, S, W, hang)[0][1:2], "the same tones again keep the stream")


def test_no_channels():
    N, R, nb = 4096, 2, 3
    from test_fine_tuning_gpu import signal
    p = G.Pipeline(N, R, [], max_blocks=nb, keep_spectrum=True)
    p.set_levels(True)
    p.set_squelch(1.0)
    p.set_demod("fm")
    p.set_tones(np.zeros((0, 3), np.uint32), 16, 2)
    p.set_tone_squelch(np.zeros(0, np.int32), 1.0)
    outs, spec = p.work(signal(nb * (N - N // R), 1), want_spectrum=True)
    assert outs == [] and np.abs(spec).max() > 0 and "tone squelch" not in p.describe()
    assert p.tone_squelch_setting()[4:] == (0, 0)
    p.set_tone_squelch(None)
    assert p.tone_squelch_setting() is None


@pytest.mark.parametrize("k", (0, 2), ids=[plan_ids[0], plan_ids[2]])
def test_device_entries(k):
    """process_device over a ring: 0..3 then 3..7 continue the stream; 4..7 behind it is a call elsewhere and starts anew; dec, the mask and the device
    buffers are the model's"""
    T, S, W = SETTINGS[1]
    hang = 1
    _name, N, chans, flags = PLANS[k]
    H, ovl = N - N // 2, N // 2
    x, Z, cm, thr_o, thr_c, tone, o, c, r = base(k, T, S, W)
    ring = np.concatenate([np.zeros(ovl, np.complex64), x])
    p = toned(k, T, S, W, hang)
    ref = plain(k, T, S, W)
    ref.set_squelch(thr_o, thr_c, 1)
    model = M.Stream(len(chans), W)
    with DeviceBuffers() as dev:
        for j, (first, n) in enumerate(((0, 3), (3, 4), (4, 3), (4, 3))):
            d_in = dev.put(np.ascontiguousarray(ring[first * H:first * H + ovl + n * H]))
            d_o = dev.put(np.zeros(p.output_samples(n), np.float32))
            d_r = dev.put(np.zeros(p.output_samples(n), np.float32))
            ref.process_device(d_in, first, n, d_r)
            ref.synchronize()
            p.process_device(d_in, first, n, d_o)
            p.synchronize()
            same_bytes(dev.get(d_o, p.output_samples(n), np.float32), dev.get(d_r, p.output_samples(n), np.float32), "d_out of call %d" % j)
            wd, wm = model.call(first, ref.tones(n), ref.squelch(n), tone, o, c, r, GUARD, hang)
            same_bytes(p.tone_squelch(n), wd, "dec of call %d" % j)
            same_bytes(p.squelch(n), wm, "the mask of call %d" % j)
            if wd.size:
                same_bytes(dev.get(C.c_void_p(p.tone_squelch_device()), wd.size, np.uint8).reshape(wd.shape), wd, "tone_squelch_device()")
            same_bytes(dev.get(C.c_void_p(p.squelch_device()), wm.size, np.uint8).reshape(wm.shape), wm, "squelch_device()")
        assert model.next == 7 and model.fill == 1


@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_the_feature_off_changes_nothing(k):
    """a handle that had the tone squelch on and switched it off, and one that never had it: the mask, the audio, the packed audio and the rows of both
    are the same bytes, and neither says it ran"""
    T, S, W = SETTINGS[1]
    D, taps = 8, G.lowpass_taps(8, 64)
    x, Z, cm, thr_o, thr_c, tone, o, c, r = base(k, T, S, W)
    for packed in (False, True):
        never = plain(k, T, S, W, audio=(D, taps))
        never.set_squelch(thr_o, thr_c, 1)
        was = toned(k, T, S, W, 1, audio=(D, taps))
        was.work(x)
        was.set_tone_squelch(None)
        was.reset()
        for h in (never, was):
            if packed:
                h.set_audio_packing(True)
        a, b = never.work(x), was.work(x)
        same_bytes(was.squelch(), never.squelch(), "the mask")
        same_bytes(never.squelch(), cm, "the carrier mask")
        same_bytes(was.tones(), never.tones(), "the rows")
        same_bytes(was.audio_packed() if packed else was.audio(), never.audio_packed() if packed else never.audio(), "the audio, packed %r" % packed)
        for cidx, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, "what work() returns, ch%d" % cidx)
        assert "tone squelch" not in never.describe() and "tone squelch" not in was.describe()
        with pytest.raises(ValueError):
            was.tone_squelch()


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
p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pw = G.Pipeline(8192, 2, MIXED, max_blocks=nb, host_sub_blocks=3)
pd = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
for h, mode in ((p, "fm"), (pw, "mag"), (pd, "fm")):
    h.set_levels(True)
    h.set_squelch(1e-3, 1e-4, 1)
    h.set_demod(mode, 0.5)
    h.set_audio(8, G.lowpass_taps(8, 32))
    h.set_tones(inc, 16, 3)
    h.set_tone_squelch(7, 1e-3, 1e-4, 0.5, 1, 2)
p.set_audio_packing(True)
Cn = 4
d_ring, d_out, d_fr, d_dec, d_s0, d_s1, d_m = (C.c_void_p() for _ in range(7))
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(4 * pd.output_samples(nb))) == 0
assert hip.hipMalloc(C.byref(d_fr), C.c_size_t(8 * Cn * 50 * 4)) == 0 and hip.hipMemset(d_fr, 0, C.c_size_t(8 * Cn * 50 * 4)) == 0
assert hip.hipMalloc(C.byref(d_dec), C.c_size_t(Cn * 4)) == 0 and hip.hipMalloc(C.byref(d_m), C.c_size_t(Cn * nb)) == 0
assert hip.hipMemset(d_m, 1, C.c_size_t(Cn * nb)) == 0
assert hip.hipMalloc(C.byref(d_s0), C.c_size_t(8 * Cn)) == 0 and hip.hipMalloc(C.byref(d_s1), C.c_size_t(8 * Cn)) == 0 and hip.hipMemset(d_s0, 0, C.c_size_t(8 * Cn)) == 0
blk = [0]

def device():
    pd.process_device(d_ring, blk[0], nb, d_out)          # a stream that goes on: the state is used and swapped, frames straddle the calls
    blk[0] += nb
    pd.synchronize()
    pd.tone_squelch(nb)
    pd.squelch(nb)

def the_pass():
    pd.tone_squelch_pass_device(d_fr, d_dec, nb, 2, d_s0, d_s1, d_m)
    pd.synchronize()

entries = {"fdc_pipeline_work (path 5, packed)": lambda: (p.work(x), p.tone_squelch(), p.squelch()),
           "fdc_pipeline_work (spectrum path, sub-batches)": lambda: (pw.work(x2), pw.tone_squelch()),
           "fdc_pipeline_process_device and fdc_pipeline_tone_squelch": device,
           "fdc_pipeline_tone_squelch_pass_device": the_pass,
           "another setting before every call": lambda: (p.set_tone_squelch(3, 1e-2, 1e-3, 0.0, 0, 0), p.work(x), p.set_tone_squelch(7, 1e-3, 1e-4, 0.5, 1, 2), p.work(x)),
           "off and on again": lambda: (pw.set_tone_squelch(None), pw.set_tone_squelch(7, 1e-3, 1e-4, 0.5, 1, 2), pw.work(x2))}
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
assert all("tone squelch: pass" in h.describe() for h in (p, pw, pd)), (p.describe(), pw.describe(), pd.describe())
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
    from test_fine_tuning_gpu import signal
    N, R, nb = 4096, 2, 6
    H = N - N // R
    x = signal(2 * nb * H, 11)
    S, W = 16, 2
    inc1 = G.tone_increments(G.ctcss_tones(), 25000.0, S)
    common = dict(inptype=8, demod="fm", demod_gain=CYCLES, levels=True, squelch_db=-60.0, squelch_hang=1, tones=inc1, tone_group=S, tone_frame=W)
    off = G.FrequencyDomainChannelizer(**common, **KW)
    rows, masks = [], []
    for xs in (x[:nb * H], x[nb * H:]):
        off.work(xs)
        rows.append(off.tones)
        masks.append(off.squelch)
    Cn = rows[0].shape[1]
    tone = np.array([3, -1, 40][:Cn] + [0] * max(0, Cn - 3), np.int32)
    e = np.array([[M.energies(z[c])[max(int(tone[c]), 0)] for c in range(Cn)] for z in np.concatenate(rows)], np.float32)
    o = np.median(e.astype(np.float64), axis=0).astype(np.float32)
    c = (o * np.float32(0.5)).astype(np.float32)
    on = G.FrequencyDomainChannelizer(tone_squelch=tone, tone_open=o, tone_close=c, tone_ratio=0.0, tone_guard=2, tone_hang=1, **common, **KW)
    st = on.pipeline.tone_squelch_setting()
    assert st[0].tolist() == tone.tolist() and st[1].tobytes() == o.tobytes() and st[4:] == (2, 1)
    model = M.Stream(Cn, W)
    seen = set()
    for j, xs in enumerate((x[:nb * H], x[nb * H:])):
        on.work(xs)
        wd, wm = model.call(j * nb, rows[j], masks[j], tone, o, c, np.zeros(Cn, np.float32), 2, 1)
        same_bytes(on.tone_squelch_dec, wd, "hier block: dec of call %d" % j)
        same_bytes(on.squelch, wm, "hier block: the mask of call %d" % j)
        same_bytes(on.tones, rows[j], "hier block: the rows of call %d" % j)
        seen |= set(wd[:, tone >= 0].ravel().tolist())
    assert seen == {0, 1}
    on.work(x[:0])
    assert on.tone_squelch_dec.shape == (0, Cn)
    with pytest.raises(ValueError):
        G.FrequencyDomainChannelizer(tone_squelch=0, tone_open=1.0, inptype=8, demod="fm", tones=inc1, **KW)        # without squelch_db
