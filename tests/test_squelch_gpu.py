"""GPU tests (-m gpu) of the channel squelch (fdc_pipeline_set_squelch and its kin; include/fdc_amd.h): the decision on the device and the gated audio.

THE REFERENCE FOR BITS is tests/squelch_model.py fed with the handle's own levels (whose bits do not depend on how the stream is cut: the levels'
contract, tests/test_levels_gpu.py): the mask must equal the model's BYTE FOR BYTE, so no tolerance appears anywhere.  The gated audio is held to
the ungated audio of a second handle with the closed (row, channel) segments replaced by zero bits.

THE STREAM: one tone a little off every channel's centre (so that the FM audio is not zero), keyed per (block, channel) between three amplitudes a
decade of power apart (SEQS: 2 strong, 1 middle, 0 low), over a little noise.  The thresholds are the geometric means: the strongest block's power
of the channel times 10^-0.5 and 10^-1.5.  Every stream test asserts on the model's mask that every channel shows both values, a closure (every closure is a hang expiry), a middle block that holds the
channel open and a reopening: a test that never closes hides everything."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
import squelch_model as S
from footprint import DeviceBanded, twice
from test_demod_gpu import CYCLES, KW, SINKS_KW
from test_fine_tuning_gpu import BANK
from test_fine_tuning_routes_gpu import DeviceBuffers
from test_iq_input_gpu import EXAMPLE, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = [("path 5", 4096, EXAMPLE, 0), ("example plan, spectrum path", 4096, EXAMPLE, G.FDC_PIPE_NO_FUSED), ("bank", 16384, BANK, 0)]
plan_ids = [f[0] for f in PLANS]
NB = 9
SEQS = ((2, 1, 0, 0, 0, 0, 2, 0, 0), (0, 2, 1, 0, 0, 0, 0, 2, 1), (2, 1, 1, 0, 0, 0, 0, 2, 0))
AMP = (0.1, 10.0 ** -0.5, 1.0)                # powers 0.01, 0.1, 1
HANGS = (0, 1, 3, 100)
FORMATS = (("f32", 1.0, np.float32), ("s16", 9000.0, np.int16))


def keyed(N, R, chans, nb=NB, seed=0):
    H = N - N // R
    rng = np.random.default_rng(seed)
    t = np.arange(nb * H, dtype=np.float64)
    x = 1e-3 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    for c, (f, l, _p, _s) in enumerate(chans):
        amp = np.repeat(np.array([AMP[k] for k in np.resize(SEQS[c % 3], nb)]), H)
        x += amp * np.exp(2j * np.pi * (((f + 0.513 * l) / N - 0.5) * t + rng.uniform()))
    return x.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def stream(k):
    """(x, power[NB][C] of a handle with the levels alone, open thresholds, close thresholds): computed once and left unchanged"""
    _name, N, chans, flags = PLANS[k]
    x = keyed(N, 2, chans, seed=k)
    p = G.Pipeline(N, 2, chans, max_blocks=NB, flags=flags)
    p.set_levels(True)
    p.work(x)
    power = p.levels()[:, :, 0].copy()
    top = power.max(axis=0)
    thr_o, thr_c = (top * np.float32(10.0 ** -0.5)).astype(np.float32), (top * np.float32(10.0 ** -1.5)).astype(np.float32)
    for a in (x, power, thr_o, thr_c):
        a.setflags(write=False)
    return x, power, thr_o, thr_c


def shows_everything(mask, power, thr_o, thr_c, what):
    """the model's mask of a whole stream: both values, a closure, a hold by a middle block and a reopening, in every channel"""
    strong, low = S.classes(power, None, thr_o, thr_c)
    for c in range(mask.shape[1]):
        m = mask[:, c].astype(int)
        d = np.diff(m)
        assert m.min() == 0 and m.max() == 1, (what, c, m.tolist())
        assert (d == -1).any(), (what, "no closure", c, m.tolist())
        assert (~strong[:, c] & ~low[:, c] & (m == 1)).any(), (what, "no hold by a middle block", c, m.tolist())
        first_open = int(np.argmax(m))
        assert (d[first_open:] == 1).any(), (what, "no reopening", c, m.tolist())


def squelched(N, chans, thr_o, thr_c, hang, nb=NB, flags=0, **kw):
    p = G.Pipeline(N, 2, chans, max_blocks=nb, flags=flags, **kw)
    p.set_levels(True)
    p.set_squelch(thr_o, thr_c, hang)
    return p


# ---- the mask of a stream ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hang", HANGS)
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_mask_against_the_model(k, hang):
    """1, 2, 3, 5 and 9 blocks from a stream start: the mask is the model's over the handle's own levels of the call"""
    _name, N, chans, flags = PLANS[k]
    H = N - N // 2
    x, power, thr_o, thr_c = stream(k)
    p = squelched(N, chans, thr_o, thr_c, hang, flags=flags)
    st = p.squelch_setting()
    assert st[0].tobytes() == thr_o.tobytes() and st[1].tobytes() == thr_c.tobytes() and st[2] == hang
    for nb in (1, 2, 3, 5, 9):
        p.reset()
        p.work(x[:nb * H])
        lev = p.levels()[:, :, 0]
        same_bytes(lev, power[:nb], "the levels of %d blocks" % nb)
        want, _state = S.squelch(lev, None, thr_o, thr_c, hang)
        got = p.squelch()
        assert got.shape == (nb, len(chans)) and got.dtype == np.uint8
        same_bytes(got, want, "hang %d, %d blocks" % (hang, nb))
    assert "squelch: pass" in p.describe() and "levels: pass" in p.describe()
    if hang < NB:
        shows_everything(want, power, thr_o, thr_c, "hang %d" % hang)
    else:
        assert want.any() and not want.all() and (np.diff(want.astype(int), axis=0) >= 0).all()       # opened, and the hang never ran out


@pytest.mark.parametrize("hang", (1, 3))
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_cuts_of_the_stream_give_the_same_bits(k, hang):
    """9 blocks as 9, 4 + 5, 1 + 1 + 7 and 9 x 1; host_sub_blocks = 2 (five enqueue-path calls whose rows append and whose states link) and
    chunk_blocks = 2 (launch groups inside one enqueue call: one decision over the whole call)"""
    _name, N, chans, flags = PLANS[k]
    H = N - N // 2
    x, power, thr_o, thr_c = stream(k)
    whole, _state = S.squelch(power, None, thr_o, thr_c, hang)
    shows_everything(whole, power, thr_o, thr_c, "hang %d" % hang)
    for cut in ((9,), (4, 5), (1, 1, 7), (1,) * 9):
        p = squelched(N, chans, thr_o, thr_c, hang, flags=flags)
        model, b0 = S.Stream(len(chans)), 0
        for j, n in enumerate(cut):
            p.work(x[b0 * H:(b0 + n) * H])
            want = model.call(b0, p.levels()[:, :, 0], None, thr_o, thr_c, hang)
            same_bytes(p.squelch(), want, "cut %r, call %d" % (cut, j))
            same_bytes(want, whole[b0:b0 + n], "the model: cut %r, call %d" % (cut, j))
            b0 += n
    for kw in (dict(host_sub_blocks=2), dict(chunk_blocks=2), dict(chunk_blocks=2, host_sub_blocks=3)):
        p = squelched(N, chans, thr_o, thr_c, hang, flags=flags, **kw)
        p.work(x)
        same_bytes(p.levels()[:, :, 0], power, "levels, %r" % kw)
        same_bytes(p.squelch(), whole, repr(kw))


# ---- the decision alone, on hand-made powers --------------------------------------------------------------------------------------------------------------

SEAM_COUNTS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8200)
SEAM_HANGS = (0, 1, 2, 5, 70)
OPEN, CLOSE = np.array([10, 20, 30, 40], np.float32), np.array([4, 8, 12, 40], np.float32)


def seam_powers(nb, hang, seed):
    """[nb][4] float32: seeded classes, mostly low; behind every boundary of the kernel's scans that the call holds (a lane's 16 blocks, 64, 256, a wave's
    1024, a trip's 4096) a strong block a little in front and low blocks across it, so that a closing run straddles it; NaN, +-Inf and the thresholds
    themselves at fixed places"""
    rng = np.random.default_rng(seed)
    cls = rng.choice(3, size=(nb, 4), p=(0.86, 0.08, 0.06))
    for b in (16, 64, 256, 1024, 4096):
        for c in range(4):
            s = b - 1 - (hang * (c + 1)) // 4 - c % 2
            if s >= 0 and b + hang + 3 <= nb:
                cls[s, c] = 2
                cls[s + 1:b + hang + 3, c] = 0
    # per channel: low = Tc / 2, middle = (To + Tc) / 2 (channel 3: To = Tc, no middle: it counts as strong), strong = 1.5 To
    p = np.where(cls == 2, 1.5 * OPEN[None, :], np.where(cls == 1, 0.5 * (OPEN + CLOSE)[None, :], 0.5 * CLOSE[None, :])).astype(np.float32)
    special = ((3, 0, np.nan), (5, 1, np.inf), (6, 1, -np.inf), (10, 2, OPEN[2]), (11, 2, CLOSE[2]), (12, 2, np.nextafter(CLOSE[2], np.float32(0))),
               (70, 0, np.nan), (71, 0, OPEN[0]), (300, 3, np.inf), (301, 3, np.nan), (600, 1, CLOSE[1]), (2050, 0, -np.inf), (4100, 2, np.nan), (4101, 2, OPEN[2]))
    for m, c, v in special:
        if m < nb:
            p[m, c] = v
    return p


def run_pass(p, dev, power, state):
    """fdc_pipeline_squelch_pass_device over hand-made powers: (mask, new state)"""
    nb, Cn = power.shape
    lev = np.zeros((nb, Cn, 2), np.float32)
    lev[:, :, 0] = power
    lev[:, :, 1] = 7.0                                                # (the peaks are not looked at)
    d_lev, d_mask = dev.put(lev), dev.put(np.full(nb * Cn, 0xEE, np.uint8))
    d_in = dev.put(np.ascontiguousarray(state, np.int32)) if state is not None else None
    d_out = dev.put(np.full(2 * Cn, -77, np.int32))
    p.squelch_pass_device(d_lev, d_mask, nb, d_in, d_out)
    p.synchronize()
    return dev.get(d_mask, nb * Cn, np.uint8).reshape(nb, Cn), dev.get(d_out, 2 * Cn, np.int32).reshape(Cn, 2)


@pytest.mark.parametrize("hang", SEAM_HANGS)
def test_scan_seams(hang):
    """every block count around the seams of the scans, every carried state (one per channel: closed, open with h = 0, h in the middle, h = hang), then
    the same call continued from the state it wrote: mask and state are the model's"""
    p = G.Pipeline(4096, 2, EXAMPLE, max_blocks=4)
    p.set_levels(True)
    p.set_squelch(OPEN, CLOSE, hang)
    carried = np.array([(0, 0), (1, 0), (1, (hang + 1) // 2), (1, hang)], np.int32)
    seen = np.zeros(2, bool)
    with DeviceBuffers() as dev:
        for nb in SEAM_COUNTS:
            power = seam_powers(nb, hang, 1000 * hang + nb)
            for state in (None, carried, carried[::-1].copy(), np.array([(5, 99999), (1, -4), (0, 3), (-1, 1)], np.int32)):
                want, wstate = S.squelch(power, None, OPEN, CLOSE, hang, state)
                got, gstate = run_pass(p, dev, power, state)
                same_bytes(got, want, "hang %d, %d blocks, state %r" % (hang, nb, None if state is None else state.tolist()))
                same_bytes(gstate, wstate, "the state behind hang %d, %d blocks, state %r" % (hang, nb, None if state is None else state.tolist()))
                seen |= [bool((want == 0).any()), bool((want == 1).any())]
            if nb >= 600:
                scan, _s = S.scan_classes(*S.classes(power, None, OPEN, CLOSE), hang, carried)
                assert scan.any() and (np.diff(scan.astype(int), axis=0) == -1).any() and (np.diff(scan.astype(int), axis=0) == 1).any()
    assert seen.all()
    lib = _lib.lib()
    assert lib.fdc_pipeline_squelch_pass_device(p._h, None, 1, None, 2, 1, None) == -1 and lib.fdc_pipeline_squelch_pass_device(p._h, 1, None, None, 2, 1, None) == -1
    assert lib.fdc_pipeline_squelch_pass_device(p._h, 1, 1, None, None, 1, None) == -1          # no state to write
    assert lib.fdc_pipeline_squelch_pass_device(p._h, 1, 1, 2, 2, 1, None) == -1                # one buffer for both states
    assert lib.fdc_pipeline_squelch_pass_device(p._h, None, None, None, None, 0, None) == 0 and lib.fdc_pipeline_squelch_pass_device(p._h, 1, 1, None, 2, -1, None) == -1
    p.set_squelch(None)
    assert lib.fdc_pipeline_squelch_pass_device(p._h, 1, 1, None, 2, 1, None) == -1             # the squelch is off


def test_gains_scale_the_thresholds():
    """gains of 0.03 .. 30 with the thresholds unchanged: the mask of the model's g2 products, on powers that follow the gain (so the same classes come
    out, up to rounding at the thresholds themselves, which the model decides) and in a whole stream with the gains on.  Gain 0: both threshold products
    are +0, which every power that is not NaN reaches (the rule as stated: p >= To), so the model's mask is open wherever p is a number"""
    p = G.Pipeline(4096, 2, EXAMPLE, max_blocks=NB)
    p.set_levels(True)
    p.set_squelch(OPEN, CLOSE, 2)
    base = seam_powers(700, 2, 5)
    with DeviceBuffers() as dev:
        for gains in ([0.03, 0.3, 3.0, 30.0], [30.0, 1.0, 0.03, 7.5], [0.0, 1.0, 0.0, 2.0]):
            g = np.array(gains, np.float32)
            p.set_gains(g)
            power = (base * (g * g)[None, :]).astype(np.float32)
            power[40:60, 0] = 0.0
            want, wstate = S.squelch(power, g, OPEN, CLOSE, 2)
            got, gstate = run_pass(p, dev, power, None)
            same_bytes(got, want, "gains %r" % gains)
            same_bytes(gstate, wstate, "the state, gains %r" % gains)
            assert want.any() and not want.all()
        assert want[:, 0].all() and np.isnan(power[3, 0])              # gain 0: a power of +0 reaches a product of +0 (the lone NaN blocks are low, and the hang holds them)
    # a stream with the gains on: the thresholds stay those of the ungained powers
    _name, N, chans, flags = PLANS[0]
    x, power, thr_o, thr_c = stream(0)
    plain, _s = S.squelch(power, None, thr_o, thr_c, 1)
    g = np.array([0.03, 0.5, 4.0, 30.0], np.float32)
    q = squelched(N, chans, thr_o, thr_c, 1)
    q.set_gains(g)
    q.work(x)
    want, _s = S.squelch(q.levels()[:, :, 0], g, thr_o, thr_c, 1)
    same_bytes(q.squelch(), want, "a stream with gains")
    same_bytes(want, plain, "the gains do not defeat the thresholds")
    assert "gains:" in q.describe()


# ---- the gated audio ------------------------------------------------------------------------------------------------------------------------------------

def gate(mat, mask, lout, D):
    """the ungated audio matrix [nb][A] with the columns of closed (row, channel) pairs replaced by zero bits"""
    out, at = mat.copy(), 0
    for c, lo in enumerate(lout):
        out[mask[:, c] == 0, at:at + lo // D] = 0
        at += lo // D
    return out


@pytest.mark.parametrize("D,K", [(8, 64), (1, 256), (64, 1)], ids=["D8 K64", "D1 K256", "D64 K1"])
@pytest.mark.parametrize("k", (0, 2), ids=[plan_ids[0], plan_ids[2]])
def test_gated_audio(k, D, K):
    """the same stream through a handle with the squelch and one without: the gated audio is the ungated one with the closed segments zeroed, in both
    formats.  hang = 1; the stream is cut 6 + 3: channels 0, 3, .. reopen at block 6, the first of the second call, the others at block 7, in its middle:
    behind the opening the audio has the bits of the ungated pass, so the history ran on through the closed blocks"""
    _name, N, chans, flags = PLANS[k]
    H = N - N // 2
    x, power, thr_o, thr_c = stream(k)
    taps = G.lowpass_taps(D, K) if K > 1 else np.array([0.75], np.float32)
    whole, _s = S.squelch(power, None, thr_o, thr_c, 1)
    shows_everything(whole, power, thr_o, thr_c, "hang 1")
    assert whole[5, 0] == 0 and whole[6, 0] == 1 and whole[6, 1] == 0 and whole[7, 1] == 1
    for fmt, scale, dt in FORMATS:
        un = G.Pipeline(N, 2, chans, max_blocks=NB, flags=flags)
        un.set_levels(True)
        on = squelched(N, chans, thr_o, thr_c, 1, flags=flags)
        for h in (un, on):
            h.set_demod("fm", CYCLES)
            h.set_audio(D, taps, fmt, scale)
        b0 = 0
        for n in (6, 3):
            un.work(x[b0 * H:(b0 + n) * H])
            outs = on.work(x[b0 * H:(b0 + n) * H])
            mask = on.squelch()
            same_bytes(mask, whole[b0:b0 + n], "the mask, call at %d" % b0)
            plain = un.audio()
            assert plain.dtype == dt and np.count_nonzero(plain) > plain.size // 2
            want = gate(plain, mask, on.lout, D)
            same_bytes(on.audio(), want, "%s D %d K %d, call at %d" % (fmt, D, K, b0))
            same_bytes(np.concatenate(outs), np.concatenate(G.audio_channels(want, on.lout, D)), "what work() returns")
            b0 += n
        assert "audio: pass, gated" in on.describe() and "squelch: pass" in on.describe() and "gated" not in un.describe()
    # the demodulated ports of a device entry are not gated
    ovl = N // 2
    ring = np.concatenate([np.zeros(ovl, np.complex64), x])
    with DeviceBuffers() as dev:
        d_in = dev.put(ring)
        res = []
        for h in (un, on):
            d_o = dev.put(np.zeros(h.output_samples(NB), np.float32))
            h.process_device(d_in, 0, NB, d_o)
            h.synchronize()
            res.append(dev.get(d_o, h.output_samples(NB), np.float32))
        same_bytes(res[1], res[0], "d_out of a device entry")
        same_bytes(on.squelch(NB), whole, "the mask of a device entry")
        same_bytes(dev.get(C.c_void_p(on.squelch_device()), NB * len(chans), np.uint8).reshape(NB, -1), whole, "squelch_device()")
        same_bytes(on.audio(NB), gate(un.audio(NB), whole, on.lout, D), "the audio of a device entry")


@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_mask_only(k):
    """with the audio off, and with the demodulation off too, the squelch gives the mask and the call's outputs are those of a handle without it"""
    _name, N, chans, flags = PLANS[k]
    x, power, thr_o, thr_c = stream(k)
    whole, _s = S.squelch(power, None, thr_o, thr_c, 1)
    for demod in (None, "fm", "mag"):
        un = G.Pipeline(N, 2, chans, max_blocks=NB, flags=flags)
        un.set_levels(True)
        on = squelched(N, chans, thr_o, thr_c, 1, flags=flags)
        for h in (un, on):
            if demod:
                h.set_demod(demod, 0.5)
        a, b = un.work(x), on.work(x)
        for c in range(len(chans)):
            same_bytes(b[c], a[c], "demod %r, the port of ch%d" % (demod, c))
        same_bytes(on.squelch(), whole, "demod %r, the mask" % (demod,))
        same_bytes(on.levels(), un.levels(), "the levels")
        assert "audio" not in on.describe() and on.describe() == un.describe() + "; squelch: pass"


# ---- the setting ---------------------------------------------------------------------------------------------------------------------------------------

def test_setting_semantics():
    _name, N, chans, flags = PLANS[0]
    H = N - N // 2
    x, power, thr_o, thr_c = stream(0)
    lib = _lib.lib()
    fp = C.POINTER(C.c_float)
    p = G.Pipeline(N, 2, chans, max_blocks=NB)
    # off by default; refused while the levels are off
    assert p.squelch_setting() is None and p.squelch_device() is None and "squelch" not in p.describe()
    with pytest.raises(G.FdcError) as e:
        p.set_squelch(thr_o, thr_c, 1)
    assert e.value.status == -1 and "levels" in str(e.value) and p.squelch_setting() is None
    with pytest.raises(ValueError):
        p.squelch()
    p.set_levels(True)
    p.set_squelch(thr_o, thr_c, 1)
    assert p.squelch_device() is not None
    buf = np.full(NB * 4, 0xA5, np.uint8)
    assert lib.fdc_pipeline_squelch(p._h, buf.ctypes.data, buf.nbytes, NB) == -1 and (buf == 0xA5).all()      # no call yet
    p.work(x[:2 * H])
    m0 = p.squelch()
    before = p.squelch_setting()
    # every refusal leaves the setting and the state as they were
    o, c = thr_o.copy(), thr_c.copy()
    bad_o, neg, nan = thr_c * np.float32(0.5), -thr_o, np.full(4, np.nan, np.float32)
    ptr = lambda a: a.ctypes.data_as(fp)
    for args in ((ptr(o), ptr(c), 3, 1), (ptr(o), ptr(c), 5, 1), (ptr(nan), ptr(c), 4, 1), (ptr(o), ptr(nan), 4, 1), (ptr(neg), ptr(neg), 4, 1),
                 (ptr(bad_o), ptr(c), 4, 1), (ptr(o), ptr(c), 4, -1), (ptr(o), ptr(c), 4, 65536), (ptr(o), None, 4, 1), (None, None, 3, 0)):
        assert lib.fdc_pipeline_set_squelch(p._h, *args) == -1, args[2:]
        now = p.squelch_setting()
        assert now[0].tobytes() == before[0].tobytes() and now[1].tobytes() == before[1].tobytes() and now[2] == before[2]
    with pytest.raises(G.FdcError) as e:
        p.set_levels(False)
    assert e.value.status == -1 and "squelch" in str(e.value) and p.levels().shape == (2, 4, 2)
    with pytest.raises(G.FdcError):
        p.work(np.zeros((NB + 1) * H, np.complex64))                  # above max_blocks: refused
    with pytest.raises(G.FdcError):
        p.work_spectrum(np.zeros(2 * N, np.complex64))                # refused under the levels
    p.work(x[2 * H:])
    whole, _s = S.squelch(power, None, thr_o, thr_c, 1)
    same_bytes(np.concatenate([m0, p.squelch()]), whole, "behind the refused calls the stream went on")
    # the getter's capacity rule
    need = 7 * 4
    buf = np.full(need + 64, 0xA5, np.uint8)
    for cap, nb in ((need - 1, 7), (0, 7), (need + 64, 6), (need + 64, 8)):
        assert lib.fdc_pipeline_squelch(p._h, buf.ctypes.data, cap, nb) == -1 and (buf == 0xA5).all()
    assert "bytes" in lib.fdc_last_error().decode() or "blocks" in lib.fdc_last_error().decode()
    assert lib.fdc_pipeline_squelch(p._h, None, need, 7) == -1
    assert lib.fdc_pipeline_squelch(p._h, buf.ctypes.data, need, 7) == 0 and (buf[need:] == 0xA5).all()
    same_bytes(buf[:need].reshape(7, 4), whole[2:], "the raw getter")
    # the setting survives reset(), the state does not
    p.reset()
    assert p.squelch_setting()[2] == 1 and "squelch" not in p.describe()
    p.work(x[2 * H:])
    fresh, _s = S.squelch(p.levels()[:, :, 0], None, thr_o, thr_c, 1)
    same_bytes(p.squelch(), fresh, "after reset() every channel starts closed")
    assert fresh.tobytes() != whole[2:].tobytes()
    # new thresholds keep `open`; a smaller hang clamps h.  Blocks 0 .. 1 with hang 100 leave the channels that opened at (1, 100 or 99); then hang 0
    # and thresholds no power reaches: the model continued from the state with the new setting
    p.reset()
    p.set_squelch(thr_o, thr_c, 100)
    model = S.Stream(4)
    p.work(x[:2 * H])
    same_bytes(p.squelch(), model.call(0, p.levels()[:, :, 0], None, thr_o, thr_c, 100), "hang 100")
    assert model.state[:, 0].any() and model.state[:, 1].max() >= 99
    high = (thr_o * np.float32(1e6)).astype(np.float32)
    p.set_squelch(high, thr_c, 0)
    p.work(x[2 * H:5 * H])
    want = model.call(2, p.levels()[:, :, 0], None, high, thr_c, 0)
    same_bytes(p.squelch(), want, "new thresholds and a smaller hang")
    assert want[0].any()                                               # a channel that was open stayed open through a middle or low block
    # switching it off and on again starts closed; a device call elsewhere in the stream starts closed
    p.set_squelch(None)
    assert p.squelch_setting() is None and p.squelch_device() is None
    p.set_squelch(thr_o, thr_c, 100)
    p.work(x[5 * H:7 * H])
    same_bytes(p.squelch(), S.squelch(power[5:7], None, thr_o, thr_c, 100)[0], "switched on again")
    ring = np.concatenate([np.zeros(N // 2, np.complex64), x])
    with DeviceBuffers() as dev:
        d_in, d_o = dev.put(ring), dev.put(np.zeros(p.output_samples(NB), np.complex64))
        model = S.Stream(4)
        for first, n in ((0, 3), (3, 3), (5, 4), (5, 4)):
            p.process_device(C.c_void_p(d_in.value + 8 * first * H), first, n, d_o)
            p.synchronize()
            want = model.call(first, p.levels(n)[:, :, 0], None, thr_o, thr_c, 100)
            same_bytes(p.squelch(n), want, "process_device at %d" % first)
    # a plan without channels accepts it
    z = G.Pipeline(N, 2, [], max_blocks=3, keep_spectrum=True)
    z.set_levels(True)
    z.set_squelch(1.0, 0.5, 2)
    z.work(x[:3 * H])
    assert z.squelch().shape == (3, 0) and z.squelch_setting()[2] == 2 and "squelch" not in z.describe()
    z.set_squelch(None)
    z.set_levels(False)


def test_refused_while_a_pipelined_sinks_batch_is_inside():
    """a batch of the pipelined sinks entry inside the handle: set_squelch is refused with the sinks message (in front of the levels check: the levels are
    off here, as that entry demands), the switch-off call too, and the setting stays off; behind the flush loop both settings are accepted"""
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x, _power, thr_o, thr_c = stream(0)
    lib = _lib.lib()
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, lookahead=True, max_blocks=nb, **SINKS_KW)
    p.work(x[:nb * H], sinks=bank)
    with pytest.raises(G.FdcError) as e:
        p.set_squelch(thr_o, thr_c, 1)
    assert e.value.status == -1 and "sinks" in str(e.value) and "levels" not in str(e.value)
    assert p.squelch_setting() is None and p.squelch_device() is None
    assert lib.fdc_pipeline_set_squelch(p._h, None, None, 4, 0) == -1 and "sinks" in lib.fdc_last_error().decode()
    while p.flush_sinks(bank) > 0:
        pass
    p.set_levels(True)
    p.set_squelch(thr_o, thr_c, 1)                                     # nothing inside any more
    assert p.squelch_setting()[2] == 1 and p.squelch_device() is not None
    p.reset()
    p.work(x[:nb * H])
    same_bytes(p.squelch(), S.squelch(p.levels()[:, :, 0], None, thr_o, thr_c, 1)[0], "behind the flush")


# ---- footprint ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (0, 2), ids=[plan_ids[0], plan_ids[2]])
def test_footprint(k):
    """the decision: d_mask, d_state_in and d_state_out as three payloads between poisoned guards: exactly nblocks C bytes and C int32 pairs change.
    The gated audio pass: its output and its new history between guards, over the mask the handle holds: the ungated pass's bytes, gated"""
    _name, N, chans, flags = PLANS[k]
    H = N - N // 2
    x, power, thr_o, thr_c = stream(k)
    Cn, D, K = len(chans), 8, 64
    taps = G.lowpass_taps(D, K)
    on = squelched(N, chans, thr_o, thr_c, 1, flags=flags)
    un = G.Pipeline(N, 2, chans, max_blocks=NB, flags=flags)
    un.set_levels(True)
    for h in (un, on):
        h.set_demod("fm", CYCLES)
    ports = un.work(x)                                               # the demodulated ports, per channel
    for h in (un, on):
        h.set_audio(D, taps)
    un.reset()
    un.work(x)
    on.work(x)
    whole = on.squelch()
    state_in = np.array([(c % 2, c % 3) for c in range(Cn)], np.int32)
    lev = on.levels()
    want, wstate = S.squelch(lev[:, :, 0], None, thr_o, thr_c, 1, state_in)
    flat = np.zeros(on.output_samples(NB), np.float32)
    for c, w in enumerate(ports):
        flat[on.channel_offset(c, NB):on.channel_offset(c, NB) + NB * on.lout[c]] = w
    row = sum(on.lout) // D
    with DeviceBuffers() as dev:
        d_lev = dev.put(lev)
        band = DeviceBanded(dev, [NB * Cn, 8 * Cn, 8 * Cn], Cn)
        for poison in twice(band):
            assert dev.hip.hipMemcpy(band.ptr(1), C.c_void_p(state_in.ctypes.data), C.c_size_t(state_in.nbytes), 1) == 0
            on.squelch_pass_device(d_lev, band.ptr(0), NB, band.ptr(1), band.ptr(2))
            on.synchronize()
            band.check([want, state_in, wstate], "the decision")
        same_bytes(dev.get(d_lev, lev.size, np.float32).reshape(lev.shape), lev, "the levels")
        d_in = dev.put(flat)
        aud = DeviceBanded(dev, [4 * NB * row, 4 * Cn * (K - 1)], 4 * row)
        hist = np.concatenate([w[-(K - 1):] for w in ports]).astype(np.float32)
        for poison in twice(aud):
            on.audio_pass_device(d_in, aud.ptr(0), NB, None, aud.ptr(1))
            on.synchronize()
            aud.check([gate(un.audio(), whole, on.lout, D), hist], "the gated audio pass")
        assert _lib.lib().fdc_pipeline_audio_pass_device(on._h, d_in, aud.ptr(0), None, aud.ptr(1), NB - 1, None) == -1     # not the mask's block count


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
taps = G.lowpass_taps(8, 64)
p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pw = G.Pipeline(8192, 2, MIXED, max_blocks=nb, host_sub_blocks=3)
pd = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
for h in (p, pw, pd):
    h.set_levels(True)
    h.set_squelch(300.0, 100.0, 2)
p.set_demod("fm", 0.5)
p.set_audio(8, taps)
d_ring, d_out, d_lev, d_mask, d_s0, d_s1 = (C.c_void_p() for _ in range(6))
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(8 * pd.output_samples(nb))) == 0
assert hip.hipMalloc(C.byref(d_lev), C.c_size_t(8 * 4 * nb)) == 0 and hip.hipMemset(d_lev, 0, C.c_size_t(8 * 4 * nb)) == 0
assert hip.hipMalloc(C.byref(d_mask), C.c_size_t(4 * nb)) == 0
assert hip.hipMalloc(C.byref(d_s0), C.c_size_t(32)) == 0 and hip.hipMalloc(C.byref(d_s1), C.c_size_t(32)) == 0 and hip.hipMemset(d_s0, 0, C.c_size_t(32)) == 0
blk = [0]

def device():
    pd.process_device(d_ring, blk[0], nb, d_out)          # a stream that goes on: the state is used and swapped
    blk[0] += nb
    pd.synchronize()
    pd.squelch(nb)

def the_pass():
    pd.squelch_pass_device(d_lev, d_mask, nb, d_s0, d_s1)
    pd.synchronize()

entries = {"fdc_pipeline_work (path 5, gated audio)": lambda: (p.work(x), p.squelch()),
           "fdc_pipeline_work (spectrum path, sub-batches, the mask alone)": lambda: (pw.work(x2), pw.squelch()),
           "fdc_pipeline_process_device and fdc_pipeline_squelch": device,
           "fdc_pipeline_squelch_pass_device": the_pass,
           "new thresholds and a new hang before every call": lambda: (p.set_squelch(200.0, 50.0, 5), p.work(x), p.set_squelch(300.0, 100.0, 2), p.work(x)),
           "fdc_pipeline_set_squelch off and on again": lambda: (pw.set_squelch(None), pw.set_squelch(300.0, 100.0, 2), pw.work(x2))}
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
assert "squelch: pass" in p.describe() and "gated" in p.describe() and "squelch: pass" in pw.describe() and "squelch: pass" in pd.describe(), (p.describe(), pw.describe())
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
    ref = G.FrequencyDomainChannelizer(inptype=8, levels=True, **KW)
    chans = [(f, l, p, s) for (f, l, _lo, p, s) in ref.channel_params]
    x = keyed(N, R, chans, nb=2 * nb, seed=21)
    ref.work(x[:nb * H])
    la = ref.levels
    ref.work(x[nb * H:])
    lev = np.concatenate([la, ref.levels])[:, :, 0]
    lout = np.array(ref.pipeline.lout, np.float64)
    top_db = 10.0 * np.log10(lev.max(axis=0) / lout)                 # dB of mean power of each channel's strongest block
    on = G.FrequencyDomainChannelizer(inptype=8, levels=True, squelch_db=top_db - 5.0, squelch_close_db=top_db - 15.0, squelch_hang=1, **KW)
    thr_o, thr_c = G.squelch_thresholds(on.pipeline.lout, top_db - 5.0, top_db - 15.0)
    st = on.pipeline.squelch_setting()
    assert st[0].tobytes() == thr_o.tobytes() and st[1].tobytes() == thr_c.tobytes() and st[2] == 1
    model = S.Stream(len(chans))
    for j in range(2):
        on.work(x[j * nb * H:(j + 1) * nb * H])
        want = model.call(j * nb, on.levels[:, :, 0], None, thr_o, thr_c, 1)
        same_bytes(on.squelch, want, "hier block, call %d" % j)
    whole, _s = S.squelch(lev, None, thr_o, thr_c, 1)
    shows_everything(whole, lev, thr_o, thr_c, "hier block")
    on.work(x[:0])
    assert on.squelch.shape == (0, 3) and on.squelch.dtype == np.uint8
    # set_squelch: a new level and hang from the next call on, which channels are open is kept; None switches it off
    on.set_squelch(top_db + 30.0, top_db - 15.0, 0)
    assert on.pipeline.squelch_setting()[2] == 0
    on.set_squelch(None)
    assert on.pipeline.squelch_setting() is None
    # with the audio: closed blocks are zero, open ones the block's audio without a squelch
    taps = G.lowpass_taps(D, 33)
    kw = dict(KW, levels=True, demod="fm", demod_gain=CYCLES, audio_decim=D, audio_taps=taps)
    un = G.FrequencyDomainChannelizer(inptype=8, **kw)
    gated = G.FrequencyDomainChannelizer(inptype=8, squelch_db=top_db - 5.0, squelch_close_db=top_db - 15.0, squelch_hang=1, **kw)
    a, b = un.work(x[:nb * H]), gated.work(x[:nb * H])
    same_bytes(gated.squelch, whole[:nb], "hier block with the audio: the mask")
    for c, lo in enumerate(gated.pipeline.lout):
        keep = np.repeat(gated.squelch[:, c] != 0, lo // D)
        same_bytes(b[c], np.where(keep, a[c], np.float32(0)).astype(np.float32), "hier block with the audio, ch%d" % c)
