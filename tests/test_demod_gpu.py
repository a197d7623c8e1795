"""GPU tests (-m gpu) of the channel demodulation (fdc_pipeline_set_demod, fdc_pipeline_demod; include/fdc_amd.h): the setting's semantics, the
refusals, FM against its bound and MAG in bits, every cut of a stream and every host route, the device entries and the carry, the footprint, the other
settings, rows that are not finite, no allocation in the steady state, and the hier block.  tests/test_demod_routes_gpu.py covers every plan and the
inside of the kernel.

The reference of every comparison is y, the complex float32 outputs of THE SAME handle with the setting off (tests/demod_model.py): every FM sample
within |gain| (5 + 13 |theta64|) 2^-24 of gain theta64 modulo 2 pi |gain| (or +0.0 in bits where the float32 product is zero), every MAG sample
bit-equal to numpy's float32 statement.  FM outputs of two device runs over the same stream are compared in bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
import demod_model as M
from footprint import DeviceBanded, DeviceRing, POISONS, twice
from test_fine_tuning_gpu import BANK, MIXED, signal
from test_fine_tuning_routes_gpu import ALIAS_N, TINY, DeviceBuffers, alias_plan, by_channel, edge_nus
from test_iq_input_gpu import EXAMPLE, iq, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLES = float(np.float32(1.0 / (2.0 * np.pi)))            # the gain that gives cycles per output sample
MODES = (("fm", CYCLES), ("mag", 0.75))
PLANS = [("example, N = 4096", 4096, EXAMPLE), ("bank of 64, N = 16384", 16384, BANK)]
plan_ids = [f[0] for f in PLANS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def demod_hold(ref, got, mode, gain, what, fronts=None):
    """one call: got = its float32 outputs, ref = the complex64 outputs of the same call with the setting off, fronts = the sample in front of each
    channel's first (None: a stream start).  Returns the largest FM error in units of the bound."""
    assert len(ref) == len(got), what
    worst = 0.0
    for c, (y, d) in enumerate(zip(ref, got)):
        assert d.dtype == np.float32 and d.shape == (y.size,), (what, c, d.dtype, d.shape)
        assert np.abs(y).max() > 0, what
        if mode == "fm":
            worst = max(worst, M.fm_check(d, y, 0 if fronts is None else fronts[c], gain, "%s, ch%d" % (what, c)))
        else:
            same_bytes(d, M.mag32(y, gain), "%s, ch%d: MAG against numpy's float32 statement" % (what, c))
    return worst


def off_and_on(p, call, mode, gain):
    """call() from block 0 of handle p with the setting off and on: (y, d, describe() behind the demodulating call)"""
    p.set_demod(None)
    p.reset()
    ref = call()
    p.set_demod(mode, gain)
    p.reset()
    got = call()
    return ref, got, p.describe()


def checked(p, call, mode, gain, what):
    ref, got, d = off_and_on(p, call, mode, gain)
    demod_hold(ref, got, mode, gain, what)
    assert ("demod: %s" % mode) in d, d
    return ref, got


# ---- the setting ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_setting_semantics(k):
    _name, N, chans = PLANS[k]
    R, nb = 2, 3
    H = N - N // R
    x = signal(3 * nb * H, 6)
    q = G.Pipeline(N, R, chans, max_blocks=nb)
    plain = [q.work(x[j * nb * H:(j + 1) * nb * H]) for j in range(3)]
    d_plain = q.describe()
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    # off by default
    assert p.demod() == (None, 1.0) and "demod" not in p.describe()
    a0 = p.work(x[:nb * H])
    assert a0[0].dtype == np.complex64
    p.set_demod("fm", CYCLES)
    assert p.demod() == ("fm", CYCLES)
    a1 = p.work(x[nb * H:2 * nb * H])
    # (the first demodulating call starts the stream anew: nothing stands in front of its first sample)
    demod_hold(plain[1], a1, "fm", CYCLES, "second call, FM")
    assert "demod: fm" in p.describe()
    # it does not touch the stream; off again restores the bytes and the describe string
    p.set_demod(None)
    assert p.demod() == (None, 1.0)
    a2 = p.work(x[2 * nb * H:])
    for c in range(len(chans)):
        same_bytes(a0[c], plain[0][c], "call 0 ch%d against a handle that never demodulated" % c)
        same_bytes(a2[c], plain[2][c], "call 2 ch%d" % c)
    assert p.describe() == d_plain, (p.describe(), d_plain)
    # the setting survives reset(), the carry does not: the first call behind it is the first call of a stream, in bits
    p.set_demod("fm", 2.0)
    p.reset()
    f0 = p.work(x[:nb * H])
    f1 = p.work(x[nb * H:2 * nb * H])
    demod_hold(plain[1], f1, "fm", 2.0, "a continuing call", fronts=[y[-1] for y in plain[0]])
    p.reset()
    assert p.demod() == ("fm", 2.0) and "demod" not in p.describe()
    g0 = p.work(x[:nb * H])
    for c in range(len(chans)):
        same_bytes(g0[c], f0[c], "after reset(), ch%d" % c)
        assert bits(g0[c][:1]).tolist() == [0]
    # MAG in the middle of the stream; a change of mode starts FM's stream anew; a change of gain alone keeps the carry
    p.set_demod("mag", -3.0)
    m = p.work(x[nb * H:2 * nb * H])
    demod_hold(plain[1], m, "mag", -3.0, "MAG")
    assert "demod: mag" in p.describe()
    p.set_demod("fm", 2.0)
    h = p.work(x[2 * nb * H:])
    demod_hold(plain[2], h, "fm", 2.0, "FM behind MAG: anew")
    p.reset()
    p.work(x[:nb * H])
    p.set_demod("fm", 0.5)
    h1 = p.work(x[nb * H:2 * nb * H])
    assert p.demod() == ("fm", 0.5)
    demod_hold(plain[1], h1, "fm", 0.5, "a new gain keeps the carry", fronts=[y[-1] for y in plain[0]])
    assert any(h1[c][0] != 0 for c in range(len(chans)))


def test_refusals():
    N, R, nb = 4096, 2, 2
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    lib = _lib.lib()
    p.set_demod("mag", 2.0)
    for mode, gain in ((3, 1.0), (-1, 1.0), (1, 0.0), (2, -0.0), (1, float("nan")), (2, float("inf")), (1, -float("inf"))):
        assert lib.fdc_pipeline_set_demod(p._h, mode, gain) == -1, (mode, gain)
        assert p.demod() == ("mag", 2.0)                                   # the previous setting stays in force
    assert lib.fdc_pipeline_set_demod(p._h, 0, 0.0) == 0 and p.demod() == (None, 1.0)      # the gain is ignored with OFF
    assert lib.fdc_pipeline_set_demod(None, 1, 1.0) == -1 and lib.fdc_pipeline_demod(None, None, None) == -1
    assert lib.fdc_pipeline_demod(p._h, None, None) == 0
    # exclusive with integer output, in both directions; the public format enum is not extended
    p.set_output_format("sc16", 100.0)
    with pytest.raises(G.FdcError) as e:
        p.set_demod("fm")
    assert e.value.status == -1 and "FDC_OQ_FC32" in str(e.value) and p.demod() == (None, 1.0)
    assert lib.fdc_pipeline_set_demod(p._h, 0, 1.0) == 0                   # OFF is always accepted
    p.set_output_format(None)
    p.set_demod("fm")
    for fmt in ("sc16", "sc8"):
        with pytest.raises(G.FdcError) as e:
            p.set_output_format(fmt, 100.0)
        assert e.value.status == -1 and "demodulation" in str(e.value)
    assert p.output_format() == ("fc32", 1.0) and p.demod() == ("fm", 1.0)
    assert lib.fdc_pipeline_set_output_format(p._h, 3, 1.0) == -1
    p.set_output_format(None)                                              # FC32 is accepted while it is on
    out = p.work(signal(nb * (N - N // R), 1))
    assert out[0].dtype == np.float32


def test_no_channels():
    """C = 0: on is accepted, and a call has nothing to demodulate"""
    N, R, nb = 4096, 2, 3
    H = N - N // R
    p = G.Pipeline(N, R, [], max_blocks=nb, keep_spectrum=True)
    p.set_demod("fm")
    outs, spec = p.work(signal(nb * H, 1), want_spectrum=True)
    assert outs == [] and np.abs(spec).max() > 0 and p.demod() == ("fm", 1.0) and "demod" not in p.describe()


SINKS_KW = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01)


def test_refused_while_a_pipelined_sinks_batch_is_inside():
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x = signal(nb * H, 7)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, lookahead=True, max_blocks=nb, **SINKS_KW)
    p.work(x, sinks=bank)
    with pytest.raises(G.FdcError) as e:
        p.set_demod("fm")
    assert e.value.status == -1 and p.demod() == (None, 1.0)
    while p.flush_sinks(bank) > 0:
        pass
    p.set_demod("fm")                                                      # nothing inside any more
    assert p.demod() == ("fm", 1.0)


def test_entries_that_write_complex_float_are_refused():
    """work_sinks, work_spectrum, process_device_power and work_waterfall return FDC_ERR_INVALID_ARGUMENT and leave history, block counter and carry
    untouched: the next work continues the stream bit for bit"""
    N, R, nb = 4096, 2, 3
    H, ovl = N - N // R, N // R
    x = signal(2 * nb * H, 7)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    q = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, max_blocks=nb, **SINKS_KW)
    w = G.Waterfall(N, 1e6, R, 1, 0, -100.0, 0.0, 0, 0, max_items=nb)
    spec_items = np.zeros(nb * N, np.complex64)
    with DeviceBuffers() as dev:
        d_ring, d_out = dev.put(np.zeros(ovl + nb * H, np.complex64)), dev.put(np.zeros(p.output_samples(nb), np.complex64))
        d_spec, d_pow = dev.put(np.zeros(nb * N, np.complex64)), dev.put(np.zeros(nb * N // 16, np.float32))
        entries = [("work(sinks=)", lambda: p.work(x[nb * H:], sinks=bank)),
                   ("work_spectrum", lambda: p.work_spectrum(spec_items)),
                   ("work_waterfall", lambda: p.work_waterfall(x[nb * H:], w)),
                   ("process_device(d_group_power=)", lambda: p.process_device(d_ring, 0, nb, d_out, d_spectrum=d_spec, d_group_power=d_pow))]
        for h in (p, q):
            h.set_demod("fm", CYCLES)
        a0, b0 = p.work(x[:nb * H]), q.work(x[:nb * H])
        for name, call in entries:
            with pytest.raises((G.FdcError, ValueError)) as e:
                call()
            assert "demodulation" in str(e.value), name
        assert p.flush_sinks(bank) == 0                                    # not refused: nothing inside, nothing to flush
        a1, b1 = p.work(x[nb * H:]), q.work(x[nb * H:])
        for c in range(len(EXAMPLE)):
            same_bytes(a0[c], b0[c], "before the refusals, ch%d" % c)
            same_bytes(a1[c], b1[c], "after the refusals, ch%d" % c)
        assert any(a1[c][0] != 0 for c in range(len(EXAMPLE)))
        p.set_demod(None)
        for name, call in entries:
            call()                                            # they work again
        p.synchronize()


def test_the_group_entries_refuse_a_demodulating_member():
    N, R, nb = 4096, 2, 8
    H = N - N // R
    x = signal(nb * H, 8)
    g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    lib = _lib.lib()
    member = lib.fdc_pipeline_group_member(g._h, 1)
    assert lib.fdc_pipeline_set_demod(member, 1, 1.0) == 0
    for call in (lambda: g.work(x), lambda: g.work_real(x.real.copy()), lambda: g.work_iq(iq(nb * H, np.int16, 3))):
        with pytest.raises(G.FdcError) as e:
            call()
        assert e.value.status == -1 and "demodulation" in str(e.value)
    assert lib.fdc_pipeline_set_demod(member, 0, 1.0) == 0
    for c, (u, v) in enumerate(zip(g.work(x), p.work(x))):                 # nothing of the refused calls is left in the group
        same_bytes(u, v, "the group after the refusals, ch%d" % c)


# ---- FM against the bound, MAG in bits ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,gain", MODES + (("fm", -1000.0), ("mag", float(np.float32(1e-3)))), ids=["fm", "mag", "fm, gain -1000", "mag, gain 1e-3"])
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_every_sample_against_the_model(k, mode, gain):
    _name, N, chans = PLANS[k]
    R, nb = 2, 5
    H = N - N // R
    x = signal(nb * H, 20 + k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    checked(p, lambda: p.work(x), mode, gain, "%s, gain %g" % (mode, gain))


# ---- cuts and host routes -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,gain", MODES, ids=["fm", "mag"])
@pytest.mark.parametrize("N,R,chans,flags", [(4096, 2, EXAMPLE, 0), (16384, 2, BANK, 0), (8192, 2, MIXED, 0), (4096, 2, EXAMPLE, G.FDC_PIPE_NO_FUSED)],
                         ids=["path 5", "bank", "mixed", "example plan, spectrum path"])
def test_cuts_of_the_stream_give_the_same_bits(N, R, chans, flags, mode, gain):
    """7 blocks as 7, as 3 + 4 and as 1 + 1 + 5; with host_sub_blocks = 2 (four enqueue-path calls linked by the carry) and chunk_blocks = 2 (launch
    groups inside one enqueue call: one pass over the whole call)"""
    nb = 7
    H = N - N // R
    x = signal(nb * H, 2)
    one = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    _ref, whole = checked(one, lambda: one.work(x), mode, gain, "7 blocks")
    for cut in ((3, 4), (1, 1, 5)):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
        p.set_demod(mode, gain)
        parts, b0 = [], 0
        for n in cut:
            parts.append(p.work(x[b0 * H:(b0 + n) * H]))
            b0 += n
        for c in range(len(chans)):
            same_bytes(np.concatenate([q[c] for q in parts]), whole[c], "cut %r, ch%d" % (cut, c))
    for kw in (dict(host_sub_blocks=2), dict(chunk_blocks=2), dict(chunk_blocks=2, host_sub_blocks=3)):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags, **kw)
        assert "chunk_blocks" not in kw or p.chunk_blocks() == 2
        p.set_demod(mode, gain)
        for c, (u, v) in enumerate(zip(p.work(x), whole)):
            same_bytes(u, v, "%r, ch%d" % (kw, c))


@pytest.mark.parametrize("mode,gain", MODES, ids=["fm", "mag"])
@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("sub", [0, 2], ids=["one sub-batch", "sub-batches of 2"])
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_sub_batches_registered_outputs_and_ragged_calls(k, sub, registered, mode, gain):
    """calls of 1, 7, 3 and 5 blocks (host sub-batches; staged outputs, or registered ones through the copy form of k_scatter_oq): the bits of one call
    of 16 blocks on a second handle, which holds the model"""
    _name, N, chans = PLANS[k]
    R, mb, sizes = 2, 7, (1, 7, 3, 5)
    H = N - N // R
    x = signal(sum(sizes) * H, 300 + k)
    one = G.Pipeline(N, R, chans, max_blocks=sum(sizes))
    _ref, whole = checked(one, lambda: one.work(x), mode, gain, "one call of 16 blocks")
    p = G.Pipeline(N, R, chans, max_blocks=mb, host_sub_blocks=sub or None)
    p.set_demod(mode, gain)
    bufs = [np.zeros(mb * lo, np.float32) for lo in p.lout]
    if registered:
        for b in bufs:
            G.register_host(b)
    try:
        pieces, b0 = [[] for _ in chans], 0
        for n in sizes:
            outs = [b[:n * lo] for b, lo in zip(bufs, p.lout)]
            p.work(x[b0 * H:(b0 + n) * H], outs=outs)
            for c, o in enumerate(outs):
                pieces[c].append(o.copy())
            b0 += n
    finally:
        if registered:
            for b in bufs:
                G.unregister_host(b)
    for c in range(len(chans)):
        same_bytes(np.concatenate(pieces[c]), whole[c], "ragged stream ch%d" % c)
    assert ("demod: %s" % mode) in p.describe() and "; output " not in p.describe(), p.describe()


@pytest.mark.parametrize("mode,gain", MODES, ids=["fm", "mag"])
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_outputs_that_are_not_wanted(k, mode, gain):
    """outs[c] = NULL for some channels of ragged calls: the others are complete, and the carry of a channel nobody reads is still kept"""
    _name, N, chans = PLANS[k]
    R, nb = 2, 6
    H = N - N // R
    x = signal(nb * H, 310 + k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    _ref, full = checked(p, lambda: p.work(x), mode, gain, "every output")
    p.reset()
    lib = _lib.lib()
    outs = [np.zeros(nb * lo, np.float32) for lo in p.lout]
    b0 = 0
    for j, n in enumerate((1, 3, 2)):
        keep = [(c + j) % 2 == 0 for c in range(len(chans))]
        ptrs = (C.c_void_p * len(outs))(*[o[b0 * lo:].ctypes.data if kp else None for o, lo, kp in zip(outs, p.lout, keep)])
        assert lib.fdc_pipeline_work(p._h, x[b0 * H:].ctypes.data, n, ptrs, None) == n
        for c, (lo, kp) in enumerate(zip(p.lout, keep)):
            want = full[c][b0 * lo:(b0 + n) * lo] if kp else np.zeros(n * lo, np.float32)
            same_bytes(outs[c][b0 * lo:(b0 + n) * lo], want, "call %d ch%d" % (j, c))
        b0 += n


@pytest.mark.parametrize("mode,gain", MODES, ids=["fm", "mag"])
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_real_and_integer_input(k, mode, gain):
    _name, N, chans = PLANS[k]
    R, nb = 2, 5
    H = N - N // R
    xr = signal(nb * H, 320 + k).real.copy()
    xi = iq(nb * H, np.int16, 33)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    _r, a = checked(p, lambda: p.work_real(xr), mode, gain, "work_real")
    # work_real in two calls: the carry links them
    p.reset()
    parts = [p.work_real(xr[:2 * H]), p.work_real(xr[2 * H:])]
    for c in range(len(chans)):
        same_bytes(np.concatenate([q[c] for q in parts]), a[c], "work_real as 2 + 3, ch%d" % c)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    checked(p, lambda: p.work_iq(xi, scale=2.0 ** -12), mode, gain, "work_iq")


# ---- device entries -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_device_entries_and_the_carry(k):
    """process_device over a ring of 7 blocks.  0..3 then 3..7: the second call continues the stream and uses the carry, bit-equal to one call.  A call
    elsewhere (4..7 behind 0..3; 3..7 first of all) starts anew: its first sample is +0.0 and the rest is the one call's.  A call on the caller's stream.
    Above max_blocks a call is refused while the setting is on and nothing is enqueued."""
    _name, N, chans = PLANS[k]
    R, nb = 2, 7
    H, ovl = N - N // R, N // R
    x = signal(nb * H, 340 + k)
    ring = np.concatenate([np.zeros(ovl, np.complex64), x])
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    y = p.work(x)
    p.reset()
    with DeviceBuffers() as dev:
        st = C.c_void_p()
        assert dev.hip.hipStreamCreate(C.byref(st)) == 0
        try:
            def run(first, n, stream=None):
                d_in = dev.put(np.ascontiguousarray(ring[first * H:first * H + ovl + n * H]))
                d_o = dev.put(np.zeros(p.output_samples(n), np.float32))
                p.process_device(d_in, first, n, d_o, stream=stream)
                if stream is not None:
                    assert dev.hip.hipStreamSynchronize(stream) == 0
                p.synchronize()
                return by_channel(p, dev.get(d_o, p.output_samples(n), np.float32), n)

            for mode, gain in MODES:
                fm = mode == "fm"
                p.set_demod(None)
                p.set_demod(mode, gain)
                whole = run(0, nb)
                demod_hold(y, whole, mode, gain, "process_device, 7 blocks, %s" % mode)
                assert ("demod: %s" % mode) in p.describe()
                p.set_demod(None)
                p.set_demod(mode, gain)                                    # (off and on: the stream starts anew)
                a, b = run(0, 3), run(3, 4, stream=st)
                for c, lo in enumerate(p.lout):
                    same_bytes(np.concatenate([a[c], b[c]]), whole[c], "0..3 and 3..7 against one call, %s ch%d" % (mode, c))
                e = run(4, 3)                                              # behind 3..7 the stream goes on at block 7, not at 4
                for c, lo in enumerate(p.lout):
                    if fm:
                        assert bits(e[c][:1]).tolist() == [0], c
                        same_bytes(e[c][1:], whole[c][4 * lo + 1:], "a call elsewhere, ch%d" % c)
                        assert whole[c][4 * lo] != 0
                    else:
                        same_bytes(e[c], whole[c][4 * lo:], "a call elsewhere, MAG ch%d" % c)
                f = run(7 - 3, 3)                                          # ... and nor does the same call again continue itself
                for c in range(len(chans)):
                    same_bytes(f[c], e[c], "the same call again, %s ch%d" % (mode, c))
            # above max_blocks: refused with the setting on (nothing is enqueued: the output stays as it is), served without
            big = dev.put(np.zeros(ovl + 2 * nb * H, np.complex64))
            d_big = dev.put(np.full(p.output_samples(2 * nb), 7, np.complex64))
            p.set_demod("mag", 1.0)
            with pytest.raises(G.FdcError) as err:
                p.process_device(big, 0, 2 * nb, d_big)
            assert err.value.status == -1
            p.synchronize()
            assert (dev.get(d_big, p.output_samples(2 * nb), np.complex64) == 7).all()
            p.set_demod(None)
            p.process_device(big, 0, 2 * nb, d_big)
            p.synchronize()
        finally:
            dev.hip.hipStreamDestroy(st)


@pytest.mark.parametrize("mode,gain", MODES, ids=["fm", "mag"])
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_footprint_of_the_device_entry(k, mode, gain):
    """process_device into a d_out between guards, from a ring inside NaN, on a handle of 8 blocks serving calls of 1 and 5: exactly 4 * nblocks * sum
    lout bytes, the real samples at element offset nblocks * out_off_c, and no guard byte changes (both poison bytes)"""
    _name, N, chans = PLANS[k]
    R, mb = 2, 8
    H, ovl = N - N // R, N // R
    x = signal(mb * H, 12)
    p = G.Pipeline(N, R, chans, max_blocks=mb)
    q = G.Pipeline(N, R, chans, max_blocks=mb)
    p.set_demod(mode, gain)
    q.set_demod(mode, gain)
    for nb in (1, 5):
        ring = np.concatenate([np.zeros(ovl, np.complex64), x[:nb * H]])
        q.reset()
        want = q.work(x[:nb * H])
        n_out = p.output_samples(nb)
        assert n_out == nb * sum(p.lout)
        flat, seen = np.zeros(n_out * 4, np.uint8), np.zeros(n_out, bool)
        for c, w in enumerate(want):
            a, cnt = p.channel_offset(c, nb), nb * p.lout[c]
            assert not seen[a:a + cnt].any()
            seen[a:a + cnt] = True
            flat[a * 4:(a + cnt) * 4] = np.ascontiguousarray(w).view(np.uint8)
        assert seen.all()
        with DeviceBuffers() as dev:
            band = DeviceBanded(dev, [n_out * 4], sum(p.lout) * 4)
            d_ring = DeviceRing(dev, ring, H)
            for _poison in twice(band):
                p.set_demod(None)
                p.set_demod(mode, gain)                                    # (every call the first of a stream, as q's)
                p.process_device(d_ring.ptr, 0, nb, band.ptr())
                p.synchronize()
                band.check(flat, "%d blocks" % nb)
                d_ring.unchanged("%d blocks" % nb)
    assert POISONS[0] != POISONS[1]


CARRY_PLANS = [("example, N = 4096", 4096, 2, lambda: EXAMPLE), ("ragged runs, N = 8192", 8192, 4, lambda: TINY),
               ("aliased channels, N = 16384", ALIAS_N, 2, lambda: alias_plan(ALIAS_N))]


@pytest.mark.parametrize("k", range(len(CARRY_PLANS)), ids=[f[0] for f in CARRY_PLANS])
def test_footprint_of_the_pass_and_the_carry_buffers(k):
    """fdc_pipeline_demod_device, the kernel's launcher on buffers of the caller: the real output, the carry it reads and the carry it writes lie as
    three payloads between guards.  The input is the second of two calls of a stream (5 and 3 blocks; 1 and 4), the carry in front of it the last
    complex sample of every channel of the first.  FM: the output is, in bits, what a demodulating handle gives for that second call; of the carry
    buffers exactly C float2 change, entry c is the last sample of channel c's run (a copied channel has its own entry), the carry that is read
    stays as it was, and no guard byte moves.  MAG: numpy's bits, and neither carry buffer is touched.  Both poison bytes.  With no carry in front
    (NULL) the output is that of a stream start."""
    _name, N, R, plan = CARRY_PLANS[k]
    chans = plan()
    H = N - N // R
    g = CYCLES
    for n1, n2 in ((5, 3), (1, 4)):
        x = signal((n1 + n2) * H, 60 + k)
        p = G.Pipeline(N, R, chans, max_blocks=max(n1, n2))
        C_ = len(p.lout)
        y1, y2 = p.work(x[:n1 * H]), p.work(x[n1 * H:])
        p.set_demod("fm", g)
        p.reset()
        p.work(x[:n1 * H])
        want = p.work(x[n1 * H:])
        p.reset()
        p.work(x[:n1 * H])                  # (the handle now stands behind the first call, its own carry in place)
        n_out = p.output_samples(n2)

        def flat(parts, dtype):
            out = np.zeros(n_out, dtype)
            for c, w in enumerate(parts):
                a = p.channel_offset(c, n2)
                out[a:a + n2 * p.lout[c]] = w
            return out

        carry_in = np.array([y[-1] for y in y1], np.complex64)
        carry_out = np.array([y[-1] for y in y2], np.complex64)
        with DeviceBuffers() as dev:
            d_in = dev.put(flat(y2, np.complex64))
            band = DeviceBanded(dev, [n_out * 4, C_ * 8, C_ * 8], sum(p.lout) * 4)
            for poison in twice(band):
                untouched = np.full(C_ * 8, poison, np.uint8)
                assert dev.hip.hipMemcpy(band.ptr(1), C.c_void_p(carry_in.ctypes.data), C.c_size_t(carry_in.nbytes), 1) == 0
                p.demod_device("fm", g, d_in, band.ptr(0), n2, d_carry_in=band.ptr(1), d_carry_out=band.ptr(2))
                p.synchronize()
                band.check([flat(want, np.float32), carry_in, carry_out], "FM behind a carry, %d blocks" % n2)
                band.fill(poison)
                p.demod_device("mag", 0.75, d_in, band.ptr(0), n2, d_carry_in=band.ptr(1), d_carry_out=band.ptr(2))
                p.synchronize()
                band.check([flat([M.mag32(y, 0.75) for y in y2], np.float32), untouched, untouched], "MAG, %d blocks" % n2)
                band.fill(poison)
                p.demod_device("fm", g, d_in, band.ptr(0), n2, d_carry_in=None, d_carry_out=band.ptr(2))
                p.synchronize()
                got = dev.get(band.ptr(0), n_out, np.float32)
                band.check([got, untouched, carry_out], "FM at a stream start, %d blocks" % n2)
                for c, w in enumerate(want):
                    a = p.channel_offset(c, n2)
                    assert bits(got[a:a + 1]).tolist() == [0], c
                    same_bytes(got[a + 1:a + n2 * p.lout[c]], w[1:], "FM at a stream start, ch%d" % c)
            same_bytes(dev.get(d_in, n_out, np.complex64), flat(y2, np.complex64), "the input")
        # the handle's own setting, carry and stream position were not touched: its stream goes on behind the first call, in bits
        assert p.demod() == ("fm", g)
        for c, (u, v) in enumerate(zip(p.work(x[n1 * H:]), want)):
            same_bytes(u, v, "the handle's own second call, ch%d" % c)
    lib = _lib.lib()
    assert lib.fdc_pipeline_demod_device(None, 1, 1.0, None, None, None, None, 1, None) == -1
    for bad in ((0, 1.0), (3, 1.0), (1, 0.0), (2, float("nan"))):
        assert lib.fdc_pipeline_demod_device(p._h, bad[0], bad[1], 1, 1, None, 1, 1, None) == -1, bad
    assert lib.fdc_pipeline_demod_device(p._h, 1, 1.0, 1, 1, None, None, 1, None) == -1          # FM without a carry to write
    assert lib.fdc_pipeline_demod_device(p._h, 1, 1.0, 1, 1, 2, 2, 1, None) == -1                # one buffer for both
    assert lib.fdc_pipeline_demod_device(p._h, 1, 1.0, None, None, None, None, 0, None) == 0 and lib.fdc_pipeline_demod_device(p._h, 1, 1.0, 1, 1, None, 1, -1, None) == -1


# ---- with the other settings: cut -> fine tuning -> gain -> levels, lag-1 -> demodulation -----------------------------------------------------------------

@pytest.mark.parametrize("N,chans", [(16384, BANK), (4096, EXAMPLE), (8192, MIXED)], ids=["bank", "path 5", "spectrum path"])
def test_fine_tuning_moves_the_fm_output(N, chans):
    """The samples are the turned ones (the model holds on them), and against fine tuning off the output moves by -2 pi nu gain.  The bound: a turned
    sample is within 11 2^-24 |y| of y exp(-2 pi i phi(t)) (DESIGN "Fine tuning", Error bound), so its argument within asin(11 2^-24), and the angle
    theta' of the exact product of two turned float32 samples within 22.1 2^-24 of theta - 2 pi nu' (nu' = inc / 2^64, within 2^-65 of nu).  d' and d
    are each within the FM bound of gain theta' and gain theta.  So, modulo 2 pi |gain|,
        |d' - d + 2 pi nu gain| <= |gain| (22.1 + (5 + 13 |theta'|) + (5 + 13 |theta|)) 2^-24
    for every sample but the first of the stream (+0.0 both times)."""
    R, nb = 2, 4
    H = N - N // R
    x = signal(nb * H, 400)
    nu = np.random.default_rng(3).uniform(-0.45, 0.45, len(chans))
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    y0, d0 = checked(p, lambda: p.work(x), "fm", CYCLES, "fine tuning off")
    p.set_fine_tuning(nu)
    y1, d1 = checked(p, lambda: p.work(x), "fm", CYCLES, "fine tuning on")
    assert "fine tuning: " in p.describe() and "demod: fm" in p.describe()
    p.set_fine_tuning(None)
    g = float(np.float32(CYCLES))
    for c in range(len(chans)):
        th0, th1 = M.theta64(y0[c]), M.theta64(y1[c])
        lim = abs(g) * (22.1 + (5 + 13 * np.abs(th1)) + (5 + 13 * np.abs(th0))) * 2.0 ** -24
        diff = d1[c].astype(np.float64) - d0[c].astype(np.float64) + 2 * np.pi * nu[c] * g
        period = 2 * np.pi * abs(g)
        diff = np.abs(diff - np.round(diff / period) * period)
        print("ch%d: the FM output moved by -2 pi nu gain within %.3g of its bound" % (c, (diff / lim)[1:].max()))
        assert (diff[1:] <= lim[1:]).all(), (c, (diff / lim)[1:].max())
        assert bits(d0[c][:1]).tolist() == [0] and bits(d1[c][:1]).tolist() == [0]


@pytest.mark.parametrize("N,chans", [(16384, BANK), (4096, EXAMPLE)], ids=["bank", "path 5"])
@pytest.mark.parametrize("e", [-3, 1, 5])
def test_under_a_power_of_two_gain(N, chans, e):
    """g = 2^e for every channel: every sample is scaled exactly, every product of FM by 4^e exactly, so the angle is the same in bits; MAG is scaled
    by 2^e exactly (no value near the ends of the exponent range: the input is of order 1)"""
    R, nb = 2, 4
    H = N - N // R
    x = signal(nb * H, 410)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    _y, fm0 = checked(p, lambda: p.work(x), "fm", CYCLES, "gains off")
    _y, mag0 = checked(p, lambda: p.work(x), "mag", 0.75, "gains off")
    p.set_gains(np.full(len(chans), 2.0 ** e, np.float32))
    _y, fm1 = checked(p, lambda: p.work(x), "fm", CYCLES, "g = 2^%d" % e)
    _y, mag1 = checked(p, lambda: p.work(x), "mag", 0.75, "g = 2^%d" % e)
    assert "gains: " in p.describe()
    for c in range(len(chans)):
        same_bytes(fm1[c], fm0[c], "FM under g = 2^%d, ch%d" % (e, c))
        same_bytes(mag1[c], mag0[c] * np.float32(2.0 ** e), "MAG under g = 2^%d, ch%d" % (e, c))


@pytest.mark.parametrize("mode,gain", MODES, ids=["fm", "mag"])
@pytest.mark.parametrize("N,chans", [(16384, BANK), (4096, EXAMPLE)], ids=["bank", "path 5"])
def test_levels_and_lag1_are_those_of_the_complex_samples(N, chans, mode, gain):
    """levels and lag-1 with fine tuning and gains off and on: bit-equal with the demodulation on and off, and the demodulated outputs are those
    without levels and lag-1"""
    R, nb = 2, 5
    H = N - N // R
    x = signal(nb * H, 420)
    g = np.random.default_rng(4).uniform(0.5, 2.0, len(chans)).astype(np.float32)
    nu = edge_nus(len(chans), 2)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    for fine, gn in ((False, False), (True, True)):
        what = "fine tuning %s, gains %s" % (fine, gn)
        p.set_fine_tuning(nu if fine else None)
        p.set_gains(g if gn else None)
        p.set_levels(False)
        p.set_lag1(False)
        _y, d = checked(p, lambda: p.work(x), mode, gain, what)
        p.set_levels(True)
        p.set_lag1(True)
        p.set_demod(None)
        p.reset()
        p.work(x)
        lev, s = p.levels(), p.lag1()
        p.set_demod(mode, gain)
        p.reset()
        d2 = p.work(x)
        same_bytes(p.levels(), lev, what + ": the levels")
        same_bytes(p.lag1(), s, what + ": the lag-1 correlation")
        for c in range(len(chans)):
            same_bytes(d2[c], d[c], what + ", ch%d" % c)
        desc = p.describe()
        assert "levels: " in desc and "lag1: pass" in desc and ("demod: %s" % mode) in desc, desc


# ---- rows that are not finite -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,gain", MODES, ids=["fm", "mag"])
def test_samples_that_are_not_finite_disturb_no_other_sample(mode, gain):
    """an input sample of NaN reaches the blocks that overlap it; every output sample whose own complex sample and (FM) the one in front are finite
    has the bits it has without the NaN, every other one is NaN"""
    N, R, nb = 8192, 2, 6
    H = N - N // R
    x = signal(nb * H, 9)
    p = G.Pipeline(N, R, MIXED, max_blocks=nb)
    bad = x.copy()
    bad[4 * H + 100] = complex(np.nan, 1.0)
    _y, clean = checked(p, lambda: p.work(x), mode, gain, "clean")
    yb, got = off_and_on(p, lambda: p.work(bad), mode, gain)[:2]
    for c in range(len(MIXED)):
        nf = ~np.isfinite(yb[c].view(np.float32).reshape(-1, 2)).all(axis=1)
        hit = nf | np.concatenate([[False], nf[:-1]]) if mode == "fm" else nf
        assert hit.any() and not hit.all()
        same_bytes(got[c][~hit], clean[c][~hit], "the samples away from the NaN, ch%d" % c)
        assert np.isnan(got[c][hit]).all(), c


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
p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pw = G.Pipeline(8192, 2, MIXED, max_blocks=nb, host_sub_blocks=3)
po = G.Pipeline(8192, 2, MIXED, max_blocks=nb)
pd = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
po.set_fine_tuning([0.1, -0.2])
po.set_gains([2.0, 0.5])
po.set_levels(True)
po.set_lag1(True)
p.set_demod("fm", 0.5)
pw.set_demod("mag", 2.0)
po.set_demod("fm", 1.0)
pd.set_demod("fm", 1.0)
d_ring, d_out = C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(4 * pd.output_samples(nb))) == 0
blk = [0]

def device():
    pd.process_device(d_ring, blk[0], nb, d_out)          # a stream that goes on: the carry is used and swapped
    blk[0] += nb
    pd.synchronize()

entries = {"fdc_pipeline_work (path 5, FM)": lambda: p.work(x),
           "fdc_pipeline_work (spectrum path, sub-batches, MAG)": lambda: pw.work(x2),
           "fdc_pipeline_work (fine tuning, gains, levels, lag-1, FM)": lambda: (po.work(x2), po.lag1(), po.levels()),
           "fdc_pipeline_process_device": device,
           "a new gain before every call": lambda: (p.set_demod("fm", 0.25), p.work(x)),
           "fdc_pipeline_set_demod off and on again": lambda: (pw.set_demod(None), pw.set_demod("fm", 1.0), pw.work(x2))}
bad = []
for name, call in entries.items():
    for _ in range(3):
        call()
    before = counts()
    for _ in range(50):
        call()
    after = counts()
    print(name, [a - b for a, b in zip(after, before)])
    if after != before:
        bad.append((name, [a - b for a, b in zip(after, before)]))
assert "demod: fm" in p.describe() and "demod: fm" in po.describe(), (p.describe(), po.describe())
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

KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05], [-0.2, 0.1], [0.31, 0.02]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False, max_blocks=6)


def test_hier_block():
    N, R, nb = 4096, 2, 6
    H = N - N // R
    x = signal(2 * nb * H, 11)
    off = G.FrequencyDomainChannelizer(inptype=8, **KW)
    ya, yb = off.work(x[:nb * H]), off.work(x[nb * H:])
    for mode, gain in MODES:
        on = G.FrequencyDomainChannelizer(inptype=8, demod=mode, demod_gain=gain, **KW)
        assert on.demod == mode and on.pipeline.demod() == (mode, float(np.float32(gain)))
        da, db = on.work(x[:nb * H]), on.work(x[nb * H:])
        demod_hold(ya, da, mode, gain, "hier block, first call")
        demod_hold(yb, db, mode, gain, "hier block, second call", fronts=[y[-1] for y in ya])
        assert [o.shape for o in on.work(x[:0])] == [(0,)] * 3
    # together with fine tuning, levels, gains and lag1: levels and lag1 are those of the block without demod
    kw = dict(KW, fine_tuning=True, levels=True, lag1=True, gains=[2.0, 0.5, -1.0])
    both = G.FrequencyDomainChannelizer(inptype=8, demod="fm", demod_gain=CYCLES, **kw)
    ref = G.FrequencyDomainChannelizer(inptype=8, **kw)
    d, y = both.work(x[:nb * H]), ref.work(x[:nb * H])
    demod_hold(y, d, "fm", CYCLES, "hier block with fine tuning, levels, gains and lag1")
    same_bytes(both.levels, ref.levels, "levels")
    same_bytes(both.lag1, ref.lag1, "lag1")
    # the Float input type and integer input
    fl = G.FrequencyDomainChannelizer(inptype=4, demod="mag", **KW)
    fr = G.FrequencyDomainChannelizer(inptype=4, **KW)
    demod_hold(fr.work(x[:nb * H].real.copy()), fl.work(x[:nb * H].real.copy()), "mag", 1.0, "hier block, Float input")
    xi = iq(nb * H, np.int16, 5)
    ii = G.FrequencyDomainChannelizer(inptype=8, iq_input="sc16", iq_scale=2.0 ** -12, demod="fm", **KW)
    ir = G.FrequencyDomainChannelizer(inptype=8, iq_input="sc16", iq_scale=2.0 ** -12, **KW)
    demod_hold(ir.work(xi), ii.work(xi), "fm", 1.0, "hier block, sc16 input")
