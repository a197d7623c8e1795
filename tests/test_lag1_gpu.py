"""GPU tests (-m gpu) of the channel lag-1 correlation (fdc_pipeline_set_lag1, fdc_pipeline_lag1, fdc_pipeline_lag1_device and the group's two entries;
include/fdc_amd.h): the setting's semantics, the refusals, the one-order rule, every call form, the order of the settings, no allocation in the steady
state, the hier block, and a closed loop on a tone.  tests/test_lag1_routes_gpu.py covers every plan and the inside of the kernel.

Every comparison is against the two models of tests/lag1_model.py applied to the float32 outputs of THE SAME call (lag-1 on does not change them, which
is asserted: byte-equal to the same handle's outputs with it off): both components of every (block, channel) row within (lout + 8) 2^-24 M of the float64
sum, M = sum |y[j]| |y[j - 1]| in float64, and bit-equal to the float32 model that follows the stated order."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from footprint import DeviceBanded, DeviceRing, POISONS, twice
from lag1_model import agrees, model64
from test_fine_tuning_gpu import BANK, FORCED, MIXED, narrowed, signal, work_span
from test_fine_tuning_routes_gpu import TINY, DeviceBuffers, by_channel, edge_nus, int_scale
from test_iq_input_gpu import EXAMPLE, iq, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lag1_hold(p, outs, s, what):
    """the models on every row of one call: outs = the float32 outputs the call returned (or would return before narrowing), s = its lag-1 correlation.
    Channels of one row length go through the models together.  Returns the largest error in units of the bound."""
    lout = list(p.lout)
    nb = outs[0].size // lout[0] if outs else 0
    assert s.shape == (nb, len(lout)) and s.dtype == np.complex64, (what, s.shape, s.dtype)
    worst = 0.0
    for lo in sorted(set(lout)):
        cs = [c for c in range(len(lout)) if lout[c] == lo]
        y = np.concatenate([np.ascontiguousarray(outs[c], np.complex64).reshape(-1) for c in cs])
        worst = max(worst, agrees(np.ascontiguousarray(s[:, cs].T).reshape(-1), y, lo, "%s, channels %d..%d" % (what, cs[0], cs[-1])))
    assert all(np.abs(y).max() > 0 for y in outs), what
    return worst


def on_and_off(p, call):
    """call() from block 0 of handle p with lag-1 on, its result and describe() behind it, and call() again with it off"""
    p.reset()
    p.set_lag1(True)
    got = call()
    s, d = p.lag1(), p.describe()
    p.set_lag1(False)
    p.reset()
    plain = call()
    assert "lag1: pass" in d and "lag1" not in p.describe(), (d, p.describe())
    return got, s, d, plain


def checked(p, call, what, ref=None):
    """on_and_off, the outputs byte-equal to lag-1 off, the models on the result (ref: the float samples, where the call returns narrow ones); returns
    (outputs, lag-1 correlation, describe)"""
    got, s, d, plain = on_and_off(p, call)
    for c, (u, v) in enumerate(zip(got, plain)):
        same_bytes(u, v, "%s: outputs with lag-1 on against off, ch%d" % (what, c))
    lag1_hold(p, got if ref is None else ref, s, what)
    return got, s, d


def raw_lag1(h, nblocks, nchan, fn=None):
    """the C entry's status and what it wrote (a buffer of NaN where it wrote nothing)"""
    out = np.full((max(nblocks, 0), nchan, 2), np.nan, np.float32)
    rc = (fn or _lib.lib().fdc_pipeline_lag1)(h, out.ctypes.data_as(C.POINTER(C.c_float)), nblocks)
    return rc, out


# ---- the setting ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,chans", [(4096, EXAMPLE), (8192, MIXED)], ids=["path 5", "spectrum path"])
def test_setting_semantics(N, chans):
    R, nb = 2, 3
    H = N - N // R
    x = signal(3 * nb * H, 6)
    q = G.Pipeline(N, R, chans, max_blocks=nb)
    plain = [q.work(x[k * nb * H:(k + 1) * nb * H]) for k in range(3)]
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    lib = _lib.lib()
    # off by default: no result, no device buffer, no text in describe; before any call and with a wrong count the accessor refuses
    assert p.lag1_device() is None and "lag1" not in p.describe()
    a0 = p.work(x[:nb * H])
    assert raw_lag1(p._h, nb, len(chans))[0] == -1                         # the setting is off
    p.set_lag1(True)
    assert p.lag1_device() is not None
    rc, out = raw_lag1(p._h, nb, len(chans))
    assert rc == -1 and np.isnan(out).all()                                # on, but no call yet
    a1 = p.work(x[nb * H:2 * nb * H])
    for bad in (nb - 1, nb + 1, 0, -1):
        rc, out = raw_lag1(p._h, bad, len(chans))
        assert rc == -1 and np.isnan(out).all(), bad
    s1 = p.lag1()
    lag1_hold(p, a1, s1, "second call")
    # a call of no blocks leaves the previous result in place
    assert p.work(x[:0]) is not None
    same_bytes(p.lag1(nb), s1, "after a call of no blocks")
    # it does not touch the stream: the third call continues it; the setting survives reset()
    a2 = p.work(x[2 * nb * H:])
    lag1_hold(p, a2, p.lag1(), "third call")
    for k, a in enumerate((a0, a1, a2)):
        for c in range(len(chans)):
            same_bytes(a[c], plain[k][c], "call %d ch%d against a handle that never had lag-1" % (k, c))
    p.reset()
    assert p.lag1_device() is not None
    b0 = p.work(x[:nb * H])
    lag1_hold(p, b0, p.lag1(), "after reset()")
    for c in range(len(chans)):
        same_bytes(b0[c], plain[0][c], "after reset(), ch%d" % c)
    # switched off and on again: the old result is gone
    dev = p.lag1_device()
    p.set_lag1(False)
    assert p.lag1_device() is None and raw_lag1(p._h, nb, len(chans))[0] == -1
    p.set_lag1(True)
    assert p.lag1_device() == dev                                          # allocated once
    assert raw_lag1(p._h, nb, len(chans))[0] == -1
    assert lib.fdc_pipeline_set_lag1(None, 1) == -1 and lib.fdc_pipeline_lag1(None, None, nb) == -1


@pytest.mark.parametrize("N,chans", [(4096, EXAMPLE), (16384, BANK)], ids=["path 5", "bank"])
def test_on_and_off_again_restores_the_fused_integer_route(N, chans):
    """sc16 output: the kernels narrow in their own stores ("fused"), write float under the pass ("narrowed") and narrow themselves again once it is off;
    the narrow bytes are the same three times"""
    R, nb = 2, 4
    H = N - N // R
    x = signal(nb * H, 8)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    yf = p.work(x)
    scale = int_scale(yf, np.int16)
    p.set_output_format("sc16", scale)
    p.reset()
    before, d0 = p.work(x), p.describe()
    got, s, d, after = on_and_off(p, lambda: p.work(x))
    d1 = p.describe()
    for c in range(len(chans)):
        same_bytes(got[c], before[c], "on against before, ch%d" % c)
        same_bytes(after[c], before[c], "off again against before, ch%d" % c)
        same_bytes(got[c], narrowed(yf[c], scale, np.int16), "against the narrowed float samples, ch%d" % c)
    lag1_hold(p, yf, s, "sc16 output: S is that of the float samples")
    assert "output sc16: narrowed" in d and "lag1" not in d0 and "lag1" not in d1, (d0, d, d1)
    assert FORCED or ("output sc16: fused" in d0 and "output sc16: fused" in d1), (d0, d1)


def test_no_channels():
    """C = 0: on is accepted and every result is empty"""
    N, R, nb = 4096, 2, 3
    H = N - N // R
    p = G.Pipeline(N, R, [], max_blocks=nb, keep_spectrum=True)
    p.set_lag1(True)
    outs, spec = p.work(signal(nb * H, 1), want_spectrum=True)
    assert outs == [] and np.abs(spec).max() > 0
    assert p.lag1().shape == (nb, 0)
    assert _lib.lib().fdc_pipeline_lag1(p._h, None, nb) == 0 and _lib.lib().fdc_pipeline_lag1(p._h, None, nb + 1) == -1


SINKS_KW = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01)


def test_refused_while_a_pipelined_sinks_batch_is_inside():
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x = signal(nb * H, 7)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, lookahead=True, max_blocks=nb, **SINKS_KW)
    p.work(x, sinks=bank)
    with pytest.raises(G.FdcError) as e:
        p.set_lag1(True)
    assert e.value.status == -1 and p.lag1_device() is None
    while p.flush_sinks(bank) > 0:
        pass
    p.set_lag1(True)                                                       # nothing inside any more
    assert p.lag1_device() is not None
    p.set_lag1(False)
    p.work(x, sinks=bank)
    assert _lib.lib().fdc_pipeline_set_lag1(p._h, 1) == -1 and p.lag1_device() is None
    while p.flush_sinks(bank) > 0:
        pass


def test_entries_that_give_no_lag1_are_refused():
    """work_sinks, work_spectrum, process_device_power and work_waterfall return FDC_ERR_INVALID_ARGUMENT and leave history and block counter untouched:
    the next work continues the stream bit for bit; flush_sinks still flushes"""
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
        p.set_lag1(True)
        a0, b0 = p.work(x[:nb * H]), q.work(x[:nb * H])
        s0 = p.lag1()
        for name, call in entries:
            with pytest.raises(G.FdcError) as e:
                call()
            assert e.value.status == -1 and "lag-1" in str(e.value), name
        assert p.flush_sinks(bank) == 0                                    # not refused: nothing inside, nothing to flush
        same_bytes(p.lag1(nb), s0, "the result of the last successful call")
        a1, b1 = p.work(x[nb * H:]), q.work(x[nb * H:])
        for c in range(len(EXAMPLE)):
            same_bytes(a0[c], b0[c], "before the refusals, ch%d" % c)
            same_bytes(a1[c], b1[c], "after the refusals, ch%d" % c)
        lag1_hold(p, a1, p.lag1(), "after the refusals")
        p.set_lag1(False)
        for name, call in entries:
            call()                                            # they work again
        p.synchronize()


# ---- what the pass writes -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["fc32 out", "sc16 out"])
@pytest.mark.parametrize("N,chans", [(4096, EXAMPLE), (8192, TINY), (16384, BANK)], ids=["path 5", "tiny rows", "bank"])
def test_footprint_of_the_device_entry(N, chans, fmt):
    """process_device into a d_out between guards, from a ring inside NaN, on a handle of 8 blocks serving calls of 1 and 5: the output bytes are those of
    the setting off and no guard byte changes; of the handle's lag-1 buffer, filled with a poison byte before the call, the first nb * C values are the
    call's and every byte behind them keeps the poison (both poison bytes)"""
    R, mb = 4 if chans is TINY else 2, 8
    H, ovl = N - N // R, N // R
    x = signal(mb * H, 12)
    p = G.Pipeline(N, R, chans, max_blocks=mb)
    q = G.Pipeline(N, R, chans, max_blocks=mb)
    osz, scale = 8, 1.0
    if fmt:
        scale, osz = int_scale(q.work(x), np.int16), 4
        q.reset()
        for h in (p, q):
            h.set_output_format(fmt, scale)
    p.set_lag1(True)
    total = mb * len(chans) * 8
    for nb in (1, 5):
        ring = np.concatenate([np.zeros(ovl, np.complex64), x[:nb * H]])
        q.reset()
        want = q.work(x[:nb * H])
        n_out = p.output_samples(nb)
        flat, seen = np.zeros(n_out * osz, np.uint8), np.zeros(n_out, bool)
        for c, w in enumerate(want):                                       # channel c's stream at channel_offset(c, nb), the streams tiling the buffer
            a, cnt = p.channel_offset(c, nb), nb * p.lout[c]
            assert not seen[a:a + cnt].any()
            seen[a:a + cnt] = True
            flat[a * osz:(a + cnt) * osz] = np.ascontiguousarray(w).reshape(-1).view(np.uint8)
        assert seen.all()
        with DeviceBuffers() as dev:
            band = DeviceBanded(dev, [n_out * osz], sum(p.lout) * osz)
            d_ring = DeviceRing(dev, ring, H)
            d_lag = C.c_void_p(p.lag1_device())
            both = []
            for poison in twice(band):
                assert dev.hip.hipMemset(d_lag, C.c_int(poison), C.c_size_t(total)) == 0 and dev.hip.hipDeviceSynchronize() == 0
                p.process_device(d_ring.ptr, 0, nb, band.ptr())
                s = p.lag1(nb)
                band.check(flat, "%d blocks" % nb)
                d_ring.unchanged("%d blocks" % nb)
                raw = dev.get(d_lag, total, np.uint8)
                used = nb * len(chans) * 8
                assert raw[:used].tobytes() == s.tobytes() and (raw[used:] == poison).all(), (nb, poison)
                both.append(s)
            same_bytes(both[0], both[1], "under both poison bytes")
            # (the float samples of the call: those of a float-output handle; here the setting is checked against the other handle's host entry)
            q.set_output_format(None)
            q.reset()
            lag1_hold(p, q.work(x[:nb * H]), both[0], "process_device, %d blocks" % nb)
            if fmt:
                q.set_output_format(fmt, scale)
    assert POISONS[0] != POISONS[1]


# ---- one order per sum ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,R,chans,flags", [(4096, 2, EXAMPLE, 0), (8192, 4, TINY, 0), (16384, 2, BANK, 0), (4096, 2, EXAMPLE, G.FDC_PIPE_NO_FUSED)],
                         ids=["path 5", "tiny rows at odd offsets", "bank", "example plan, spectrum path"])
def test_cuts_of_the_stream_give_the_same_bits(N, R, chans, flags):
    """7 blocks as 7, as 3 + 4 and as 1 + 1 + 5; on a handle with another chunk_blocks and host_sub_blocks; and by process_device at the same first_block
    into a d_out whose rows land at another alignment"""
    nb = 7
    H, ovl = N - N // R, N // R
    x = signal(nb * H, 2)
    one = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    one.set_lag1(True)
    whole = one.work(x)
    sw = one.lag1()
    lag1_hold(one, whole, sw, "7 blocks")
    for cut in ((3, 4), (1, 1, 5)):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
        p.set_lag1(True)
        parts, b0 = [], 0
        for n in cut:
            p.work(x[b0 * H:(b0 + n) * H])
            parts.append(p.lag1())
            b0 += n
        same_bytes(np.concatenate(parts), sw, "cut %r" % (cut,))
    p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags, chunk_blocks=2, host_sub_blocks=3)
    assert p.chunk_blocks() == 2
    p.set_lag1(True)
    outs = p.work(x)
    for c, (u, v) in enumerate(zip(outs, whole)):
        same_bytes(u, v, "chunk_blocks 2, host_sub_blocks 3, ch%d" % c)
    same_bytes(p.lag1(), sw, "chunk_blocks 2, host_sub_blocks 3")
    # the device entry on blocks 3 .. 6 (a call of 4 blocks: channel c's run starts at 4 * out_off, not at 7 * out_off) and on block 6 alone
    ring = np.concatenate([np.zeros(ovl, np.complex64), x])
    with DeviceBuffers() as dev:
        for first, n in ((3, 4), (6, 1)):
            if chans is TINY:
                # the rows of some channel change between the 16-byte and the 8-byte branch with the cut: nb_call * out_off changes parity
                off = [(one.channel_offset(c, nb) % 2, p.channel_offset(c, n) % 2) for c, lo in enumerate(p.lout) if lo % 2 == 0]
                assert first == 6 or any(a != b for a, b in off), off
            n_out = p.output_samples(n)
            d_in, d_o = dev.put(np.ascontiguousarray(ring[first * H:first * H + ovl + n * H])), dev.put(np.zeros(n_out, np.complex64))
            p.process_device(d_in, first, n, d_o)
            s = p.lag1()
            got = by_channel(p, dev.get(d_o, n_out, np.complex64), n)
            for c, (u, v) in enumerate(zip(got, whole)):
                same_bytes(u, v[first * p.lout[c]:(first + n) * p.lout[c]], "process_device at block %d, ch%d" % (first, c))
            same_bytes(s, sw[first:first + n], "process_device at block %d" % first)
            same_bytes(dev.get(C.c_void_p(p.lag1_device()), n * len(chans), np.complex64).reshape(n, len(chans)), s, "lag1_device")


# ---- call forms ----------------------------------------------------------------------------------------------------------------------------------------

FORMS = [("mixed, N = 8192", 8192, MIXED), ("bank, N = 16384", 16384, BANK), ("example, N = 4096", 4096, EXAMPLE)]
form_ids = [f[0] for f in FORMS]


@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["float", "sc16"])
@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("sub", [0, 2], ids=["one sub-batch", "sub-batches of 2"])
@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_sub_batches_registered_outputs_and_ragged_calls(k, sub, registered, fmt):
    """calls of 1, 7, 3 and 5 blocks (host sub-batches; pageable outputs or registered ones through k_scatter_out / k_scatter_oq): outputs and results are
    those of one call of 16 blocks on a second handle, which holds the models"""
    _name, N, chans = FORMS[k]
    R, mb, sizes = 2, 7, (1, 7, 3, 5)
    H = N - N // R
    x = signal(sum(sizes) * H, 300 + k)
    one = G.Pipeline(N, R, chans, max_blocks=sum(sizes))
    yf, sw, _d = checked(one, lambda: one.work(x), "one call of 16 blocks")
    dt = np.int16 if fmt else np.complex64
    scale = int_scale(yf, np.int16) if fmt else 1.0
    p = G.Pipeline(N, R, chans, max_blocks=mb, host_sub_blocks=sub or None)
    p.set_lag1(True)
    if fmt:
        p.set_output_format(fmt, scale)
    bufs = [np.zeros((mb * lo, 2) if fmt else mb * lo, dt) for lo in p.lout]
    if registered:
        for b in bufs:
            G.register_host(b)
    try:
        pieces, ss, b0 = [[] for _ in chans], [], 0
        for n in sizes:
            outs = [b[:n * lo] for b, lo in zip(bufs, p.lout)]
            p.work(x[b0 * H:(b0 + n) * H], outs=outs)
            ss.append(p.lag1())
            for c, o in enumerate(outs):
                pieces[c].append(o.copy())
            b0 += n
    finally:
        if registered:
            for b in bufs:
                G.unregister_host(b)
    for c in range(len(chans)):
        want = narrowed(yf[c], scale, np.int16) if fmt else yf[c]
        same_bytes(np.concatenate(pieces[c]), want, "ragged stream ch%d" % c)
    same_bytes(np.concatenate(ss), sw, "ragged stream: lag-1")
    d = p.describe()
    assert "lag1: pass" in d and (not fmt or "output sc16: narrowed" in d), d


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_outputs_that_are_not_wanted(k):
    """outs[c] = NULL for some channels, and for all of them (a call that only watches the band): the result is still complete"""
    _name, N, chans = FORMS[k]
    R, nb = 2, 5
    H = N - N // R
    x = signal(nb * H, 310 + k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    full, sw, _d = checked(p, lambda: p.work(x), "every output")
    p.set_lag1(True)
    lib = _lib.lib()
    for keep in ([c % 2 == 0 for c in range(len(chans))], [False] * len(chans)):
        p.reset()
        outs = [np.zeros(nb * lo, np.complex64) for lo in p.lout]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data if kp else None for o, kp in zip(outs, keep)])
        assert lib.fdc_pipeline_work(p._h, x.ctypes.data, nb, ptrs, None) == nb
        same_bytes(p.lag1(nb), sw, "outputs kept: %r" % keep)
        for c, kp in enumerate(keep):
            same_bytes(outs[c], full[c] if kp else np.zeros_like(full[c]), "ch%d" % c)


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_real_and_integer_input(k):
    _name, N, chans = FORMS[k]
    R, nb = 2, 5
    H = N - N // R
    xr = signal(nb * H, 320 + k).real.copy()
    xi = iq(nb * H, np.int16, 33)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    checked(p, lambda: p.work_real(xr), "work_real")
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    checked(p, lambda: p.work_iq(xi, scale=2.0 ** -12), "work_iq")


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_span_entries_far_into_the_stream(k):
    """work_span and work_span_iq at first_block = 2^40 + 3: bit-equal to the same rows of a whole call (the value needs no sample of another span: the
    whole call starts at the halo too), and the row index is the block of the CALL"""
    _name, N, chans = FORMS[k]
    R, nb, first = 2, 4, 2 ** 40 + 3
    H, ovl = N - N // R, N // R
    x, halo = signal(nb * H, 330 + k), signal(ovl, 24)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    p.set_lag1(True)
    got = work_span(p, halo, x, first, nb)
    s = p.lag1(nb)
    p.set_lag1(False)
    for c, (u, v) in enumerate(zip(got, work_span(p, halo, x, first, nb))):
        same_bytes(u, v, "work_span, lag-1 on against off, ch%d" % c)
    lag1_hold(p, got, s, "work_span at block 2^40 + 3")
    # the spans of that call, each with the samples in front of it as its halo: the same rows, bit for bit
    ring = np.concatenate([halo, x])
    p.set_lag1(True)
    for j, n in ((1, 3), (3, 1), (0, 2)):
        part = work_span(p, np.ascontiguousarray(ring[j * H:j * H + ovl]), np.ascontiguousarray(x[j * H:(j + n) * H]), first + j, n)
        for c, (u, v) in enumerate(zip(part, got)):
            same_bytes(u, v[j * p.lout[c]:(j + n) * p.lout[c]], "the span at block 2^40 + %d, ch%d" % (3 + j, c))
        same_bytes(p.lag1(n), s[j:j + n], "the span at block 2^40 + %d: the rows of the whole call" % (3 + j))
    p.reset()
    p.set_lag1(True)
    xi, hi = iq(nb * H, np.int16, 31), iq(ovl, np.int16, 32)
    gi = p.work_span_iq(hi, xi, first, scale=2.0 ** -12)
    lag1_hold(p, gi, p.lag1(), "work_span_iq at block 2^40 + 3")


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_device_entries(k):
    """process_device and process_device_iq at first_block = 13 on a stream of the caller's: the result comes from fdc_pipeline_lag1 (which synchronises
    that stream) and from the device buffer.  Above max_blocks a device call with lag-1 on is refused and nothing is enqueued."""
    _name, N, chans = FORMS[k]
    R, nb, first = 2, 4, 13
    H, ovl = N - N // R, N // R
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    n_out = p.output_samples(nb)
    ring_f, ring_i = signal(ovl + nb * H, 340 + k), iq(ovl + nb * H, np.int16, 31)
    with DeviceBuffers() as dev:
        st = C.c_void_p()
        assert dev.hip.hipStreamCreate(C.byref(st)) == 0
        try:
            d_f, d_i, d_o = dev.put(ring_f), dev.put(ring_i), dev.put(np.zeros(n_out, np.complex64))
            for what, call in (("process_device", lambda: p.process_device(d_f, first, nb, d_o, stream=st)),
                               ("process_device_iq", lambda: p.process_device_iq("sc16", 2.0 ** -12, d_i, first, nb, d_o, stream=st))):
                def run():
                    call()
                    s = p.lag1() if p.lag1_device() is not None else None      # (synchronises the call's stream)
                    assert dev.hip.hipStreamSynchronize(st) == 0
                    return by_channel(p, dev.get(d_o, n_out, np.complex64), nb), s
                p.set_lag1(True)
                got, s = run()
                d = p.describe()
                same_bytes(dev.get(C.c_void_p(p.lag1_device()), nb * len(chans), np.complex64).reshape(nb, len(chans)), s, what + ": the device buffer")
                p.set_lag1(False)
                plain, _ = run()
                for c, (u, v) in enumerate(zip(got, plain)):
                    same_bytes(u, v, "%s, lag-1 on against off, ch%d" % (what, c))
                lag1_hold(p, got, s, what)
                assert "lag1: pass" in d, d
            # above max_blocks: refused with lag-1 on (nothing is enqueued: the output stays as it is), served without
            big = dev.put(np.zeros(ovl + 2 * nb * H, np.complex64))
            d_big = dev.put(np.full(p.output_samples(2 * nb), 7, np.complex64))
            p.set_lag1(True)
            with pytest.raises(G.FdcError) as e:
                p.process_device(big, 0, 2 * nb, d_big)
            assert e.value.status == -1
            p.synchronize()
            assert (dev.get(d_big, p.output_samples(2 * nb), np.complex64) == 7).all()
            p.set_lag1(False)
            p.process_device(big, 0, 2 * nb, d_big)
            p.synchronize()
        finally:
            dev.hip.hipStreamDestroy(st)


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_group_of_two_virtual_members_against_one_handle(k):
    _name, N, chans = FORMS[k]
    R, nb = 2, 8
    H = N - N // R
    x = signal(2 * nb * H, 350 + k)
    g = G.PipelineGroup(N, R, chans, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    lib = _lib.lib()
    rc, out = raw_lag1(g._h, nb, len(chans), lib.fdc_pipeline_group_lag1)
    assert rc == -1 and np.isnan(out).all()                               # before any call
    g.set_lag1(True)
    p.set_lag1(True)
    assert raw_lag1(g._h, nb, len(chans), lib.fdc_pipeline_group_lag1)[0] == -1
    for j, n in enumerate((nb, 5)):                                        # 5 blocks: spans of 3 and 2
        a, b = g.work(x[j * nb * H:(j * nb + n) * H]), p.work(x[j * nb * H:(j * nb + n) * H])
        for c, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, "call %d ch%d" % (j, c))
        assert sum(m > 0 for _f, m in g.last_spans()) == 2
        sg = g.lag1()
        same_bytes(sg, p.lag1(), "call %d: the group's result against one handle's" % j)
        lag1_hold(p, a, sg, "group call %d" % j)
        assert raw_lag1(g._h, n + 1, len(chans), lib.fdc_pipeline_group_lag1)[0] == -1
    g.set_lag1(False)
    assert raw_lag1(g._h, 5, len(chans), lib.fdc_pipeline_group_lag1)[0] == -1
    assert lib.fdc_pipeline_group_set_lag1(None, 1) == -1 and lib.fdc_pipeline_group_lag1(None, None, 1) == -1


# ---- rows that are not finite -------------------------------------------------------------------------------------------------------------------------

def test_rows_that_are_not_finite_disturb_no_other_row():
    """an input sample of NaN reaches the blocks that overlap it; every other row has the bits it has without it"""
    N, R, nb = 8192, 2, 6
    H = N - N // R
    x = signal(nb * H, 9)
    p = G.Pipeline(N, R, MIXED, max_blocks=nb)
    p.set_lag1(True)
    p.work(x)
    sc = p.lag1()
    bad = x.copy()
    bad[4 * H + 100] = complex(np.nan, 1.0)
    p.reset()
    outs = p.work(bad)
    s = p.lag1()
    hit = np.array([[not np.isfinite(o[m * lo:(m + 1) * lo]).all() for o, lo in zip(outs, p.lout)] for m in range(nb)])
    assert hit.any() and not hit.all()
    same_bytes(s[~hit], sc[~hit], "the rows without a NaN")
    assert np.isnan(s[hit].real).all() and np.isnan(s[hit].imag).all()
    for c, lo in enumerate(p.lout):
        s64, _m = model64(outs[c], lo)
        assert (np.isnan(s64.real) == np.isnan(s[:, c].real)).all() and (np.isnan(s64.imag) == np.isnan(s[:, c].imag)).all(), c


# ---- the order of the settings: cut -> fine tuning -> gain -> levels, lag-1 -> narrowing --------------------------------------------------------------

@pytest.mark.parametrize("N,chans", [(16384, BANK), (4096, EXAMPLE), (8192, MIXED)], ids=["bank", "path 5", "spectrum path"])
def test_with_fine_tuning_the_samples_are_the_turned_ones(N, chans):
    """S is that of the turned samples.  Turning by exp(-2 pi i nu t) multiplies every exact term by exp(-2 pi i nu), so S = exp(-2 pi i nu) S0 but for
    the roundings: of S against the float64 sum over the turned float32 samples ((lout + 8) 2^-24 M per component, asserted by the models), of S0
    against the float64 sum over the plain samples (the same), and of the turn itself (a turned sample is within 11 2^-24 |y| of its exact product,
    DESIGN "Fine tuning", Error bound: each term within 22 2^-24 |a| |b| to first order, the sum within 23 2^-24 M with the second order).  So
    |S - exp(-2 pi i nu) S0| <= (2 sqrt(2) (lout + 8) + 23) 2^-24 M, and arg moves by -2 pi nu within asin of that over |S|."""
    R, nb = 2, 4
    H = N - N // R
    x = signal(nb * H, 400)
    nu = np.random.default_rng(3).uniform(-0.45, 0.45, len(chans))
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    plain, s0, _d = checked(p, lambda: p.work(x), "fine tuning off")
    p.set_fine_tuning(nu)
    got, s, d = checked(p, lambda: p.work(x), "fine tuning on")
    p.set_fine_tuning(None)
    assert "fine tuning: " in d and any(u.tobytes() != v.tobytes() for u, v in zip(got, plain)), d
    for c, lo in enumerate(p.lout):
        _s64, m = model64(got[c], lo)
        lim = (2 * np.sqrt(2.0) * (lo + 8) + 23) * 2.0 ** -24 * m * 1.001     # (M of the turned samples is M of the plain ones within 2^-19)
        want = s0[:, c].astype(np.complex128) * np.exp(-2j * np.pi * nu[c])
        err = np.abs(s[:, c].astype(np.complex128) - want)
        print("ch%d: |S - turned S0| at most %.3g of its bound" % (c, (err / lim).max()))
        assert (err <= lim).all(), (c, (err / lim).max())
        strong = np.abs(want) > 0.05 * m                                   # where the row has a mean frequency worth the name
        moved = np.angle(s[strong, c].astype(np.complex128) * np.conj(s0[strong, c].astype(np.complex128)) * np.exp(2j * np.pi * nu[c]))
        assert (np.abs(moved) <= np.arcsin(np.minimum(1.0, lim[strong] / np.abs(want[strong]))) + 1e-12).all(), c


@pytest.mark.parametrize("N,chans", [(16384, BANK), (4096, EXAMPLE)], ids=["bank", "path 5"])
@pytest.mark.parametrize("k", [-3, 1, 5])
def test_under_a_power_of_two_gain_s_is_the_scaled_s(N, chans, k):
    """g = 2^k for every channel: every sample is scaled exactly, every product by 4^k exactly, and so is every sum: S bit-equal to 4^k times the S
    of the gains-off call (no value near the ends of the exponent range: the input is of order 1)"""
    R, nb = 2, 4
    H = N - N // R
    x = signal(nb * H, 410)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    _plain, s0, _d = checked(p, lambda: p.work(x), "gains off")
    p.set_gains(np.full(len(chans), 2.0 ** k, np.float32))
    yg, s, d = checked(p, lambda: p.work(x), "g = 2^%d" % k)
    assert "gains: " in d, d
    same_bytes(s, (s0.view(np.float32) * np.float32(4.0 ** k)).view(np.complex64), "S under g = 2^%d against 4^%d S" % (k, k))
    # ... and on the route where the gain pass narrows and leaves the float staging as it was cut (the device entry, sc16 output)
    scale = int_scale(yg, np.int16)
    p.set_output_format("sc16", scale)
    p.set_lag1(True)
    p.reset()
    gi = p.work(x)
    d = p.describe()
    same_bytes(p.lag1(), s, "sc16 output, g = 2^%d" % k)
    for c, (u, v) in enumerate(zip(gi, yg)):
        same_bytes(u, narrowed(v, scale, np.int16), "sc16 output, ch%d" % c)
    assert "output sc16: narrowed" in d and (FORCED or "gains: with the narrowing" in d), d


@pytest.mark.parametrize("N,chans", [(16384, BANK), (4096, EXAMPLE), (8192, TINY)], ids=["bank", "path 5", "tiny rows"])
def test_with_levels_both_results_are_those_of_each_alone(N, chans):
    """levels and lag-1 on together, with fine tuning and gains off and on (every levels route: the pass, with the rotation, with the gains): the levels
    are bit-equal to levels alone, S to lag-1 alone, the outputs to neither"""
    R, nb = 4 if chans is TINY else 2, 5
    H = N - N // R
    x = signal(nb * H, 420)
    g = np.random.default_rng(4).uniform(0.5, 2.0, len(chans)).astype(np.float32)
    nu = edge_nus(len(chans), 2)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    for fine, gain in ((False, False), (True, False), (False, True), (True, True)):
        what = "fine tuning %s, gains %s" % (fine, gain)
        p.set_fine_tuning(nu if fine else None)
        p.set_gains(g if gain else None)
        y, s, _d = checked(p, lambda: p.work(x), what + ", lag-1 alone")
        p.set_levels(True)
        p.reset()
        y1 = p.work(x)
        lev = p.levels()
        p.set_lag1(True)
        p.reset()
        y2 = p.work(x)
        d = p.describe()
        same_bytes(p.levels(), lev, what + ": the levels")
        same_bytes(p.lag1(), s, what + ": S")
        for c in range(len(chans)):
            same_bytes(y1[c], y[c], what + ", levels alone, ch%d" % c)
            same_bytes(y2[c], y[c], what + ", both, ch%d" % c)
        assert "levels: " in d and "lag1: pass" in d, d
        p.set_levels(False)
        p.set_lag1(False)


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
pw = G.Pipeline(8192, 2, MIXED, max_blocks=nb)
po = G.Pipeline(8192, 2, MIXED, max_blocks=nb)
pd = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
po.set_output_format("sc16", 100.0)
po.set_fine_tuning([0.1, -0.2])
po.set_gains([2.0, 0.5])
po.set_levels(True)
for h in (p, pw, po, pd, g):
    h.set_lag1(True)
d_ring, d_out = C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(8 * pd.output_samples(nb))) == 0

def afc(h, x):
    # the loop of examples/afc.py: read, average, set
    h.work(x)
    h.set_fine_tuning(0.5 * G.lag1_frequency(h.lag1().mean(axis=0)))

entries = {"fdc_pipeline_work (path 5)": lambda: (p.work(x), p.lag1()),
           "fdc_pipeline_work (spectrum path)": lambda: (pw.work(x2), pw.lag1()),
           "fdc_pipeline_work (fine tuning, gains, levels, sc16 out)": lambda: (po.work(x2), po.lag1(), po.levels()),
           "fdc_pipeline_process_device": lambda: (pd.process_device(d_ring, 5, nb, d_out), pd.lag1()),
           "fdc_pipeline_group_work": lambda: (g.work(x), g.lag1()),
           "an AFC loop": lambda: afc(pw, x2),
           "fdc_pipeline_set_lag1 again": lambda: (pw.set_lag1(False), pw.set_lag1(True), pw.work(x2), pw.lag1())}
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
assert "lag1: pass" in p.describe() and "lag1: pass" in po.describe(), (p.describe(), po.describe())
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
    x = signal(nb * H, 11)
    on = G.FrequencyDomainChannelizer(inptype=8, lag1=True, **KW)
    off = G.FrequencyDomainChannelizer(inptype=8, **KW)
    assert on.lag1 is None and off.lag1 is None
    ya, yb = on.work(x), off.work(x)
    assert on.lag1.shape == (nb, len(KW["throughput_channels"])) and on.lag1.dtype == np.complex64 and off.lag1 is None
    for c, (u, v) in enumerate(zip(ya, yb)):
        same_bytes(u, v, "port %d" % c)
    lag1_hold(on.pipeline, ya, on.lag1, "hier block")
    # a call without items: an empty array
    on.work(x[:0])
    assert on.lag1.shape == (0, 3) and on.lag1.dtype == np.complex64
    # together with iq_output, fine_tuning and levels: S is that of the float ports of a block without iq_output, the ports its narrowed samples
    scale = int_scale(ya, np.int16)
    fine = G.FrequencyDomainChannelizer(inptype=8, lag1=True, fine_tuning=True, **KW)
    both = G.FrequencyDomainChannelizer(inptype=8, lag1=True, levels=True, fine_tuning=True, iq_output="sc16", iq_output_scale=scale, **KW)
    yf, yi = fine.work(x), both.work(x)
    lag1_hold(fine.pipeline, yf, fine.lag1, "hier block with fine tuning")
    same_bytes(both.lag1, fine.lag1, "hier block with iq_output: S is taken before the narrowing")
    assert both.levels.shape == (nb, 3, 2)
    for c, (u, v) in enumerate(zip(yi, yf)):
        same_bytes(u, narrowed(v, scale, np.int16), "port %d, sc16" % c)
    # the Float input type, and two devices
    fl = G.FrequencyDomainChannelizer(inptype=4, lag1=True, **KW)
    yr = fl.work(x.real.copy())
    lag1_hold(fl.pipeline, yr, fl.lag1, "hier block, Float input")
    kw = dict(KW, max_blocks=16)
    grp = G.FrequencyDomainChannelizer(inptype=8, lag1=True, devices=[0, 0], **kw)
    one = G.FrequencyDomainChannelizer(inptype=8, lag1=True, **kw)
    x16 = signal(16 * H, 12)
    yg, _y1 = grp.work(x16), one.work(x16)
    assert isinstance(grp.pipeline, G.PipelineGroup) and grp.lag1.shape == (16, 3)
    same_bytes(grp.lag1, one.lag1, "devices=[0, 0]")
    lag1_hold(one.pipeline, yg, grp.lag1, "hier block on two virtual members")


# ---- a closed loop on a tone ---------------------------------------------------------------------------------------------------------------------------

def test_a_closed_loop_on_a_tone(oracle):
    """One 64-bin channel (lout = 32), a unit tone 0.4 bin of N above its slice centre in noise of sigma 0.05 per component, two calls of 16 blocks.
    The expected values are the oracle's: its float64 run of the same stream, S in float64 over its outputs, and for the second call its outputs turned
    by exp(-2 pi i e1 t) in float64.  The first estimate has the oracle's sign and size; after one set_fine_tuning(0 + estimate) the second call's
    |estimate| is smaller by the factor the oracle shows, with a margin of 10 on that factor."""
    N, R, nb, delta = 4096, 2, 16, 0.4
    H = N - N // R
    freq = (2600 + delta) / N
    f, l, lout, pbw, sbw = G.get_opt_channelparams(N, R, freq, 40.0 / N)
    assert (f, l, lout) == (2568, 64, 32)
    n = np.arange(2 * nb * H, dtype=np.float64)
    rng = np.random.default_rng(77)
    x = (np.exp(2j * np.pi * (freq - 0.5) * n) + 0.05 * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))).astype(np.complex64)

    def estimate(s):
        return float(G.lag1_frequency(s.astype(np.complex128).mean()))

    yo = oracle.channelizer(N, R, 1, [(f, l, pbw, sbw)], x)[0][0]
    s1, m1 = model64(yo[:nb * lout], lout)
    e1 = estimate(s1)
    t = np.arange(nb * lout, 2 * nb * lout, dtype=np.float64)
    s2, _m2 = model64((yo[nb * lout:].astype(np.complex128) * np.exp(-2j * np.pi * e1 * t)).astype(np.complex64), lout)
    e2 = estimate(s2)
    print("oracle: first estimate %.12g (the tone sits at %.12g), second %.12g, factor %.6g" % (e1, delta / l, e2, abs(e2) / abs(e1)))
    # the oracle's two numbers, as this test computes them on the CPU: e1 = +0.00652748610099 cycles per output sample (the tone at 0.4 / 64 = 0.00625,
    # pulled by the noise and the slope of the channel's window), e2 = +1.69163148066e-05: the loop shrinks the residual by the factor 0.00259155
    assert e1 == pytest.approx(0.00652748610099, abs=1e-9) and abs(e2) / abs(e1) == pytest.approx(0.00259155, rel=1e-3)
    p = G.Pipeline(N, R, [(f, l, pbw, sbw)], windowtype=1, max_blocks=nb)
    p.set_lag1(True)
    y1 = p.work(x[:nb * H])
    d1 = estimate(p.lag1()[:, 0])
    lag1_hold(p, y1, p.lag1(), "the first call")
    # sign and size: the device's float32 outputs are within 1e-5 of the oracle's relative to their largest value (the bound of smoke()), so each term
    # moves by at most 2e-5 |a| |b| and each S by (2e-5 + (lout + 8) 2^-24) M; the angle of the mean by at most asin of that over |mean S|
    lim = np.arcsin((2e-5 + (lout + 8) * 2.0 ** -24) * m1.mean() * 1.01 / abs(s1.mean())) / (2 * np.pi)
    print("device: first estimate %.12g, %.3g from the oracle's (allowed %.3g)" % (d1, abs(d1 - e1), lim))
    assert d1 > 0 and abs(d1 - e1) <= lim, (d1, e1, lim)
    p.set_fine_tuning([0.0 + d1])
    p.work(x[nb * H:])
    d2 = estimate(p.lag1()[:, 0])
    print("device: second estimate %.12g, factor %.6g (the oracle's %.6g)" % (d2, abs(d2) / abs(d1), abs(e2) / abs(e1)))
    assert "fine tuning: " in p.describe() and "lag1: pass" in p.describe()
    assert abs(d2) <= 10.0 * (abs(e2) / abs(e1)) * abs(d1), (d2, d1, e2, e1)          # 10 x 0.00259155
