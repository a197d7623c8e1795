"""GPU tests (-m gpu) of the channel gains (fdc_pipeline_set_gains, fdc_pipeline_gains, fdc_pipeline_group_set_gains; include/fdc_amd.h): the setting's
semantics, the refusals, the order of the two roundings, the levels' summation order, every call form, no allocation in the steady state, the hier block.
tests/test_gains_routes_gpu.py covers every plan and the inside of the device code.

Every comparison is in bytes, against numpy's statement of the definition (tests/test_gains_cpu.py: gained) applied to the float32 outputs of THE SAME
handle with gains off: got == gained(y', g), or narrowed(gained(y', g), scale) with integer output.  The levels are those of the gained samples: the
model of tests/test_levels_cpu.py (agrees: its derived bound (lout + 8) 2^-24 for power, bit-equality for peak) on gained(y', g), and byte-equality
across routes and cuts.  No tolerance of its own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from test_fine_tuning_gpu import BANK, FORCED, MIXED, narrowed, signal, work_span
from test_fine_tuning_routes_gpu import TINY, DeviceBuffers, by_channel, edge_nus, int_scale
from test_gains_cpu import draw_gains, gained
from test_iq_input_gpu import EXAMPLE, iq, same_bytes
from test_levels_cpu import agrees

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODT = {"sc16": np.int16, "sc8": np.int8}


def wanted(y, g, fmt=None, scale=None):
    """what a call must write for every channel: y = the float outputs with gains off"""
    w = [gained(v, gc) for v, gc in zip(y, g)]
    return [narrowed(v, scale, ODT[fmt]) for v in w] if fmt else w


def gained_levels_hold(p, y, g, lev, what):
    """the levels' model on the gained float samples of every channel (a muted channel: power and peak exactly 0)"""
    nb = y[0].size // p.lout[0] if y else 0
    assert lev.shape == (nb, len(p.lout), 2) and lev.dtype == np.float32, (what, lev.shape)
    for c, v in enumerate(y):
        agrees(lev[:, c], gained(v, g[c]), p.lout[c], "%s ch%d" % (what, c))


def run(p, call, g, fmt=None, scale=None, levels=False):
    """call() from block 0 of handle p with gains g (None: off), output format fmt and levels; returns (outputs, levels or None, describe) and leaves
    the three settings off"""
    p.set_gains(g)
    p.set_levels(levels)
    p.set_output_format(fmt, scale if fmt else 1.0)
    p.reset()
    got = call()
    # (the block count from the outputs: a call made through the raw entry leaves none with the Python object)
    lev, d = (p.levels(len(got[0]) // p.lout[0]) if levels else None), p.describe()
    p.set_gains(None)
    p.set_levels(False)
    p.set_output_format(None)
    p.reset()
    return got, lev, d


def checked(p, call, g, what, fmt=None, scale=None, levels=False, y=None):
    """run() against the definition on the same handle's gains-off float outputs (y: those, where the caller has them already)"""
    if y is None:
        y, _l, d0 = run(p, call, None)
        assert "gains" not in d0, d0
    got, lev, d = run(p, call, g, fmt, scale, levels)
    for c, (u, v) in enumerate(zip(got, wanted(y, g, fmt, scale))):
        same_bytes(u, v, "%s ch%d (g = %r)" % (what, c, float(g[c])))
    if levels:
        gained_levels_hold(p, y, g, lev, what)
    assert "gains: " in d, d
    return y, got, lev, d


def raw_set(h, arr, n, fn=None):
    a = None if arr is None else np.ascontiguousarray(arr, np.float32)
    return (fn or _lib.lib().fdc_pipeline_set_gains)(h, None if a is None else a.ctypes.data_as(C.POINTER(C.c_float)), n)


# ---- B1. the setting -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,chans", [(4096, EXAMPLE), (16384, BANK)], ids=["example, N = 4096", "bank, N = 16384"])
def test_setting_semantics(N, chans):
    R, nb, nc = 2, 3, len(chans)
    H = N - N // R
    x = signal(3 * nb * H, 6)
    g = draw_gains(nc, 1)
    q = G.Pipeline(N, R, chans, max_blocks=nb)
    plain = [q.work(x[k * nb * H:(k + 1) * nb * H]) for k in range(3)]
    scale = int_scale(wanted(plain[0], g), np.int16)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    # off by default: ones, no line in describe
    same_bytes(p.gains(), np.ones(nc, np.float32), "gains() by default")
    a0 = p.work(x[:nb * H])
    assert "gains" not in p.describe()
    # on between two calls of one stream: the history is not touched, the second call is the gained second call of the plain stream
    p.set_gains(g)
    same_bytes(p.gains(), g, "gains() while on")
    a1 = p.work(x[nb * H:2 * nb * H])
    assert "gains: pass" in p.describe(), p.describe()
    # all ones is off; then other gains for the third call
    p.set_gains(np.ones(nc))
    same_bytes(p.gains(), np.ones(nc, np.float32), "all ones")
    g2 = draw_gains(nc, 2)
    p.set_gains(g2)
    a2 = p.work(x[2 * nb * H:])
    for c in range(nc):
        same_bytes(a0[c], plain[0][c], "call 0 ch%d" % c)
        same_bytes(a1[c], gained(plain[1][c], g[c]), "call 1 ch%d" % c)
        same_bytes(a2[c], gained(plain[2][c], g2[c]), "call 2 ch%d" % c)
    # the setting survives reset()
    p.reset()
    same_bytes(p.gains(), g2, "gains() after reset()")
    b0 = p.work(x[:nb * H])
    for c in range(nc):
        same_bytes(b0[c], gained(plain[0][c], g2[c]), "after reset(), ch%d" % c)
    assert "gains: pass" in p.describe()
    # wrong n, NaN and Inf are refused by the library itself, with the previous gains still in force
    lib = _lib.lib()
    bad = g.copy()
    for n, arr in ((nc - 1, g), (nc + 1, np.ones(nc + 1)), (0, None), (nc - 1, None)):
        assert raw_set(p._h, arr, n) == -1, n
    for v in (np.nan, np.inf, -np.inf):
        bad[:] = g
        bad[nc - 1] = v
        assert raw_set(p._h, bad, nc) == -1, v
    same_bytes(p.gains(), g2, "gains() after the refusals")
    p.reset()
    for c, o in enumerate(p.work(x[:nb * H])):
        same_bytes(o, b0[c], "after the refusals, ch%d" % c)
    out = np.zeros(nc + 1, np.float32)
    assert lib.fdc_pipeline_gains(p._h, out.ctypes.data_as(C.POINTER(C.c_float)), nc + 1) == -1 and not out.any()
    assert lib.fdc_pipeline_gains(p._h, None, nc) == -1
    # with sc16 output: on, then off again restores the parent's bytes and its fused route
    p.set_gains(None)
    p.set_output_format("sc16", scale)
    p.reset()
    i0 = p.work(x[:nb * H])
    d0 = p.describe()
    assert "gains" not in d0 and (FORCED or "output sc16: fused" in d0), d0
    p.set_gains(g)
    p.reset()
    i1 = p.work(x[:nb * H])
    d1 = p.describe()
    assert "output sc16: narrowed" in d1 and "gains: with the narrowing" in d1, d1
    p.set_gains(None)
    p.reset()
    i2 = p.work(x[:nb * H])
    assert "gains" not in p.describe() and (FORCED or "output sc16: fused" in p.describe()), p.describe()
    for c in range(nc):
        same_bytes(i0[c], narrowed(plain[0][c], scale, np.int16), "sc16, gains off, ch%d" % c)
        same_bytes(i1[c], narrowed(gained(plain[0][c], g[c]), scale, np.int16), "sc16, gains on, ch%d" % c)
        same_bytes(i2[c], i0[c], "sc16, gains off again, ch%d" % c)
    assert raw_set(p._h, np.ones(nc), nc) == 0 and raw_set(p._h, None, nc) == 0


def test_no_channels():
    """C = 0: n = 0 is accepted, any other n refused, every result is empty"""
    N, R, nb = 4096, 2, 3
    H = N - N // R
    p = G.Pipeline(N, R, [], max_blocks=nb, keep_spectrum=True)
    p.set_gains(np.zeros(0, np.float32))
    p.set_gains(None)
    assert raw_set(p._h, None, 0) == 0 and raw_set(p._h, np.ones(1), 1) == -1
    assert p.gains().shape == (0,)
    outs, spec = p.work(signal(nb * H, 1), want_spectrum=True)
    assert outs == [] and np.abs(spec).max() > 0 and "gains" not in p.describe()


SINKS_KW = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01)


def test_refused_while_a_pipelined_sinks_batch_is_inside():
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x = signal(nb * H, 7)
    g = draw_gains(len(EXAMPLE), 3)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, lookahead=True, max_blocks=nb, **SINKS_KW)
    p.work(x, sinks=bank)
    with pytest.raises(ValueError):
        p.set_gains(g)
    assert raw_set(p._h, g, len(g)) == -1
    same_bytes(p.gains(), np.ones(len(g), np.float32), "gains() after the refusal")
    while p.flush_sinks(bank) > 0:
        pass
    p.set_gains(g)                                                         # nothing inside any more
    same_bytes(p.gains(), g, "gains()")


def test_entries_that_write_the_channels_as_they_are_cut_are_refused():
    """work_sinks, work_spectrum, process_device_power and work_waterfall return FDC_ERR_INVALID_ARGUMENT and leave history and block counter untouched:
    the next work continues the stream bit for bit"""
    N, R, nb = 4096, 2, 3
    H, ovl = N - N // R, N // R
    x = signal(2 * nb * H, 7)
    g = draw_gains(len(EXAMPLE), 4)
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
        p.set_gains(g)
        a0, b0 = p.work(x[:nb * H]), q.work(x[:nb * H])
        for name, call in entries:
            with pytest.raises(G.FdcError) as e:
                call()
            assert e.value.status == -1 and "gains" in str(e.value), name
        assert p.flush_sinks(bank) == 0                                   # flushing is not refused
        a1, b1 = p.work(x[nb * H:]), q.work(x[nb * H:])
        for c in range(len(EXAMPLE)):
            same_bytes(a0[c], gained(b0[c], g[c]), "before the refusals, ch%d" % c)
            same_bytes(a1[c], gained(b1[c], g[c]), "after the refusals, ch%d" % c)
        p.set_gains(None)
        for name, call in entries:
            call()                                            # they work again
        p.synchronize()


# ---- B2. the order of the two roundings ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g1", [1.0 / 3.0, 2.7, -0.37, 1000.123])
def test_the_gain_is_rounded_before_the_narrowing(g1):
    """Integer output is oq(f32(y' g) scale), two roundings, not oq(y' f32(g scale)).  One gain on all 64 channels of the bank: 8 blocks are 131072
    components; the scale puts their standard deviation at about 8000 counts of sc16, where the two orders differ in a handful of components.  The numpy
    side alone shows that difference (asserted first), so the device cannot pass on the wrong order."""
    N, R, nb = 16384, 2, 8
    H = N - N // R
    x = signal(nb * H, 60)
    g = np.full(len(BANK), g1, np.float32)
    p = G.Pipeline(N, R, BANK, max_blocks=nb)
    y, _l, _d = run(p, lambda: p.work(x), None)
    comps = np.concatenate([v.view(np.float32) for v in y])
    assert comps.size >= 10 ** 5
    scale = float(np.float32(8000.0 / (abs(float(g[0])) * float(comps.std()))))
    right = wanted(y, g, "sc16", scale)
    wrong = [narrowed(v, float(np.float32(g[0]) * np.float32(scale)), np.int16) for v in y]
    ndiff = sum(int(np.count_nonzero(a != b)) for a, b in zip(right, wrong))
    print("g = %r, scale = %r: the two orders differ in %d of %d components" % (float(g[0]), scale, ndiff, comps.size))
    assert ndiff >= 1
    got, _l, d = run(p, lambda: p.work(x), g, "sc16", scale)
    for c, (u, v) in enumerate(zip(got, right)):
        same_bytes(u, v, "ch%d" % c)
    assert "gains: with the narrowing" in d, d


# ---- B3. the levels' one order ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [-3, 1, 5])
@pytest.mark.parametrize("N,chans", [(8192, MIXED), (16384, BANK)], ids=["mixed, N = 8192", "bank, N = 16384"])
def test_levels_under_a_power_of_two_are_the_scaled_levels(N, chans, k):
    """g = 2^k on every channel commutes with every rounding: the levels must be the gains-off levels times (4^k, 2^k), bit for bit, which pins the
    summation order of each of the three routes to k_chan_levels' (and k_fine_rotate<true>'s)"""
    R, nb = 2, 5
    H = N - N // R
    x = signal(nb * H, 61)
    g = np.full(len(chans), 2.0 ** k, np.float32)
    factor = np.array([4.0 ** k, 2.0 ** k], np.float32)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    call = lambda: p.work(x)
    for fine in (False, True):
        p.set_fine_tuning(edge_nus(len(chans), 2) if fine else None)
        y, l0, d0 = run(p, call, None, levels=True)
        scale = int_scale(wanted(y, g), np.int16)
        for fmt, route in ((None, "pass"), ("sc16", "with the narrowing")):
            _y, _got, lev, d = checked(p, call, g, "2^%d, fine %s, %s" % (k, fine, fmt), fmt, scale, levels=True, y=y)
            same_bytes(lev, l0 * factor, "2^%d, fine %s, %s: the levels" % (k, fine, fmt))
            if not FORCED:
                assert ("gains: " + ("with the rotation" if fine else route)) in d, d
                assert ("levels: " + ("with the rotation" if fine else "with the gains")) in d, d
    p.set_fine_tuning(None)


# ---- B4. cuts of the stream ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["float", "sc16"])
@pytest.mark.parametrize("N,R,chans,flags", [(4096, 2, EXAMPLE, 0), (8192, 4, TINY, 0), (16384, 2, BANK, 0), (4096, 2, EXAMPLE, G.FDC_PIPE_NO_FUSED)],
                         ids=["path 5", "tiny rows at odd offsets", "bank", "example plan, spectrum path"])
def test_cuts_of_the_stream_give_the_same_bytes(N, R, chans, flags, fmt):
    """7 blocks as 7, as 3 + 4 and as 1 + 1 + 5, and on a handle with another chunk_blocks and host_sub_blocks: outputs and levels"""
    nb = 7
    H = N - N // R
    x = signal(nb * H, 2)
    g = draw_gains(len(chans), 5)
    one = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    y, _l, _d = run(one, lambda: one.work(x), None)
    scale = int_scale(wanted(y, g), np.int16) if fmt else 1.0
    _y, whole, lw, _d = checked(one, lambda: one.work(x), g, "7 blocks", fmt, scale, levels=True, y=y)
    for cut in ((3, 4), (1, 1, 5)):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
        p.set_gains(g)
        p.set_levels(True)
        p.set_output_format(fmt, scale)
        parts, levs, b0 = [[] for _ in chans], [], 0
        for n in cut:
            for c, o in enumerate(p.work(x[b0 * H:(b0 + n) * H])):
                parts[c].append(o)
            levs.append(p.levels())
            b0 += n
        for c in range(len(chans)):
            same_bytes(np.concatenate(parts[c]), whole[c], "cut %r ch%d" % (cut, c))
        same_bytes(np.concatenate(levs), lw, "cut %r: the levels" % (cut,))
    p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags, chunk_blocks=2, host_sub_blocks=3)
    assert p.chunk_blocks() == 2
    p.set_gains(g)
    p.set_levels(True)
    p.set_output_format(fmt, scale)
    for c, (u, v) in enumerate(zip(p.work(x), whole)):
        same_bytes(u, v, "chunk_blocks 2, host_sub_blocks 3, ch%d" % c)
    same_bytes(p.levels(), lw, "chunk_blocks 2, host_sub_blocks 3: the levels")


# ---- B5. call forms --------------------------------------------------------------------------------------------------------------------------------------

FORMS = [("mixed, N = 8192", 8192, MIXED), ("bank, N = 16384", 16384, BANK), ("example, N = 4096", 4096, EXAMPLE)]
form_ids = [f[0] for f in FORMS]


@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["float", "sc16"])
@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_registered_outputs_and_ragged_calls(k, registered, fmt):
    """calls of 1, 7, 3 and 5 blocks in sub-batches of 2 (pageable outputs, or registered ones through k_scatter_out / k_scatter_oq, which narrows itself:
    the gain pass stays float there): the stream of one call of 16 blocks on a second handle"""
    _name, N, chans = FORMS[k]
    R, mb, sizes = 2, 7, (1, 7, 3, 5)
    H = N - N // R
    x = signal(sum(sizes) * H, 300 + k)
    g = draw_gains(len(chans), 10 + k)
    one = G.Pipeline(N, R, chans, max_blocks=sum(sizes))
    y, _l, _d = run(one, lambda: one.work(x), None)
    scale = int_scale(wanted(y, g), np.int16) if fmt else 1.0
    _y, want, lw, _d = checked(one, lambda: one.work(x), g, "one call of 16 blocks", fmt, scale, levels=True, y=y)
    p = G.Pipeline(N, R, chans, max_blocks=mb, host_sub_blocks=2)
    p.set_gains(g)
    p.set_levels(True)
    p.set_output_format(fmt, scale)
    bufs = [np.zeros((mb * lo, 2) if fmt else mb * lo, np.int16 if fmt else np.complex64) for lo in p.lout]
    if registered:
        for b in bufs:
            G.register_host(b)
    try:
        pieces, levs, b0 = [[] for _ in chans], [], 0
        for n in sizes:
            outs = [b[:n * lo] for b, lo in zip(bufs, p.lout)]
            p.work(x[b0 * H:(b0 + n) * H], outs=outs)
            levs.append(p.levels())
            for c, o in enumerate(outs):
                pieces[c].append(o.copy())
            b0 += n
    finally:
        if registered:
            for b in bufs:
                G.unregister_host(b)
    for c in range(len(chans)):
        same_bytes(np.concatenate(pieces[c]), want[c], "ragged stream ch%d" % c)
    same_bytes(np.concatenate(levs), lw, "ragged stream: the levels")
    d = p.describe()
    assert ("gains: " + ("with the narrowing" if fmt and not registered else "pass")) in d, d
    assert not fmt or "output sc16: narrowed" in d, d


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_real_and_integer_input(k):
    _name, N, chans = FORMS[k]
    R, nb = 2, 5
    H = N - N // R
    xr = signal(nb * H, 320 + k).real.copy()
    xi = iq(nb * H, np.int16, 33)
    g = draw_gains(len(chans), 20 + k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    checked(p, lambda: p.work_real(xr), g, "work_real")
    y, _got, _l, d = checked(p, lambda: p.work_iq(xi, scale=2.0 ** -12), g, "work_iq", levels=True)
    scale = int_scale(wanted(y, g), np.int8)
    checked(p, lambda: p.work_iq(xi, scale=2.0 ** -12), g, "work_iq, sc8 out", "sc8", scale, y=y)


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_span_entries_far_into_the_stream(k):
    _name, N, chans = FORMS[k]
    R, nb, first = 2, 4, 2 ** 40 + 3
    H, ovl = N - N // R, N // R
    x, halo = signal(nb * H, 330 + k), signal(ovl, 24)
    xi, hi = iq(nb * H, np.int16, 31), iq(ovl, np.int16, 32)
    g = draw_gains(len(chans), 30 + k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    p.set_fine_tuning(edge_nus(len(chans), 1))                             # (the phase depends on first_block: the gain comes behind it)
    checked(p, lambda: work_span(p, halo, x, first, nb), g, "work_span at block 2^40 + 3", levels=True)
    checked(p, lambda: p.work_span_iq(hi, xi, first, scale=2.0 ** -12), g, "work_span_iq at block 2^40 + 3")


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_device_entries_on_a_stream_of_the_caller(k):
    """process_device and process_device_iq at first_block = 13, float and sc16 output (the device entries narrow on the device: with the narrowing),
    levels from fdc_pipeline_levels.  Gains add no max_blocks rule: a float call above max_blocks is served."""
    _name, N, chans = FORMS[k]
    R, nb, first = 2, 4, 13
    H, ovl = N - N // R, N // R
    g = draw_gains(len(chans), 40 + k)
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
                def out(fmt=None):
                    call()
                    assert dev.hip.hipStreamSynchronize(st) == 0
                    if fmt:
                        return by_channel(p, dev.get(d_o, 2 * n_out, np.int16).reshape(-1, 2), nb)
                    return by_channel(p, dev.get(d_o, n_out, np.complex64), nb)
                y = out()
                scale = int_scale(wanted(y, g), np.int16)
                p.set_gains(g)
                p.set_levels(True)
                got = out()
                lev, d = p.levels(), p.describe()
                p.set_output_format("sc16", scale)
                goti = out("sc16")
                levi, di = p.levels(), p.describe()
                p.set_output_format(None)
                p.set_levels(False)
                p.set_gains(None)
                for c in range(len(chans)):
                    same_bytes(got[c], gained(y[c], g[c]), "%s ch%d" % (what, c))
                    same_bytes(goti[c], narrowed(gained(y[c], g[c]), scale, np.int16), "%s, sc16, ch%d" % (what, c))
                gained_levels_hold(p, y, g, lev, what)
                same_bytes(levi, lev, what + ", sc16: the levels")
                assert "gains: pass" in d and "gains: with the narrowing" in di and "levels: with the gains" in di, (d, di)
            big = dev.put(np.zeros(ovl + 2 * nb * H, np.complex64))
            d_big = dev.put(np.zeros(p.output_samples(2 * nb), np.complex64))
            p.set_gains(g)
            p.process_device(big, 0, 2 * nb, d_big)
            p.synchronize()
            p.set_gains(None)
        finally:
            dev.hip.hipStreamDestroy(st)


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_outputs_that_are_not_wanted(k):
    """outs[c] = NULL for some channels and for all of them: the wanted ones are gained, the levels complete"""
    _name, N, chans = FORMS[k]
    R, nb = 2, 5
    H = N - N // R
    x = signal(nb * H, 310 + k)
    g = draw_gains(len(chans), 50 + k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    _y, full, lw, _d = checked(p, lambda: p.work(x), g, "every output", levels=True)
    p.set_gains(g)
    p.set_levels(True)
    lib = _lib.lib()
    for keep in ([c % 2 == 0 for c in range(len(chans))], [False] * len(chans)):
        p.reset()
        outs = [np.zeros(nb * lo, np.complex64) for lo in p.lout]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data if kp else None for o, kp in zip(outs, keep)])
        assert lib.fdc_pipeline_work(p._h, x.ctypes.data, nb, ptrs, None) == nb
        same_bytes(p.levels(nb), lw, "outputs kept: %r" % keep)
        for c, kp in enumerate(keep):
            same_bytes(outs[c], full[c] if kp else np.zeros_like(full[c]), "ch%d" % c)


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_group_of_two_virtual_members_against_one_handle(k):
    _name, N, chans = FORMS[k]
    R, nb = 2, 8
    H = N - N // R
    x = signal(2 * nb * H, 350 + k)
    g1, g2 = draw_gains(len(chans), 60 + k), draw_gains(len(chans), 70 + k)
    grp = G.PipelineGroup(N, R, chans, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    q = G.Pipeline(N, R, chans, max_blocks=nb)
    for h in (grp, p):
        h.set_levels(True)
    for j, (n, g) in enumerate(((nb, g1), (5, g2))):                       # 5 blocks: spans of 3 and 2; other gains for the second call
        grp.set_gains(g)
        p.set_gains(g)
        xs = x[j * nb * H:(j * nb + n) * H]
        a, b, y = grp.work(xs), p.work(xs), q.work(xs)
        assert sum(m > 0 for _f, m in grp.last_spans()) == 2
        for c in range(len(chans)):
            same_bytes(a[c], b[c], "call %d ch%d: the group against one handle" % (j, c))
            same_bytes(a[c], gained(y[c], g[c]), "call %d ch%d" % (j, c))
        same_bytes(grp.levels(), p.levels(), "call %d: the group's levels against one handle's" % j)
        for i in range(grp.size()):
            out = np.zeros(len(chans), np.float32)
            assert _lib.lib().fdc_pipeline_gains(_lib.lib().fdc_pipeline_group_member(grp._h, i), out.ctypes.data_as(C.POINTER(C.c_float)), len(chans)) == 0
            same_bytes(out, g, "member %d" % i)
    with pytest.raises(ValueError):
        grp.set_gains(g1[:-1])
    assert raw_set(grp._h, g1, len(chans) + 1, _lib.lib().fdc_pipeline_group_set_gains) == -1
    assert raw_set(None, g1, len(chans), _lib.lib().fdc_pipeline_group_set_gains) == -1


# ---- B6. rows that are not finite ------------------------------------------------------------------------------------------------------------------------

def test_a_row_of_nan_disturbs_no_other_row():
    """an input sample of NaN reaches the blocks that overlap it; every other row has the bytes it has without it, and the rows it reaches are NaN where
    the gains-off output is (also under a gain of zero: 0 * NaN)"""
    N, R, nb = 8192, 2, 6
    H = N - N // R
    x = signal(nb * H, 9)
    bad = x.copy()
    bad[4 * H + 100] = complex(np.nan, 1.0)
    g = np.array([-3.25, 0.0], np.float32)
    p = G.Pipeline(N, R, MIXED, max_blocks=nb)
    clean, lc, _d = run(p, lambda: p.work(x), g, levels=True)
    y, _l, _d = run(p, lambda: p.work(bad), None)
    got, lev, _d = run(p, lambda: p.work(bad), g, levels=True)
    hit = np.array([[not np.isfinite(o[m * lo:(m + 1) * lo]).all() for o, lo in zip(y, p.lout)] for m in range(nb)])
    assert hit.any() and not hit.all()
    for c, lo in enumerate(p.lout):
        u, v, w = (a[c].view(np.float32).reshape(nb, -1) for a in (got, clean, y))
        same_bytes(u[~hit[:, c]], v[~hit[:, c]], "the rows without a NaN, ch%d" % c)
        assert (np.isnan(u) == np.isnan(w)).all(), c
        fin = ~np.isnan(w)
        same_bytes(u[fin], gained(y[c], g[c]).view(np.float32).reshape(nb, -1)[fin], "the finite components, ch%d" % c)
    same_bytes(lev[~hit], lc[~hit], "the levels of the rows without a NaN")
    assert np.isnan(lev[hit][:, 0]).all()


# ---- B7. no allocation in the steady state ---------------------------------------------------------------------------------------------------------------

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
po = G.Pipeline(8192, 2, MIXED, max_blocks=nb)
pd = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
po.set_output_format("sc16", 100.0)
po.set_fine_tuning([0.1, -0.2])
pd.set_output_format("sc8", 10.0)
for h in (p, po, pd, g):
    h.set_levels(True)
d_ring, d_out = C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(8 * pd.output_samples(nb))) == 0
k = [0]
def agc(h, n):
    k[0] += 1
    h.set_gains(np.linspace(0.5, 3.0, n) + 0.01 * (k[0] % 7))            # new gains before every call
entries = {"fdc_pipeline_work (host entry, path 5)": lambda: (agc(p, 4), p.work(x), p.levels()),
           "fdc_pipeline_work (fine tuning, sc16 out)": lambda: (agc(po, 2), po.work(x2), po.levels()),
           "fdc_pipeline_process_device (sc8 out)": lambda: (agc(pd, 4), pd.process_device(d_ring, 5, nb, d_out), pd.levels()),
           "fdc_pipeline_group_work": lambda: (agc(g, 4), g.work(x), g.levels()),
           "off and on again": lambda: (p.set_gains(None), agc(p, 4), p.work(x))}
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
assert "gains: pass" in p.describe() and "gains: with the rotation" in po.describe() and "gains: with the narrowing" in pd.describe(), (p.describe(), po.describe(), pd.describe())
assert not bad, bad
print("OK")
'''


def test_no_allocation_in_the_steady_state(tmp_path):
    shim = str(tmp_path / "libhipcount.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hip_alloc_counter.c"), "-o", shim,
                           "-ldl", "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([sys.executable, "-c", NO_ALLOC_CHILD, shim, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


# ---- B8. the hier block ----------------------------------------------------------------------------------------------------------------------------------

KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05], [-0.2, 0.1], [0.31, 0.02]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False, max_blocks=6)


def test_hier_block():
    N, R, nb = 4096, 2, 6
    H = N - N // R
    x = signal(2 * nb * H, 11)
    g, g2 = np.array([2.5, -0.125, 0.0], np.float32), np.array([1.0, 3.0, -7.5], np.float32)
    on = G.FrequencyDomainChannelizer(inptype=8, gains=g, levels=True, **KW)
    off = G.FrequencyDomainChannelizer(inptype=8, **KW)
    assert off.gains is None
    same_bytes(on.pipeline.gains(), g, "the handle's gains")
    ya, yb = on.work(x[:nb * H]), off.work(x[:nb * H])
    for c, (u, v) in enumerate(zip(ya, yb)):
        same_bytes(u, gained(v, g[c]), "port %d" % c)
    gained_levels_hold(on.pipeline, yb, g, on.levels, "hier block")
    # set_gains between two work() calls: the stream goes on
    on.set_gains(g2)
    ya, yb = on.work(x[nb * H:]), off.work(x[nb * H:])
    for c, (u, v) in enumerate(zip(ya, yb)):
        same_bytes(u, gained(v, g2[c]), "port %d, second call" % c)
    with pytest.raises(ValueError):
        on.set_gains([1.0, 2.0])
    with pytest.raises(ValueError):
        on.set_gains([1.0, 2.0, np.nan])
    same_bytes(on.pipeline.gains(), g2, "after the refusals")
    on.set_gains(None)
    assert on.gains is None and on.pipeline.gains().tolist() == [1.0, 1.0, 1.0]
    # a block built without gains takes them later
    off.set_gains(g)
    same_bytes(off.pipeline.gains(), g, "set_gains on a block built without")
    # together with fine_tuning and iq_output: the ports are the narrowed gained ports of a block without iq_output
    fine = G.FrequencyDomainChannelizer(inptype=8, fine_tuning=True, **KW)
    yf = fine.work(x[:nb * H])
    scale = int_scale(wanted(yf, g), np.int16)
    both = G.FrequencyDomainChannelizer(inptype=8, gains=g, fine_tuning=True, iq_output="sc16", iq_output_scale=scale, **KW)
    for c, (u, v) in enumerate(zip(both.work(x[:nb * H]), yf)):
        same_bytes(u, narrowed(gained(v, g[c]), scale, np.int16), "port %d, fine tuning and sc16" % c)
    # two devices
    kw = dict(KW, max_blocks=12)
    grp = G.FrequencyDomainChannelizer(inptype=8, gains=g, devices=[0, 0], **kw)
    one = G.FrequencyDomainChannelizer(inptype=8, **kw)
    assert isinstance(grp.pipeline, G.PipelineGroup)
    for c, (u, v) in enumerate(zip(grp.work(x), one.work(x))):
        same_bytes(u, gained(v, g[c]), "devices=[0, 0], port %d" % c)
