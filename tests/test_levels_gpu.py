"""GPU tests (-m gpu) of the channel levels (fdc_pipeline_set_levels, fdc_pipeline_levels, fdc_pipeline_levels_device and the group's two entries;
include/fdc_amd.h): the setting's semantics, the refusals, the one-order rule, every call form, no allocation in the steady state, the hier block.
tests/test_levels_routes_gpu.py covers every plan and the inside of the two kernels.

Every comparison is against the numpy model (tests/test_levels_cpu.py: model, agrees) applied to the float32 outputs of THE SAME call:
|power - P64| <= (lout + 8) 2^-24 P64 with P64 the float64 sum of squares of those samples (a term has at most three roundings; any-order float32
summation of n non-negative terms is within (n - 1) 2^-24 / (1 - (n - 1) 2^-24): DESIGN.md "Channel levels"), and peak bit-equal to np.fmax.reduce over
the absolute values of their components.  The channel outputs themselves must be byte-equal to the same handle's outputs with levels off."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from test_fine_tuning_gpu import BANK, FORCED, MIXED, narrowed, signal, work_span
from test_fine_tuning_routes_gpu import TINY, DeviceBuffers, by_channel, int_scale
from test_iq_input_gpu import EXAMPLE, iq, same_bytes
from test_levels_cpu import agrees, model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def levels_hold(p, outs, lev, what):
    """the model on every channel of one call: outs = the float32 outputs the call returned, lev = its levels"""
    nb = outs[0].size // p.lout[0] if outs else 0
    assert lev.shape == (nb, len(p.lout), 2) and lev.dtype == np.float32, (what, lev.shape)
    for c, y in enumerate(outs):
        agrees(lev[:, c], y, p.lout[c], "%s ch%d" % (what, c))
    assert all(np.abs(y).max() > 0 for y in outs), what


def on_and_off(p, call):
    """call() from block 0 of handle p with levels on, its levels and describe() behind it, and call() again with levels off"""
    p.reset()
    p.set_levels(True)
    got = call()
    lev, d = p.levels(), p.describe()
    p.set_levels(False)
    p.reset()
    plain = call()
    assert "levels: " in d and "levels" not in p.describe(), (d, p.describe())
    return got, lev, d, plain


def checked(p, call, what):
    """on_and_off, the outputs byte-equal to levels off, the model on the levels; returns (outputs, levels, describe)"""
    got, lev, d, plain = on_and_off(p, call)
    for c, (u, v) in enumerate(zip(got, plain)):
        same_bytes(u, v, "%s: outputs with levels on against off, ch%d" % (what, c))
    levels_hold(p, got, lev, what)
    return got, lev, d


def raw_levels(h, nblocks, nchan, fn=None):
    """the C entry's status and what it wrote (a buffer of NaN where it wrote nothing)"""
    out = np.full((max(nblocks, 0), nchan, 2), np.nan, np.float32)
    rc = (fn or _lib.lib().fdc_pipeline_levels)(h, out.ctypes.data_as(C.POINTER(C.c_float)), nblocks)
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
    # off by default: no levels, no device buffer, no line in describe; before any call and with a wrong count the accessor refuses
    assert p.levels_device() is None and "levels" not in p.describe()
    a0 = p.work(x[:nb * H])
    assert raw_levels(p._h, nb, len(chans))[0] == -1                       # levels are off
    p.set_levels(True)
    assert p.levels_device() is not None
    rc, out = raw_levels(p._h, nb, len(chans))
    assert rc == -1 and np.isnan(out).all()                                # on, but no call yet
    a1 = p.work(x[nb * H:2 * nb * H])
    for bad in (nb - 1, nb + 1, 0, -1):
        rc, out = raw_levels(p._h, bad, len(chans))
        assert rc == -1 and np.isnan(out).all(), bad
    l1 = p.levels()
    levels_hold(p, a1, l1, "second call")
    # a call of no blocks leaves the previous result in place
    assert p.work(x[:0]) is not None
    same_bytes(p.levels(nb), l1, "after a call of no blocks")
    # it does not touch the stream: the third call continues it; the setting survives reset()
    a2 = p.work(x[2 * nb * H:])
    levels_hold(p, a2, p.levels(), "third call")
    for k, a in enumerate((a0, a1, a2)):
        for c in range(len(chans)):
            same_bytes(a[c], plain[k][c], "call %d ch%d against a handle that never had levels" % (k, c))
    p.reset()
    assert p.levels_device() is not None
    b0 = p.work(x[:nb * H])
    levels_hold(p, b0, p.levels(), "after reset()")
    for c in range(len(chans)):
        same_bytes(b0[c], plain[0][c], "after reset(), ch%d" % c)
    # switched off and on again: the old result is gone
    dev = p.levels_device()
    p.set_levels(False)
    assert p.levels_device() is None and raw_levels(p._h, nb, len(chans))[0] == -1
    p.set_levels(True)
    assert p.levels_device() == dev                                        # allocated once
    assert raw_levels(p._h, nb, len(chans))[0] == -1
    assert lib.fdc_pipeline_set_levels(None, 1) == -1 and lib.fdc_pipeline_levels(None, None, nb) == -1


def test_no_channels():
    """C = 0: on is accepted and every result is empty"""
    N, R, nb = 4096, 2, 3
    H = N - N // R
    p = G.Pipeline(N, R, [], max_blocks=nb, keep_spectrum=True)
    p.set_levels(True)
    outs, spec = p.work(signal(nb * H, 1), want_spectrum=True)
    assert outs == [] and np.abs(spec).max() > 0
    lev = p.levels()
    assert lev.shape == (nb, 0, 2)
    assert _lib.lib().fdc_pipeline_levels(p._h, None, nb) == 0 and _lib.lib().fdc_pipeline_levels(p._h, None, nb + 1) == -1


def test_refused_while_a_pipelined_sinks_batch_is_inside():
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x = signal(nb * H, 7)
    kw = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01, max_blocks=nb)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, lookahead=True, **kw)
    p.work(x, sinks=bank)
    with pytest.raises(G.FdcError) as e:
        p.set_levels(True)
    assert e.value.status == -1 and p.levels_device() is None
    while p.flush_sinks(bank) > 0:
        pass
    p.set_levels(True)                                                     # nothing inside any more
    assert p.levels_device() is not None
    # ... and the same refusal leaves a handle that had levels before as it is: off
    p.set_levels(False)
    p.work(x, sinks=bank)
    assert _lib.lib().fdc_pipeline_set_levels(p._h, 1) == -1 and p.levels_device() is None
    while p.flush_sinks(bank) > 0:
        pass


def test_entries_that_give_no_levels_are_refused():
    """work_sinks, work_spectrum, process_device_power and work_waterfall return FDC_ERR_INVALID_ARGUMENT and leave history and block counter untouched:
    the next work continues the stream bit for bit"""
    N, R, nb = 4096, 2, 3
    H, ovl = N - N // R, N // R
    x = signal(2 * nb * H, 7)
    kw = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01, max_blocks=nb)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    q = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, **kw)
    w = G.Waterfall(N, 1e6, R, 1, 0, -100.0, 0.0, 0, 0, max_items=nb)
    spec_items = np.zeros(nb * N, np.complex64)
    with DeviceBuffers() as dev:
        d_ring, d_out = dev.put(np.zeros(ovl + nb * H, np.complex64)), dev.put(np.zeros(p.output_samples(nb), np.complex64))
        d_spec, d_pow = dev.put(np.zeros(nb * N, np.complex64)), dev.put(np.zeros(nb * N // 16, np.float32))
        entries = [("work(sinks=)", lambda: p.work(x[nb * H:], sinks=bank)),
                   ("work_spectrum", lambda: p.work_spectrum(spec_items)),
                   ("work_waterfall", lambda: p.work_waterfall(x[nb * H:], w)),
                   ("process_device(d_group_power=)", lambda: p.process_device(d_ring, 0, nb, d_out, d_spectrum=d_spec, d_group_power=d_pow))]
        p.set_levels(True)
        a0, b0 = p.work(x[:nb * H]), q.work(x[:nb * H])
        l0 = p.levels()
        for name, call in entries:
            with pytest.raises(G.FdcError) as e:
                call()
            assert e.value.status == -1 and "levels" in str(e.value), name
        same_bytes(p.levels(nb), l0, "the levels of the last successful call")
        a1, b1 = p.work(x[nb * H:]), q.work(x[nb * H:])
        for c in range(len(EXAMPLE)):
            same_bytes(a0[c], b0[c], "before the refusals, ch%d" % c)
            same_bytes(a1[c], b1[c], "after the refusals, ch%d" % c)
        levels_hold(p, a1, p.levels(), "after the refusals")
        p.set_levels(False)
        for name, call in entries:
            call()                                            # they work again
        p.synchronize()


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
    one.set_levels(True)
    whole = one.work(x)
    lw = one.levels()
    levels_hold(one, whole, lw, "7 blocks")
    for cut in ((3, 4), (1, 1, 5)):
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
        p.set_levels(True)
        parts, b0 = [], 0
        for n in cut:
            outs = p.work(x[b0 * H:(b0 + n) * H])
            lev = p.levels()
            levels_hold(p, outs, lev, "%r: the call at block %d" % (cut, b0))
            parts.append(lev)
            b0 += n
        same_bytes(np.concatenate(parts), lw, "cut %r" % (cut,))
    p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags, chunk_blocks=2, host_sub_blocks=3)
    assert p.chunk_blocks() == 2
    p.set_levels(True)
    outs = p.work(x)
    for c, (u, v) in enumerate(zip(outs, whole)):
        same_bytes(u, v, "chunk_blocks 2, host_sub_blocks 3, ch%d" % c)
    same_bytes(p.levels(), lw, "chunk_blocks 2, host_sub_blocks 3")
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
            lev = p.levels()
            got = by_channel(p, dev.get(d_o, n_out, np.complex64), n)
            for c, (u, v) in enumerate(zip(got, whole)):
                same_bytes(u, v[first * p.lout[c]:(first + n) * p.lout[c]], "process_device at block %d, ch%d" % (first, c))
            same_bytes(lev, lw[first:first + n], "process_device at block %d" % first)
            # the same through the device buffer, read ordered on the call's stream
            same_bytes(dev.get(C.c_void_p(p.levels_device()), n * len(chans) * 2, np.float32).reshape(n, len(chans), 2), lev, "levels_device")


MERGED_CHILD = r'''
import os, sys
os.environ["FDC_DEBUG_ENV"] = "1"
os.environ["FDC_LEVELS_SEPARATE"] = sys.argv[3]
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import gr_fdc_amd as G
from test_fine_tuning_routes_gpu import TINY, edge_nus
rng = np.random.default_rng(5)
res = {}
for name, N, R, chans in (("tiny", 8192, 4, TINY), ("bank", 16384, 2, [(256 * c, 256, 0.88, 1.0) for c in range(64)])):
    nb = 5
    H = N - N // R
    x = (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H)).astype(np.complex64)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb)
    p.set_fine_tuning(edge_nus(len(chans), 3))
    p.set_levels(True)
    outs = p.work(x)
    res[name + "_levels"] = p.levels()
    res[name + "_route"] = np.array(p.describe())
    for c, o in enumerate(outs):
        res["%s_out%d" % (name, c)] = o
np.savez(sys.argv[2], **res)
print("OK")
'''


def test_the_merged_route_gives_the_bits_of_the_separate_pass(tmp_path):
    """Fine tuning and levels on, off path 5: k_fine_rotate<true> reduces the turned samples it holds.  A second process with the library's debug switch
    FDC_LEVELS_SEPARATE=1 (honoured under FDC_DEBUG_ENV=1, read when the setting is switched on) runs k_fine_rotate<false>, then k_chan_levels over the same
    y': the same outputs and the same levels, bit for bit — rows of 1, 15, 8, 240, 2 and 960 samples on both access widths, and a bank."""
    got = {}
    for sep in ("0", "1"):
        path = str(tmp_path / ("sep%s.npz" % sep))
        r = subprocess.run([sys.executable, "-c", MERGED_CHILD, ROOT, path, sep], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
        got[sep] = np.load(path)
    assert set(got["0"].files) == set(got["1"].files)
    for k in got["0"].files:
        if k.endswith("_route"):
            continue
        same_bytes(got["0"][k], got["1"][k], k)
        assert np.isfinite(got["0"][k]).all() and np.abs(got["0"][k]).max() > 0, k
    if not FORCED:
        for name in ("tiny", "bank"):
            assert "levels: with the rotation" in str(got["0"][name + "_route"]), got["0"][name + "_route"]
            assert "levels: pass" in str(got["1"][name + "_route"]) and "fine tuning: rotated" in str(got["1"][name + "_route"]), got["1"][name + "_route"]


# ---- call forms ----------------------------------------------------------------------------------------------------------------------------------------

FORMS = [("mixed, N = 8192", 8192, MIXED), ("bank, N = 16384", 16384, BANK), ("example, N = 4096", 4096, EXAMPLE)]
form_ids = [f[0] for f in FORMS]


@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["float", "sc16"])
@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("sub", [0, 2], ids=["one sub-batch", "sub-batches of 2"])
@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_sub_batches_registered_outputs_and_ragged_calls(k, sub, registered, fmt):
    """calls of 1, 7, 3 and 5 blocks (host sub-batches; pageable outputs or registered ones through k_scatter_out / k_scatter_oq): outputs and levels are
    those of one call of 16 blocks on a second handle, which holds the model"""
    _name, N, chans = FORMS[k]
    R, mb, sizes = 2, 7, (1, 7, 3, 5)
    H = N - N // R
    x = signal(sum(sizes) * H, 300 + k)
    one = G.Pipeline(N, R, chans, max_blocks=sum(sizes))
    yf, lw, _d = checked(one, lambda: one.work(x), "one call of 16 blocks")
    dt = np.int16 if fmt else np.complex64
    scale = int_scale(yf, np.int16) if fmt else 1.0
    p = G.Pipeline(N, R, chans, max_blocks=mb, host_sub_blocks=sub or None)
    p.set_levels(True)
    if fmt:
        p.set_output_format(fmt, scale)
    bufs = [np.zeros((mb * lo, 2) if fmt else mb * lo, dt) for lo in p.lout]
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
        want = narrowed(yf[c], scale, np.int16) if fmt else yf[c]
        same_bytes(np.concatenate(pieces[c]), want, "ragged stream ch%d" % c)
    same_bytes(np.concatenate(levs), lw, "ragged stream: levels")
    d = p.describe()
    assert "levels: pass" in d and (not fmt or "output sc16: narrowed" in d), d


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_outputs_that_are_not_wanted(k):
    """outs[c] = NULL for some channels, and for all of them (a call that only watches the band): the levels are still complete"""
    _name, N, chans = FORMS[k]
    R, nb = 2, 5
    H = N - N // R
    x = signal(nb * H, 310 + k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    full, lw, _d = checked(p, lambda: p.work(x), "every output")
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
def test_real_input(k):
    _name, N, chans = FORMS[k]
    R, nb = 2, 5
    H = N - N // R
    xr = signal(nb * H, 320 + k).real.copy()
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    checked(p, lambda: p.work_real(xr), "work_real")


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_span_entries_far_into_the_stream(k):
    """work_span and work_span_iq at first_block = 2^40 + 3: the levels' row index is the block of the CALL"""
    _name, N, chans = FORMS[k]
    R, nb, first = 2, 4, 2 ** 40 + 3
    H, ovl = N - N // R, N // R
    x, halo = signal(nb * H, 330 + k), signal(ovl, 24)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    p.set_levels(True)
    got = work_span(p, halo, x, first, nb)
    lev = p.levels(nb)
    p.set_levels(False)
    for c, (u, v) in enumerate(zip(got, work_span(p, halo, x, first, nb))):
        same_bytes(u, v, "work_span, levels on against off, ch%d" % c)
    levels_hold(p, got, lev, "work_span at block 2^40 + 3")
    p.reset()
    p.set_levels(True)
    xi, hi = iq(nb * H, np.int16, 31), iq(ovl, np.int16, 32)
    gi = p.work_span_iq(hi, xi, first, scale=2.0 ** -12)
    levels_hold(p, gi, p.levels(), "work_span_iq at block 2^40 + 3")


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_device_entries(k):
    """process_device and process_device_iq at first_block = 13 on a stream of the caller's: the levels come from fdc_pipeline_levels (which synchronises
    that stream) and from the device buffer.  Above max_blocks a device call with levels is refused and nothing is enqueued."""
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
                    lev = p.levels() if p.levels_device() is not None else None      # (synchronises the call's stream)
                    assert dev.hip.hipStreamSynchronize(st) == 0
                    return by_channel(p, dev.get(d_o, n_out, np.complex64), nb), lev
                p.set_levels(True)
                got, lev = run()
                d = p.describe()
                same_bytes(dev.get(C.c_void_p(p.levels_device()), nb * len(chans) * 2, np.float32).reshape(nb, len(chans), 2), lev, what + ": the device buffer")
                p.set_levels(False)
                plain, _ = run()
                for c, (u, v) in enumerate(zip(got, plain)):
                    same_bytes(u, v, "%s, levels on against off, ch%d" % (what, c))
                levels_hold(p, got, lev, what)
                assert "levels: pass" in d, d
            # above max_blocks: refused with levels on (nothing is enqueued: the output stays as it is), served without
            big = dev.put(np.zeros(ovl + 2 * nb * H, np.complex64))
            d_big = dev.put(np.full(p.output_samples(2 * nb), 7, np.complex64))
            p.set_levels(True)
            with pytest.raises(G.FdcError) as e:
                p.process_device(big, 0, 2 * nb, d_big)
            assert e.value.status == -1
            p.synchronize()
            assert (dev.get(d_big, p.output_samples(2 * nb), np.complex64) == 7).all()
            p.set_levels(False)
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
    rc, out = raw_levels(g._h, nb, len(chans), lib.fdc_pipeline_group_levels)
    assert rc == -1 and np.isnan(out).all()                               # before any call
    g.set_levels(True)
    p.set_levels(True)
    assert raw_levels(g._h, nb, len(chans), lib.fdc_pipeline_group_levels)[0] == -1
    for j, n in enumerate((nb, 5)):                                        # 5 blocks: spans of 3 and 2
        a, b = g.work(x[j * nb * H:(j * nb + n) * H]), p.work(x[j * nb * H:(j * nb + n) * H])
        for c, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, "call %d ch%d" % (j, c))
        assert sum(m > 0 for _f, m in g.last_spans()) == 2
        lg = g.levels()
        same_bytes(lg, p.levels(), "call %d: the group's levels against one handle's" % j)
        levels_hold(p, a, lg, "group call %d" % j)
        assert raw_levels(g._h, n + 1, len(chans), lib.fdc_pipeline_group_levels)[0] == -1
    g.set_levels(False)
    assert raw_levels(g._h, 5, len(chans), lib.fdc_pipeline_group_levels)[0] == -1
    assert lib.fdc_pipeline_group_set_levels(None, 1) == -1 and lib.fdc_pipeline_group_levels(None, None, 1) == -1


# ---- rows that are not finite -------------------------------------------------------------------------------------------------------------------------

def test_rows_that_are_not_finite_disturb_no_other_row():
    """an input sample of NaN reaches the blocks that overlap it; every other row has the bits it has without it"""
    N, R, nb = 8192, 2, 6
    H = N - N // R
    x = signal(nb * H, 9)
    p = G.Pipeline(N, R, MIXED, max_blocks=nb)
    p.set_levels(True)
    clean = p.work(x)
    lc = p.levels()
    bad = x.copy()
    bad[4 * H + 100] = complex(np.nan, 1.0)
    p.reset()
    outs = p.work(bad)
    lev = p.levels()
    hit = np.array([[not np.isfinite(o[m * lo:(m + 1) * lo]).all() for o, lo in zip(outs, p.lout)] for m in range(nb)])
    assert hit.any() and not hit.all()
    same_bytes(lev[~hit], lc[~hit], "the rows without a NaN")
    assert np.isnan(lev[hit][:, 0]).all()
    for c, lo in enumerate(p.lout):
        _p64, peak = model(outs[c], lo)
        nan = np.isnan(peak)                                            # fmax: a row of NaN only stays NaN (whichever NaN)
        assert np.isnan(lev[nan, c, 1]).all() and lev[~nan, c, 1].tobytes() == peak[~nan].tobytes(), c


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
for h in (p, pw, po, pd, g):
    h.set_levels(True)
d_ring, d_out = C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0 and hip.hipMemset(d_ring, 0, C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(8 * pd.output_samples(nb))) == 0
entries = {"fdc_pipeline_work (path 5)": lambda: (p.work(x), p.levels()),
           "fdc_pipeline_work (spectrum path)": lambda: (pw.work(x2), pw.levels()),
           "fdc_pipeline_work (fine tuning, sc16 out)": lambda: (po.work(x2), po.levels()),
           "fdc_pipeline_process_device": lambda: (pd.process_device(d_ring, 5, nb, d_out), pd.levels()),
           "fdc_pipeline_group_work": lambda: (g.work(x), g.levels()),
           "fdc_pipeline_set_levels again": lambda: (pw.set_levels(False), pw.set_levels(True), pw.work(x2), pw.levels())}
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
assert "levels: pass" in p.describe() and "levels: with the rotation" in po.describe(), (p.describe(), po.describe())
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
    on = G.FrequencyDomainChannelizer(inptype=8, levels=True, **KW)
    off = G.FrequencyDomainChannelizer(inptype=8, **KW)
    assert on.levels is None and off.levels is None
    ya, yb = on.work(x), off.work(x)
    assert on.levels.shape == (nb, len(KW["throughput_channels"]), 2) and on.levels.dtype == np.float32 and off.levels is None
    for c, (u, v) in enumerate(zip(ya, yb)):
        same_bytes(u, v, "port %d" % c)
    levels_hold(on.pipeline, ya, on.levels, "hier block")
    # a call without items: an empty array
    on.work(x[:0])
    assert on.levels.shape == (0, 3, 2)
    # together with iq_output and fine_tuning: the levels are of the float ports of a block without iq_output, the ports its narrowed samples
    scale = int_scale(ya, np.int16)
    fine = G.FrequencyDomainChannelizer(inptype=8, levels=True, fine_tuning=True, **KW)
    both = G.FrequencyDomainChannelizer(inptype=8, levels=True, fine_tuning=True, iq_output="sc16", iq_output_scale=scale, **KW)
    yf, yi = fine.work(x), both.work(x)
    levels_hold(fine.pipeline, yf, fine.levels, "hier block with fine tuning")
    same_bytes(both.levels, fine.levels, "hier block with iq_output: the levels are taken before the narrowing")
    for c, (u, v) in enumerate(zip(yi, yf)):
        same_bytes(u, narrowed(v, scale, np.int16), "port %d, sc16" % c)
    # the Float input type, and two devices
    fl = G.FrequencyDomainChannelizer(inptype=4, levels=True, **KW)
    yr = fl.work(x.real.copy())
    levels_hold(fl.pipeline, yr, fl.levels, "hier block, Float input")
    kw = dict(KW, max_blocks=16)
    grp = G.FrequencyDomainChannelizer(inptype=8, levels=True, devices=[0, 0], **kw)
    one = G.FrequencyDomainChannelizer(inptype=8, levels=True, **kw)
    x16 = signal(16 * H, 12)
    yg, y1 = grp.work(x16), one.work(x16)
    assert isinstance(grp.pipeline, G.PipelineGroup) and grp.levels.shape == (16, 3, 2)
    same_bytes(grp.levels, one.levels, "devices=[0, 0]")
    levels_hold(one.pipeline, yg, grp.levels, "hier block on two virtual members")
