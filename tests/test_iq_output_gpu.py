"""GPU tests (-m gpu) of complex integer OUTPUT (fdc_pipeline_set_output_format / fdc_pipeline_group_set_output_format; include/fdc_amd.h).

Each component of a channel sample y becomes saturate(round_half_even(float32(y * scale))), NaN -> 0, +-Inf -> the limits: the outputs must be
BYTE-EQUAL to that numpy model applied to a float handle's outputs on the same input, whichever kernel narrowed them (path 5 and the 256-bin banks
in their own stores, every other plan behind the float kernels)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from test_iq_input_gpu import EXAMPLE, FORCED, iq, plans, same_bytes, widened

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_SCALES = [1.0, 32768.0, 1.0 / 3.0, 1e6]
FORMATS = (("sc16", np.int16), ("sc8", np.int8))
CONFIGS1 = [(256 * c, 256, 0.88, 1.0) for c in range(256)]
MIXED = [(100, 256, 0.8, 1.0), (2001, 64, 0.6, 0.9)]


def model(y, scale, dtype):
    """the contract: numpy's rint (half to even) of the float32 product, NaN -> 0, +-Inf -> the limits, saturated"""
    info = np.iinfo(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.rint(np.ascontiguousarray(y, np.complex64).view(np.float32) * np.float32(scale))
    t = np.clip(np.nan_to_num(t, nan=0, posinf=info.max, neginf=info.min), info.min, info.max)
    return t.astype(dtype).reshape(-1, 2)


def signal(n, seed, amp=100.0):
    """complex64 input whose channel outputs span the integer ranges at the scales above (1e6 saturates both ends)"""
    rng = np.random.default_rng(seed)
    return (amp * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def check(a, b, scale, dtype, what):
    assert len(a) == len(b), what
    for c, (u, v) in enumerate(zip(a, b)):
        same_bytes(u, model(v, scale, dtype), "%s ch%d" % (what, c))


def full(N, off=0):
    return [(256 * c + off, 256, 0.88, 1.0) for c in range(N // 256 - (1 if off else 0))]


# the k_blk256 forms plans() leaves out: P = 8 OFF / HALF, and R = 4 on the grid / HALF (P = 4 and 8)
EXTRA = [
    ("OFF, N = 65536", 65536, 2, full(65536, 37), 0, "fused", False),
    ("HALF, N = 65536", 65536, 2, full(65536, 128), 0, "fused", False),
    ("R = 4, N = 65536", 65536, 4, full(65536), 0, "fused", False),
    ("R = 4 HALF, N = 32768", 32768, 4, full(32768, 128), 0, "fused", False),
    ("R = 4 HALF, N = 65536", 65536, 4, full(65536, 128), 0, "fused", False),
]


def route(p):
    d = p.describe()
    assert "output " in d, d
    return "fused" if ": fused" in d.split("output ")[1] else "narrowed"


@pytest.mark.parametrize("case", plans() + EXTRA, ids=lambda c: c[0])
def test_work_is_byte_equal_to_the_model_on_every_path(case):
    name, N, R, chans, flags, r_in, keep = case
    H, nb = N - N // R, (3 if N >= 65536 else 5)
    x = signal(nb * H, 200)
    q = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
    ref = q.work(x, want_spectrum=keep)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
    saturated = {np.int16: [False, False], np.int8: [False, False]}
    for fmt, dt in FORMATS:
        for scale in OUT_SCALES:
            p.reset()
            p.set_output_format(fmt, scale)
            got = p.work(x, want_spectrum=keep)
            if keep:
                (got, sa), (b, sb) = got, ref
                same_bytes(sa, sb, "%s %s x %r: the spectrum stays complex64" % (name, fmt, scale))
            else:
                b = ref
            check(got, b, scale, dt, "%s %s x %r" % (name, fmt, scale))
            if scale == 1e6:
                allv = np.concatenate([g.ravel() for g in got])
                info = np.iinfo(dt)
                saturated[dt] = [bool((allv == info.min).any()), bool((allv == info.max).any())]
            if not FORCED:
                # (N = 65536 at R = 4 on float input narrows behind the float kernel: its integer-store forms would spill)
                want = "fused" if r_in == "fused" and not (N == 65536 and R == 4) else "narrowed"
                assert route(p) == want, (name, p.describe())
    assert saturated[np.int16] == [True, True] and saturated[np.int8] == [True, True], saturated


@pytest.mark.parametrize("case", plans() + EXTRA, ids=lambda c: c[0])
def test_integer_in_and_out_on_every_path(case):
    """sc16 / sc8 input with sc16 / sc8 output: every input form of every k_blk256 / k_f4096 form with integer stores is launched here"""
    name, N, R, chans, flags, r_in, keep = case
    H, nb = N - N // R, (3 if N >= 65536 else 5)
    for (ifmt, idt), (ofmt, odt) in (FORMATS[0], FORMATS[0]), (FORMATS[1], FORMATS[1]), (FORMATS[0], FORMATS[1]), (FORMATS[1], FORMATS[0]):
        x = iq(nb * H, idt, 310)
        sc_in, sc_out = (2.0 ** -15 if idt is np.int16 else 1 / 128), 1024.0
        q = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
        p.set_output_format(ofmt, sc_out)
        a, b = p.work_iq(x, scale=sc_in, want_spectrum=keep), q.work_iq(x, scale=sc_in, want_spectrum=keep)
        if keep:
            (a, sa), (b, sb) = a, b
            same_bytes(sa, sb, "%s: the spectrum stays complex64" % name)
        check(a, b, sc_out, odt, "%s: %s in, %s out" % (name, ifmt, ofmt))
        if not FORCED:
            d = p.describe()
            assert ("input %s: %s" % (ifmt, r_in)) in d, (name, d)
            assert route(p) == ("fused" if r_in == "fused" else "narrowed"), (name, d)


def tie_scale(y, target):
    """a float32 scale s with float32(y * s) == target exactly (numpy's float32 product is the device's contract-off product), or None"""
    s0 = np.float32(target / float(y))
    for direction in (np.float32(np.inf), np.float32(-np.inf)):
        s = s0
        for _ in range(256):
            if np.float32(y) * s == np.float32(target):
                return s
            s = np.nextafter(s, direction, dtype=np.float32)
    return None


@pytest.mark.parametrize("N,chans,registered", [(16384, full(16384), False), (4096, EXAMPLE, False), (4096, MIXED, False), (4096, MIXED, True),
                                                (4096, EXAMPLE, True)],
                         ids=["k_blk256", "k_f4096", "k_complex_to_iq", "k_scatter_oq narrowing", "k_scatter_oq copy"])
def test_ties_round_half_to_even(N, chans, registered):
    """channel outputs that land exactly on k + 1/2: half to even gives 10, 12, -10, -12 where half away from zero gives 11, 12, -11, -12, half up
    11, 12, -10, -11 and truncation 10, 11, -10, -11"""
    R, nb = 2, 3
    H = N - N // R
    x = signal(nb * H, 1200, amp=1.0)
    ref = G.Pipeline(N, R, chans, max_blocks=nb).work(x)
    y = ref[0].view(np.float32)
    cand = [i for i in np.flatnonzero((np.abs(y) > 0.05) & (np.abs(y) < 50))]
    assert len(cand) >= 8
    for fmt, dt in FORMATS:
        used = 0
        for target, want in ((10.5, 10), (11.5, 12), (-10.5, -10), (-11.5, -12)):
            sc, i = None, None
            for i in cand[used:]:
                used += 1
                sc = tie_scale(y[i], target)
                if sc is not None and np.isfinite(sc):
                    break
            assert sc is not None, target
            p = G.Pipeline(N, R, chans, max_blocks=nb)
            p.set_output_format(fmt, float(sc))
            assert np.float32(y[i]) * np.float32(p.output_format()[1]) == np.float32(target)
            outs = [np.zeros((nb * lo, 2), dt) for lo in p.lout]
            if registered:
                for o in outs:
                    G.register_host(o)
            try:
                got = p.work(x, outs=outs)
            finally:
                if registered:
                    for o in outs:
                        G.unregister_host(o)
            assert int(got[0].reshape(-1)[i]) == want, (fmt, target, int(got[0].reshape(-1)[i]), p.describe())
            check(got, ref, sc, dt, "%s tie %r" % (fmt, target))


@pytest.mark.parametrize("N,chans,flags,want,want_in", [(65536, CONFIGS1, 0, "fused", "fused"), (4096, EXAMPLE, 0, "fused", "fused"),
                                                         (32768, CONFIGS1[:128], G.FDC_PIPE_PLAIN_STORES, "narrowed", "fused"),
                                                         (4096, EXAMPLE, G.FDC_PIPE_NO_FUSED, "narrowed", "widened"),
                                                         (16384, CONFIGS1[:50] + [(13001, 64, 0.6, 0.9)], 0, "narrowed", "widened")],
                         ids=["configs[1]", "configs[0]", "plain stores", "configs[0] NO_FUSED", "mixed"])
def test_integer_in_and_out(N, chans, flags, want, want_in):
    R = 2
    H, nb = N - N // R, (3 if N >= 65536 else 6)
    for (ifmt, idt), (ofmt, odt) in (((a, b), (c, d)) for (a, b) in FORMATS for (c, d) in FORMATS):
        x = iq(nb * H, idt, 300)
        sc_in, sc_out = (2.0 ** -15 if idt is np.int16 else 1 / 128), 512.0
        q = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
        p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
        p.set_output_format(ofmt, sc_out)
        check(p.work_iq(x, scale=sc_in), q.work_iq(x, scale=sc_in), sc_out, odt, "%s in, %s out" % (ifmt, ofmt))
        if not FORCED:
            assert route(p) == want, p.describe()
            assert ("input %s: %s" % (ifmt, want_in)) in p.describe(), p.describe()


@pytest.mark.parametrize("chans", [EXAMPLE, MIXED], ids=["fused", "narrowed"])
@pytest.mark.parametrize("sub", [0, 2], ids=["one sub-batch", "sub-batches of 2"])
@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
def test_host_fed_branches_and_ragged_calls(chans, sub, registered):
    N, R, mb = 4096, 2, 7
    H = N - N // R
    sizes = (1, 7, 3, 5)
    x = signal(sum(sizes) * H, 400)
    one = G.Pipeline(N, R, chans, max_blocks=sum(sizes)).work(x)
    p = G.Pipeline(N, R, chans, max_blocks=mb, host_sub_blocks=sub or None)
    p.set_output_format("sc16", 300.0)
    bufs = [np.zeros((mb * lo, 2), np.int16) for lo in p.lout]
    if registered:
        for b in bufs:
            G.register_host(b)
    try:
        got, b0 = [[] for _ in chans], 0
        for n in sizes:
            outs = [b[:n * lo] for b, lo in zip(bufs, p.lout)]
            p.work(x[b0 * H:(b0 + n) * H], outs=outs)
            for c, o in enumerate(outs):
                got[c].append(o.copy())
            b0 += n
    finally:
        if registered:
            for b in bufs:
                G.unregister_host(b)
    check([np.concatenate(g) for g in got], one, 300.0, np.int16, "ragged stream")


def test_outs_are_checked_for_dtype_and_size():
    p = G.Pipeline(4096, 2, EXAMPLE, max_blocks=2)
    p.set_output_format("sc8", 64.0)
    x = signal(2 * 2048, 1)
    for bad in ([np.empty(2 * lo, np.complex64) for lo in p.lout], [np.empty((2 * lo, 2), np.int16) for lo in p.lout],
                [np.empty((2 * lo - 1, 2), np.int8) for lo in p.lout]):
        with pytest.raises(ValueError):
            p.work(x, outs=bad)
    outs = [np.empty((2 * lo, 2), np.int8) for lo in p.lout]
    assert p.work(x, outs=outs) is outs


def test_real_and_span_entries():
    N, R = 4096, 2
    H, ovl = N - N // R, N // R
    for chans in (EXAMPLE, MIXED):
        xr = signal(6 * H, 500).real.copy()
        q, p = G.Pipeline(N, R, chans, max_blocks=6), G.Pipeline(N, R, chans, max_blocks=6)
        p.set_output_format("sc16", 1000.0)
        check(p.work_real(xr), q.work_real(xr), 1000.0, np.int16, "work_real")
        # span entries with a halo: float input (C entry) and sc16 input
        x = signal(9 * H, 501)
        first, n = 4, 5
        halo, span = x[first * H - ovl:first * H], x[first * H:(first + n) * H]
        q, p = G.Pipeline(N, R, chans, max_blocks=n), G.Pipeline(N, R, chans, max_blocks=n)
        p.set_output_format("sc8", 2.0)
        fl = [np.empty(n * lo, np.complex64) for lo in q.lout]
        nar = [np.empty((n * lo, 2), np.int8) for lo in p.lout]
        for h, o in ((q._h, fl), (p._h, nar)):
            ptrs = (C.c_void_p * len(o))(*[a.ctypes.data for a in o])
            _lib.check(_lib.lib().fdc_pipeline_work_span(h, halo.ctypes.data, span.ctypes.data, first, n, ptrs, None))
        check(nar, fl, 2.0, np.int8, "work_span")
        xi = iq(9 * H, np.int16, 502)
        hi, si = xi[2 * (first * H - ovl):2 * first * H], xi[2 * first * H:2 * (first + n) * H]
        q, p = G.Pipeline(N, R, chans, max_blocks=n), G.Pipeline(N, R, chans, max_blocks=n)
        p.set_output_format("sc16", 2.0)
        check(p.work_span_iq(hi, si, first, scale=2.0 ** -8), q.work_span_iq(hi, si, first, scale=2.0 ** -8), 2.0, np.int16, "work_span_iq")


def test_group_of_two_virtual_members_equals_one_handle():
    N, R, nb = 65536, 2, 6
    H = N - N // R
    chans = CONFIGS1[::5]
    x = signal(2 * nb * H, 600)
    g = G.PipelineGroup(N, R, chans, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    g.set_output_format("sc16", 4096.0)
    p.set_output_format("sc16", 4096.0)
    for k in range(2):
        xs = x[k * nb * H:(k + 1) * nb * H]
        a, b = g.work(xs), p.work(xs)
        for c, (u, v) in enumerate(zip(a, b)):
            assert u.dtype == np.int16 and u.shape == (nb * p.lout[c], 2)
            same_bytes(u, v, "group call %d ch%d" % (k, c))
    xi = iq(nb * H, np.int8, 601)
    g.reset()
    p.reset()
    g.set_output_format("sc8", 8.0)
    p.set_output_format("sc8", 8.0)
    for c, (u, v) in enumerate(zip(g.work_iq(xi, scale=0.5), p.work_iq(xi, scale=0.5))):
        same_bytes(u, v, "group sc8 in / out ch%d" % c)


@pytest.mark.parametrize("chans", [EXAMPLE, MIXED], ids=["fused", "narrowed"])
def test_non_finite_values(chans):
    N, R, nb = 4096, 2, 4
    H = N - N // R
    x = signal(nb * H, 700)
    x[10] = np.nan                                         # block 0: NaN everywhere behind the transform
    x[H + 5] = np.complex64(np.inf)                        # block 1: Inf (and Inf - Inf = NaN)
    x[3 * H:3 * H + 200] = np.complex64(3e38 + 3e38j)      # block 3: overflow to +-Inf in the transform
    q, p = G.Pipeline(N, R, chans, max_blocks=nb), G.Pipeline(N, R, chans, max_blocks=nb)
    ref = q.work(x)
    assert not all(np.isfinite(r).all() for r in ref)
    for fmt, dt in FORMATS:
        p.reset()
        p.set_output_format(fmt, 1.0)
        check(p.work(x), ref, 1.0, dt, "non-finite %s" % fmt)


@pytest.mark.parametrize("chans", [EXAMPLE, MIXED], ids=["fused", "narrowed"])
def test_switching_mid_stream_and_across_reset(chans):
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x = signal(3 * nb * H, 800)
    ref = G.Pipeline(N, R, chans, max_blocks=3 * nb).work(x)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    a0 = p.work(x[:nb * H])
    p.set_output_format("sc16", 50.0)
    a1 = p.work(x[nb * H:2 * nb * H])
    p.set_output_format(None)
    a2 = p.work(x[2 * nb * H:])
    for c in range(len(chans)):
        lo = p.lout[c]
        same_bytes(a0[c], ref[c][:nb * lo], "float, ch%d" % c)
        same_bytes(a1[c], model(ref[c][nb * lo:2 * nb * lo], 50.0, np.int16), "sc16, ch%d" % c)
        same_bytes(a2[c], ref[c][2 * nb * lo:], "float again, ch%d" % c)
    p.set_output_format("sc8", 50.0)
    p.reset()                                              # the format survives a reset
    assert p.output_format() == ("sc8", 50.0)
    b = p.work(x[:nb * H])
    for c in range(len(chans)):
        same_bytes(b[c], model(ref[c][:nb * p.lout[c]], 50.0, np.int8), "sc8 after reset, ch%d" % c)


@pytest.mark.parametrize("N,chans", [(65536, CONFIGS1), (4096, EXAMPLE), (8192, MIXED)], ids=["configs[1]", "configs[0]", "mixed"])
def test_device_entries(N, chans):
    hip = C.CDLL("libamdhip64.so")
    R, nb, first = 2, 4, 13
    H, ovl = N - N // R, N // R
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    n_out = p.output_samples(nb)

    def dev(a):
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(max(1, a.nbytes))) == 0
        assert hip.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return d

    def back(d, a):
        assert hip.hipMemcpy(C.c_void_p(a.ctypes.data), d, C.c_size_t(a.nbytes), 2) == 0
        return a

    ring_i = iq(ovl + nb * H, np.int16, 900)
    ring_f = np.ascontiguousarray(signal(ovl + nb * H, 901))
    d_i, d_f = dev(ring_i), dev(ring_f)
    o_f, o_n = dev(np.zeros(n_out, np.complex64)), dev(np.zeros((n_out, 2), np.int16))
    try:
        for fmt, dt in FORMATS:
            p.set_output_format(None)
            p.process_device(d_f, first, nb, o_f)
            p.synchronize()
            f = back(o_f, np.empty(n_out, np.complex64))
            p.set_output_format(fmt, 200.0)
            p.process_device(d_f, first, nb, o_n)
            p.synchronize()
            same_bytes(back(o_n, np.empty((n_out, 2), dt)), model(f, 200.0, dt), "process_device %s N=%d" % (fmt, N))
            p.set_output_format(None)
            p.process_device_iq("sc16", 2.0 ** -10, d_i, first, nb, o_f)
            p.synchronize()
            f = back(o_f, np.empty(n_out, np.complex64))
            p.set_output_format(fmt, 200.0)
            p.process_device_iq("sc16", 2.0 ** -10, d_i, first, nb, o_n)
            p.synchronize()
            same_bytes(back(o_n, np.empty((n_out, 2), dt)), model(f, 200.0, dt), "process_device_iq sc16 -> %s N=%d" % (fmt, N))
            if not FORCED:
                assert route(p) == ("narrowed" if N == 8192 else "fused"), p.describe()
    finally:
        for d in (d_i, d_f, o_f, o_n):
            hip.hipFree(d)


def test_refusals_leave_the_stream_where_it_was():
    # R = 4 and 3 blocks a call: a refused entry that advanced the block counter would move the window phase (first_block * shift mod R)
    N, R, nb = 4096, 4, 3
    H, ovl = N - N // R, N // R
    x = signal(3 * nb * H, 1000)
    kw = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01,
              max_blocks=nb)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    q = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    serial, ahead = G.Sinks(N, R, **kw), G.Sinks(N, R, lookahead=True, **kw)
    w = G.Waterfall(N, 1e6, R, 1, 0, -100.0, 0.0, 0, 0, max_items=nb)
    p.set_output_format("sc16", 100.0)
    p.work(x[:nb * H])
    q.work(x[:nb * H])
    xb = x[2 * nb * H:3 * nb * H]
    outs = [np.empty(nb * lo, np.complex64) for lo in p.lout]
    ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    lib = _lib.lib()
    nrows = C.c_int32()
    spec_items = np.zeros(nb * N, np.complex64)
    for name, call in (("work_sinks (serial)", lambda: lib.fdc_pipeline_work_sinks(p._h, xb.ctypes.data, nb, ptrs, None, serial._h)),
                       ("work_sinks (pipelined)", lambda: lib.fdc_pipeline_work_sinks(p._h, xb.ctypes.data, nb, ptrs, None, ahead._h)),
                       ("flush_sinks", lambda: lib.fdc_pipeline_flush_sinks(p._h, ahead._h)),
                       ("work_spectrum", lambda: lib.fdc_pipeline_work_spectrum(p._h, spec_items.ctypes.data, nb, ptrs, None, None)),
                       ("process_device_power", lambda: lib.fdc_pipeline_process_device_power(p._h, None, 0, nb, None, None, None, None)),
                       ("work_waterfall", lambda: lib.fdc_pipeline_work_waterfall(p._h, w._h, xb.ctypes.data, nb, ptrs, None, None, None, 8,
                                                                                   C.byref(nrows)))):
        assert call() == -1, name
    # nothing moved: the stream continues exactly
    a = p.work(x[nb * H:2 * nb * H])
    b = q.work(x[nb * H:2 * nb * H])
    check(a, b, 100.0, np.int16, "after the refusals")
    # ... and the comparison would see a block counter moved by one refused call: the same span at first_block 2 nb differs
    s = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    moved = [np.empty(nb * lo, np.complex64) for lo in s.lout]
    mp = (C.c_void_p * len(moved))(*[o.ctypes.data for o in moved])
    halo, span = x[nb * H - ovl:nb * H], x[nb * H:2 * nb * H]
    _lib.check(lib.fdc_pipeline_work_span(s._h, halo.ctypes.data, span.ctypes.data, 2 * nb, nb, mp, None))
    assert any(not np.array_equal(model(u, 100.0, np.int16), model(v, 100.0, np.int16)) for u, v in zip(moved, b))
    # set_output_format refuses unknown formats, bad scales, and a handle with an unflushed pipelined batch
    for fmt, sc in ((3, 1.0), (-1, 1.0), (1, 0.0), (1, float("nan")), (2, float("inf")), (0, 0.0)):
        assert lib.fdc_pipeline_set_output_format(p._h, fmt, sc) == -1, (fmt, sc)
    r = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    while r.flush_sinks(ahead) > 0:
        pass
    r.work(x[:nb * H], sinks=ahead)
    assert lib.fdc_pipeline_set_output_format(r._h, 1, 1.0) == -1
    while r.flush_sinks(ahead) > 0:
        pass
    r.set_output_format("sc16", 1.0)
    assert r.output_format() == ("sc16", 1.0)


def test_group_refuses_members_with_different_formats():
    N, R, nb = 4096, 2, 8
    H = N - N // R
    x = signal(nb * H, 1300)
    g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    lib = _lib.lib()
    m1 = lib.fdc_pipeline_group_member(g._h, 1)
    _lib.check(lib.fdc_pipeline_set_output_format(m1, 1, 64.0))       # one member set on its own: the spans would be placed wrongly
    with pytest.raises(G.FdcError) as e:
        g.work(x)
    assert e.value.status == -1
    g.set_output_format("sc16", 64.0)
    a, b = g.work(x), G.Pipeline(N, R, EXAMPLE, max_blocks=nb).work(x)
    check(a, b, 64.0, np.int16, "group after the refusal")


def test_hier_block():
    N, R = 4096, 2
    H = N - N // R
    kw = dict(inpveclen=1, blocksize=N, relinvovl=R, throughput_channels=[[0.1, 0.05], [-0.2, 0.1]], activity_controlled_channels=[],
              act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False,
              fileoutput=False, outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0,
              act_det_deactivation_delay=0, minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0,
              act_det_maxblocks=0, debug=False, max_blocks=4)
    x = signal(4 * H, 1100, amp=0.5)
    a = G.FrequencyDomainChannelizer(8, iq_output="sc16", iq_output_scale=32768, **kw).work(x)
    b = G.FrequencyDomainChannelizer(8, **kw).work(x)
    for u, v in zip(a, b):
        assert u.dtype == np.int16 and u.ndim == 2 and u.shape[1] == 2
        same_bytes(u, model(v, 32768, np.int16), "hier block")
    xi = iq(4 * H, np.int16, 1101)
    a = G.FrequencyDomainChannelizer(8, iq_input="sc16", iq_scale=1 / 32768, iq_output="sc8", iq_output_scale=128, **kw).work(xi)
    b = G.FrequencyDomainChannelizer(8, **kw).work(widened(xi, 1 / 32768))
    for u, v in zip(a, b):
        same_bytes(u, model(v, 128, np.int8), "hier block, sc16 in / sc8 out")
    xr = x.real.copy()
    a = G.FrequencyDomainChannelizer(4, iq_output="sc16", iq_output_scale=32768, **kw).work(xr)
    b = G.FrequencyDomainChannelizer(4, **kw).work(xr)
    for u, v in zip(a, b):
        same_bytes(u, model(v, 32768, np.int16), "hier block, Float input")


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
x = (100 * np.random.default_rng(3).standard_normal(2 * nb * H)).astype(np.float32).view(np.complex64)
xi = np.random.default_rng(4).integers(-32768, 32768, 2 * nb * H).astype(np.int16)
EXAMPLE = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]
MIXED = [(100, 256, 0.8, 1.0), (2001, 64, 0.6, 0.9)]
pf = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pn = G.Pipeline(N, R, MIXED, max_blocks=nb, host_sub_blocks=3)
g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
for h in (pf, pn, g):
    h.set_output_format("sc16", 100.0)
ring = C.c_void_p(); dout = C.c_void_p()
assert hip.hipMalloc(C.byref(ring), C.c_size_t(8 * (nb * H + N // R))) == 0
assert hip.hipMalloc(C.byref(dout), C.c_size_t(4 * 4 * pf.output_samples(nb) + 4 * pn.output_samples(nb))) == 0
assert hip.hipMemset(ring, 0, C.c_size_t(8 * (nb * H + N // R))) == 0
entries = {"work (fused)": lambda: pf.work(x),
           "work (narrowed, sub-batches)": lambda: pn.work(x),
           "work_iq (fused)": lambda: None,
           "group work": lambda: g.work(x),
           "process_device (fused)": lambda: (pf.process_device(ring, 0, nb, dout), pf.synchronize()),
           "process_device (narrowed)": lambda: (pn.process_device(ring, 0, nb, dout), pn.synchronize())}
qi = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
qi.set_output_format("sc8", 1.0)
entries["work_iq (fused)"] = lambda: qi.work_iq(xi, scale=2.0 ** -15)
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
hip.hipFree(ring); hip.hipFree(dout)
assert not bad, bad
print("OK")
'''


def test_no_allocation_in_the_steady_state(tmp_path):
    shim = str(tmp_path / "libhipcount.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hip_alloc_counter.c"), "-o", shim,
                           "-ldl", "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([sys.executable, "-c", NO_ALLOC_CHILD, shim, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
