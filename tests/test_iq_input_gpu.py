"""GPU tests (-m gpu) of complex integer input (fdc_pipeline_work_iq / _span_iq / process_device_iq / group_work_iq; include/fdc_amd.h).

Sample k of an sc16 / sc8 stream is (float(I_k) * scale, float(Q_k) * scale) rounded once in float32, and everything behind that is the complex
path: the outputs must be BYTE-EQUAL to the float entries on np.float32(I) * np.float32(scale) viewed as complex64, whichever kernel read the
integers (path 5 and the 256-bin banks read them in their own loads; every other plan widens them first)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from test_parity_gpu import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCED = any(G.defaults.get(k) for k in ("FDC_FORCE_GENERIC", "FDC_NO_POLY", "FDC_NO_BLOCK", "FDC_NO_FUSED"))
SCALES = [1.0, 2.0 ** -15, 1.0 / 3.0]
EXAMPLE = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]    # configs[0]: the example flowgraph's plan


def iq(n, dtype, seed):
    """n complex samples of interleaved I/Q, full scale included (both extremes at the start)"""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(seed)
    x = rng.integers(info.min, info.max + 1, size=2 * n, dtype=np.int64).astype(dtype)
    x[:4] = [info.min, info.max, info.max, info.min]
    return x


def widened(x, scale):
    return (x.astype(np.float32) * np.float32(scale)).view(np.complex64)


def same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), "%s: %d of %d samples differ" % (what, int(np.count_nonzero(a != b)), a.size)


def plans():
    full = lambda N, off=0: [(256 * c + off, 256, 0.88, 1.0) for c in range(N // 256 - (1 if off else 0))]
    return [
        # (name, N, R, channels, flags, "fused" / "widened", keep_spectrum)
        ("configs[1] (path 3)", 65536, 2, full(65536), 0, "fused", False),
        ("R = 4, N = 16384", 16384, 4, full(16384), 0, "fused", False),
        ("OFF, N = 16384", 16384, 2, full(16384, 37), 0, "fused", False),
        ("HALF, N = 16384", 16384, 2, full(16384, 128), 0, "fused", False),
        ("R = 4, N = 32768", 32768, 4, full(32768), 0, "fused", False),
        ("OFF, N = 32768", 32768, 2, full(32768, 77), 0, "fused", False),
        ("HALF, N = 32768", 32768, 2, full(32768, 128), 0, "fused", False),
        ("R = 4 OFF, N = 65536", 65536, 4, full(65536, 3), 0, "fused", False),
        ("configs[0], four 256-bin channels (k_f4096, one block per workgroup)", 4096, 2, [(300 + 901 * c, 256, 0.8, 1.0) for c in range(4)], 0, "fused", False),
        ("configs[0] example plan (k_f4096, two blocks per workgroup)", 4096, 2, EXAMPLE, 0, "fused", False),
        ("example plan under FDC_PIPE_NO_FUSED", 4096, 2, EXAMPLE, G.FDC_PIPE_NO_FUSED, "widened", False),
        ("mixed plan (path 1)", 16384, 2, [(100, 256, 0.8, 1.0), (1700, 512, 0.75, 0.95), (5001, 64, 0.6, 0.9)], 0, "widened", False),
        ("mixed plan, generic kernels (path 0)", 8192, 2, [(100, 256, 0.8, 1.0), (1700, 512, 0.75, 0.95), (5001, 64, 0.6, 0.9)], 0, "widened", False),
        ("256-bin channels at N = 262144 (path 2)", 262144, 2, [(256 * c, 256, 0.88, 1.0) for c in range(0, 1024, 97)], 0, "widened", False),
        ("split plan (path 4)", 65536, 2, full(65536)[:200] + [(60000, 512, 0.8, 1.0), (61001, 128, 0.7, 0.9)], 0, "widened", False),
        ("uniform 64-bin bank", 16384, 2, [(64 * c, 64, 0.88, 1.0) for c in range(256)], 0, "widened", False),
        ("uniform 512-bin bank", 65536, 2, [(512 * c, 512, 0.88, 1.0) for c in range(128)], 0, "widened", False),
        ("uniform 1024-bin bank", 65536, 2, [(1024 * c, 1024, 0.88, 1.0) for c in range(64)], 0, "widened", False),
        ("keep_spectrum, example plan", 4096, 2, EXAMPLE, 0, "widened", True),
        ("keep_spectrum, configs[1]", 65536, 2, full(65536)[::9], 0, "widened", True),
    ]


@pytest.mark.parametrize("case", plans(), ids=lambda c: c[0])
def test_work_iq_is_byte_equal_to_work_on_the_converted_input(case):
    name, N, R, chans, flags, route, keep = case
    H, nb = N - N // R, (3 if N >= 65536 else 5)
    for dtype, fmt in ((np.int16, "sc16"), (np.int8, "sc8")):
        for k, scale in enumerate(SCALES):
            x = iq(nb * H, dtype, 100 + k)
            p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
            q = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
            a = p.work_iq(x, scale=scale, want_spectrum=keep)
            b = q.work(widened(x, scale), want_spectrum=keep)
            if keep:
                (a, sa), (b, sb) = a, b
                same_bytes(sa, sb, "%s %s scale %r: spectrum" % (name, fmt, scale))
            for c, (u, v) in enumerate(zip(a, b)):
                same_bytes(u, v, "%s %s scale %r ch%d" % (name, fmt, scale, c))
            assert p.path() == q.path(), name
            d = p.describe()
            assert ("input %s: " % fmt) in d, d
            if not FORCED:
                assert ("input %s: %s" % (fmt, route)) in d, (name, d)


@pytest.mark.parametrize("teams_plan", [[(300 + 901 * c, 256, 0.8, 1.0) for c in range(4)], EXAMPLE], ids=["one block", "two blocks"])
def test_both_k_f4096_forms_are_fused(teams_plan):
    if FORCED:
        pytest.skip("the suite runs under a forced path")
    p = G.Pipeline(4096, 2, teams_plan, max_blocks=4)
    p.work_iq(iq(4 * 2048, np.int16, 5), scale=2.0 ** -15)
    d = p.describe()
    assert p.path() == 5 and "input sc16: fused" in d, d
    assert ("one block" if teams_plan is not EXAMPLE else "two blocks") in d, d


def test_stream_state_across_calls():
    N, R, mb = 16384, 2, 100
    H = N - N // R
    chans = [(256 * c + 128, 256, 0.88, 1.0) for c in range(63)]
    total = 1 + 7 + 100 + mb
    for dtype in (np.int16, np.int8):
        x = iq(total * H, dtype, 7)
        one = G.Pipeline(N, R, chans, max_blocks=total).work_iq(x, scale=1 / 3)
        p = G.Pipeline(N, R, chans, max_blocks=mb)
        got = [[] for _ in chans]
        b0 = 0
        for n in (1, 7, 100, mb):
            outs = p.work_iq(x[2 * b0 * H:2 * (b0 + n) * H], scale=1 / 3)
            for c, o in enumerate(outs):
                got[c].append(o)
            b0 += n
        for c in range(len(chans)):
            same_bytes(np.concatenate(got[c]), one[c], "ch%d" % c)


def test_span_entry_with_an_integer_halo():
    N, R = 4096, 2
    H, ovl = N - N // R, N // R
    for chans in (EXAMPLE, [(100, 256, 0.8, 1.0), (2001, 64, 0.6, 0.9)]):
        x = iq(9 * H, np.int16, 8)
        first, n = 4, 5
        halo = x[2 * (first * H - ovl):2 * first * H]
        span = x[2 * first * H:2 * (first + n) * H]
        p, q = G.Pipeline(N, R, chans, max_blocks=n), G.Pipeline(N, R, chans, max_blocks=n)
        a = p.work_span_iq(halo, span, first, scale=2.0 ** -15)
        hq = widened(halo, 2.0 ** -15)
        outs = [np.empty(n * lo, np.complex64) for lo in q.lout]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        xs = widened(span, 2.0 ** -15)
        _lib.check(_lib.lib().fdc_pipeline_work_span(q._h, hq.ctypes.data, xs.ctypes.data, first, n, ptrs, None))
        for c, (u, v) in enumerate(zip(a, outs)):
            same_bytes(u, v, "span ch%d" % c)


def test_group_of_two_virtual_members_equals_one_handle():
    N, R, nb = 65536, 2, 6
    H = N - N // R
    chans = [(256 * c, 256, 0.88, 1.0) for c in range(0, 256, 5)]
    x = iq(2 * nb * H, np.int16, 9)
    g = G.PipelineGroup(N, R, chans, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    for k in range(2):
        xs = x[2 * k * nb * H:2 * (k + 1) * nb * H]
        a, b = g.work_iq(xs, scale=2.0 ** -15), p.work_iq(xs, scale=2.0 ** -15)
        for c, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, "call %d ch%d" % (k, c))
    with pytest.raises(G.FdcError):
        g.work(widened(x[:2 * nb * H], 1.0))             # latched to sc16
    g.reset()
    g.work(widened(x[:2 * nb * H], 1.0))


@pytest.mark.parametrize("N,chans", [(65536, [(256 * c, 256, 0.88, 1.0) for c in range(256)]), (4096, EXAMPLE), (8192, [(100, 256, 0.8, 1.0), (5001, 64, 0.6, 0.9)])],
                         ids=["configs[1]", "configs[0]", "mixed"])
def test_process_device_iq_equals_process_device(N, chans):
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

    for dtype, fmt in ((np.int16, "sc16"), (np.int8, "sc8")):
        ring = iq(ovl + nb * H, dtype, 10)
        d_iq, d_f = dev(ring), dev(np.ascontiguousarray(widened(ring, 1 / 3)))
        o1, o2 = dev(np.zeros(n_out, np.complex64)), dev(np.zeros(n_out, np.complex64))
        try:
            p.process_device_iq(fmt, 1 / 3, d_iq, first, nb, o1)
            p.process_device(d_f, first, nb, o2)
            p.synchronize()
            a, b = np.empty(n_out, np.complex64), np.empty(n_out, np.complex64)
            assert hip.hipMemcpy(C.c_void_p(a.ctypes.data), o1, C.c_size_t(a.nbytes), 2) == 0
            assert hip.hipMemcpy(C.c_void_p(b.ctypes.data), o2, C.c_size_t(b.nbytes), 2) == 0
        finally:
            for d in (d_iq, d_f, o1, o2):
                hip.hipFree(d)
        same_bytes(a, b, "%s N=%d" % (fmt, N))
        assert ("input %s: " % fmt) in p.describe()


def test_input_form_is_latched():
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x = iq(3 * nb * H, np.int16, 11)
    xf = widened(x, 1.0)
    ref = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    r = [ref.work(xf[k * nb * H:(k + 1) * nb * H]) for k in range(3)]
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    a0 = p.work(xf[:nb * H])
    with pytest.raises(G.FdcError) as e:                 # float-latched: an integer call is refused and changes nothing
        p.work_iq(x[2 * nb * H:4 * nb * H], scale=1.0)
    assert e.value.status == -1
    a1 = p.work(xf[nb * H:2 * nb * H])
    for c in range(len(EXAMPLE)):
        same_bytes(a0[c], r[0][c], "ch%d" % c)
        same_bytes(a1[c], r[1][c], "ch%d after the refused call" % c)
    # integer-latched: another scale, another format and a float call are refused; the stream goes on
    q = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    b0 = q.work_iq(x[:2 * nb * H], scale=1.0)
    for bad in (lambda: q.work_iq(x[2 * nb * H:4 * nb * H], scale=0.5), lambda: q.work_iq(x[2 * nb * H:4 * nb * H].astype(np.int8), scale=1.0),
                lambda: q.work(xf[nb * H:2 * nb * H]), lambda: q.work_real(xf.real[nb * H:2 * nb * H].copy())):
        with pytest.raises(G.FdcError) as e:
            bad()
        assert e.value.status == -1
    b1 = q.work_iq(x[2 * nb * H:4 * nb * H], scale=1.0)
    for c in range(len(EXAMPLE)):
        same_bytes(b0[c], r[0][c], "ch%d" % c)
        same_bytes(b1[c], r[1][c], "ch%d after the refused calls" % c)
    q.reset()                                            # unlatched: a new form is taken
    c0 = q.work(xf[:nb * H])
    same_bytes(c0[0], r[0][0], "after reset")


@pytest.mark.parametrize("chans", [EXAMPLE, [(100, 256, 0.8, 1.0), (2001, 64, 0.6, 0.9)]], ids=["fused", "widened"])
@pytest.mark.parametrize("mb", [1, 2, 5])
def test_reset_then_a_wider_format(chans, mb):
    """sc8, reset, sc16 (the integer ring holds the widest format whatever was latched first; at R = 2 and max_blocks 1 / 2 the history of
    sc16 is as long as an sc8 ring of the whole call), then reset and float input: each stream byte-equal to a fresh handle."""
    N, R = 4096, 2
    H = N - N // R
    x8, x16 = iq(2 * mb * H, np.int8, 15), iq(2 * mb * H, np.int16, 16)
    p = G.Pipeline(N, R, chans, max_blocks=mb)
    for k in range(2):
        p.work_iq(x8[2 * k * mb * H:2 * (k + 1) * mb * H], scale=0.25)
    p.reset()
    fresh = G.Pipeline(N, R, chans, max_blocks=mb)
    for k in range(2):
        xs = x16[2 * k * mb * H:2 * (k + 1) * mb * H]
        a, b = p.work_iq(xs, scale=2.0 ** -15), fresh.work(widened(xs, 2.0 ** -15))
        for c, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, "sc16 after sc8 and reset, call %d ch%d" % (k, c))
    assert "input sc16: " in p.describe()
    p.reset()
    assert "input " not in p.describe()                  # the route of the earlier stream is gone
    fresh = G.Pipeline(N, R, chans, max_blocks=mb)
    xf = widened(x16[:2 * mb * H], 1.0)
    for c, (u, v) in enumerate(zip(p.work(xf), fresh.work(xf))):
        same_bytes(u, v, "float after reset ch%d" % c)
    assert "input " not in p.describe()


def test_group_reset_then_a_wider_format():
    N, R, nb = 4096, 2, 8
    H = N - N // R
    g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    g.work_iq(iq(nb * H, np.int8, 17), scale=0.5)
    g.reset()
    x = iq(nb * H, np.int16, 18)
    a, b = g.work_iq(x, scale=1 / 3), G.Pipeline(N, R, EXAMPLE, max_blocks=nb).work(widened(x, 1 / 3))
    for c, (u, v) in enumerate(zip(a, b)):
        same_bytes(u, v, "group sc16 after sc8 and reset ch%d" % c)


def test_pipelined_sinks_entry_refuses_a_float_call_on_an_integer_stream():
    N, R, nb = 4096, 2, 4
    H = N - N // R
    kw = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01,
              max_blocks=nb)
    p, bank = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True), G.Sinks(N, R, lookahead=True, **kw)
    x = iq(nb * H, np.int16, 19)
    p.work_iq(x, scale=1.0)
    with pytest.raises(G.FdcError) as e:
        p.work(widened(x, 1.0), sinks=bank)
    assert e.value.status == -1
    assert p.flush_sinks(bank) == 0                      # nothing of the refused call went in


def test_unknown_format_and_bad_scales_are_refused():
    p = G.Pipeline(4096, 2, EXAMPLE, max_blocks=2)
    x = iq(2 * 2048, np.int16, 12)
    outs = [np.empty(2 * lo, np.complex64) for lo in p.lout]
    ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    lib = _lib.lib()
    for fmt, sc in ((3, 1.0), (0, 1.0), (1, float("nan")), (1, 0.0), (2, float("inf"))):
        assert lib.fdc_pipeline_work_iq(p._h, fmt, sc, x.ctypes.data, 2, ptrs, None) == -1, (fmt, sc)
        assert lib.fdc_pipeline_process_device_iq(p._h, fmt, sc, None, 0, 0, None, None, None) == -1, (fmt, sc)
    p.work_iq(x, scale=1.0)                              # nothing was latched by the refused calls


def test_against_the_oracle(oracle):
    N, R, nb = 4096, 2, 6
    H = N - N // R
    x = iq(nb * H, np.int16, 13)
    xc = (x.astype(np.float64) / 32768.0).view(np.complex128).astype(np.complex64)
    outs = G.Pipeline(N, R, EXAMPLE, windowtype=1, max_blocks=nb).work_iq(x, scale=1 / 32768)
    ref, _ = oracle.channelizer(N, R, 1, EXAMPLE, xc)
    for c, (o, r) in enumerate(zip(outs, ref)):
        assert_close(o, r, "ch%d" % c)


def test_hier_block_routes_to_work_iq():
    N, R = 4096, 2
    H = N - N // R
    x = iq(4 * H, np.int16, 14)
    kw = dict(inpveclen=1, blocksize=N, relinvovl=R, throughput_channels=[[0.1, 0.05], [-0.2, 0.1]], activity_controlled_channels=[],
              act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False,
              fileoutput=False, outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0,
              act_det_deactivation_delay=0, minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0,
              act_det_maxblocks=0, debug=False, max_blocks=4)
    a = G.FrequencyDomainChannelizer(8, iq_input="sc16", iq_scale=1 / 32768, **kw).work(x)
    b = G.FrequencyDomainChannelizer(8, **kw).work(widened(x, 1 / 32768))
    for u, v in zip(a, b):
        same_bytes(u, v, "hier block")


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

N, R, nb = 4096, 2, 8
H = N - N // R
x = np.random.default_rng(3).integers(-32768, 32768, 2 * nb * H).astype(np.int16)
EXAMPLE = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]
p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pw = G.Pipeline(8192, 2, [(100, 256, 0.8, 1.0), (5001, 64, 0.6, 0.9)], max_blocks=nb)
x2 = np.random.default_rng(4).integers(-128, 128, 2 * nb * 4096).astype(np.int8)
g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
entries = {"fdc_pipeline_work_iq (fused)": lambda: p.work_iq(x, scale=2.0 ** -15),
           "fdc_pipeline_work_iq (widened)": lambda: pw.work_iq(x2, scale=0.25),
           "fdc_pipeline_group_work_iq": lambda: g.work_iq(x, scale=2.0 ** -15)}
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
assert not bad, bad
print("OK")
'''


def test_no_allocation_in_the_steady_state(tmp_path):
    shim = str(tmp_path / "libhipcount.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hip_alloc_counter.c"), "-o", shim,
                           "-ldl", "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([sys.executable, "-c", NO_ALLOC_CHILD, shim, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
