"""GPU tests (-m gpu) of fine tuning (fdc_pipeline_set_fine_tuning / fdc_pipeline_group_set_fine_tuning; include/fdc_amd.h).

The model: sample t of channel c's stream times w = exp(-2 pi i ((inc_c t) mod 2^64) / 2^64) in float64, applied to the float32 output of THE SAME handle on
the same input with fine tuning off, so the channelizer's own rounding and the path cancel out of every comparison.

Error bound (derived, DESIGN.md "Fine tuning"; not measured): the device multiplies y * base * step in float32.  base and step are each within 3 * 2^-24
of the exact phasors (sincospi <= 2 ulp + the argument's 2 pi 2^-27; the table: one rounding), two complex products add <= 2.5 * 2^-24 relative each:
11 * 2^-24 in total.  The tests assert |y' - y w| <= 20 * 2^-24 |y| + 2^-40 max|y| per sample: under twice the derived bound; the absolute term only
covers samples near zero."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from test_iq_input_gpu import EXAMPLE, iq, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCED = any(G.defaults.get(k) for k in ("FDC_FORCE_GENERIC", "FDC_NO_POLY", "FDC_NO_BLOCK", "FDC_NO_FUSED"))
FOUR256 = [(300 + 901 * c, 256, 0.8, 1.0) for c in range(4)]
MIXED = [(100, 256, 0.8, 1.0), (5001, 64, 0.6, 0.9)]
BANK = [(256 * c, 256, 0.88, 1.0) for c in range(64)]


def signal(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def phasors(nu, lout, first_block, nb):
    """w[t] for the nb * lout samples from block first_block on: 64-bit wrapping product, float64 phasor"""
    inc = np.uint64(G.fine_tuning_increment(nu))
    t = np.uint64(first_block * lout) + np.arange(nb * lout, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ph = inc * t
    return np.exp(-2j * np.pi * (ph.astype(np.float64) / 2.0 ** 64))


def holds(got, plain, nu, lout, first_block, what):
    """the model on one channel: got = the handle's output with fine tuning, plain = the same handle's without"""
    nb = plain.size // lout
    want = plain.astype(np.complex128) * phasors(nu, lout, first_block, nb)
    err = np.abs(got.astype(np.complex128) - want)
    bound = 20 * 2.0 ** -24 * np.abs(plain) + 2.0 ** -40 * np.abs(plain).max()
    k = int(np.argmax(err - bound))
    print("%s: largest error %.3g of its bound" % (what, float((err / bound).max())))
    assert (err <= bound).all(), "%s: sample %d: error %.3g above %.3g" % (what, k, err[k], bound[k])
    assert np.abs(plain).max() > 0


def nus(nchan, seed):
    """two draws per plan: random in (-0.5, 0.5); and one with the values 0 and 2^-30 in it"""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-0.5, 0.5, nchan), rng.uniform(-0.5, 0.5, nchan)
    b[0] = 2.0 ** -30
    b[-1] = 0.0
    return [a, b]


def route(p):
    d = p.describe()
    assert "fine tuning: " in d, d
    return d.split("fine tuning: ")[1].split(";")[0]


SHAPES = [
    ("N = 4096, R = 2, example plan (fused, two blocks per workgroup)", 4096, 2, EXAMPLE, 5, 0, 5, "fused", "two blocks"),
    ("N = 4096, R = 2, four 256-bin channels (fused, one block per workgroup)", 4096, 2, FOUR256, 5, 0, 5, "fused", "one block"),
    ("N = 4096, R = 4, example plan (lout = 3 l / 4)", 4096, 4, EXAMPLE, 5, 0, 5, "fused", None),
    ("N = 8192, generic path", 8192, 2, MIXED, 5, 0, 0, "rotated", None),
    ("N = 16384, R = 2, bank of 64 256-bin channels (block kernel)", 16384, 2, BANK, 96, 0, 3, "rotated", "k_blk256"),
    ("example plan under FDC_PIPE_NO_FUSED", 4096, 2, EXAMPLE, 5, G.FDC_PIPE_NO_FUSED, None, "rotated", None),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_model_on_every_route(shape):
    name, N, R, chans, nb, flags, path, want_route, words = shape
    H = N - N // R
    x = signal(nb * H, 1)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags)
    for k, nu in enumerate(nus(len(chans), 10)):
        p.reset()
        p.set_fine_tuning(nu)
        got = p.work(x)
        d = p.describe()
        p.set_fine_tuning(None)
        p.reset()
        plain = p.work(x)
        assert "fine tuning" in d and "fine tuning" not in p.describe(), (d, p.describe())
        for c, (u, v) in enumerate(zip(got, plain)):
            holds(u, v, nu[c], p.lout[c], 0, "%s draw %d ch%d (nu %r)" % (name, k, c, nu[c]))
        if not FORCED:
            assert ("fine tuning: " + want_route) in d, d
            assert path is None or p.path() == path, (p.path(), d)
            assert words is None or words in d, d
        elif flags:
            assert "fine tuning: rotated" in d, d
    # nu = 0 turns nothing: the samples of that channel are the plain ones up to the sign of a zero
    assert np.array_equal(got[-1], plain[-1])


def work_span(p, halo, span, first, n):
    outs = [np.empty(n * lo, np.complex64) for lo in p.lout]
    ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    _lib.check(_lib.lib().fdc_pipeline_work_span(p._h, None if halo is None else halo.ctypes.data, span.ctypes.data, first, n, ptrs, None))
    return outs


@pytest.mark.parametrize("N,chans,flags", [(4096, EXAMPLE, 0), (8192, MIXED, 0), (4096, EXAMPLE, G.FDC_PIPE_NO_FUSED)], ids=["fused", "rotated", "rotated, N = 4096"])
def test_cut_invariance_in_bytes(N, chans, flags):
    R, nb = 2, 6
    H, ovl = N - N // R, N // R
    x = signal(nb * H, 2)
    nu = nus(len(chans), 20)[0]
    one = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    one.set_fine_tuning(nu)
    whole = one.work(x)
    p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    p.set_fine_tuning(nu)
    pieces, b0 = [], 0
    for n in (1, 2, 3):
        pieces.append(p.work(x[b0 * H:(b0 + n) * H]))
        b0 += n
    q = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    q.set_fine_tuning(nu)
    spans, b0 = [], 0
    for n in (3, 1, 2):
        halo = x[b0 * H - ovl:b0 * H] if b0 else None
        spans.append(work_span(q, halo, x[b0 * H:(b0 + n) * H], b0, n))
        b0 += n
    for c in range(len(chans)):
        same_bytes(np.concatenate([o[c] for o in pieces]), whole[c], "1 + 2 + 3 blocks, ch%d" % c)
        same_bytes(np.concatenate([o[c] for o in spans]), whole[c], "spans with first_block, ch%d" % c)


def test_group_of_two_virtual_members_equals_one_handle():
    N, R, nb = 4096, 2, 8
    H = N - N // R
    x = signal(2 * nb * H, 3)
    nu = nus(len(EXAMPLE), 30)[1]
    g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
    g.set_fine_tuning(nu)
    p.set_fine_tuning(nu)
    for k in range(2):
        a, b = g.work(x[k * nb * H:(k + 1) * nb * H]), p.work(x[k * nb * H:(k + 1) * nb * H])
        for c, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, "call %d ch%d" % (k, c))
    assert sum(n > 0 for _f, n in g.last_spans()) == 2
    with pytest.raises(ValueError):
        g.set_fine_tuning(nu[:-1])
    g.set_fine_tuning(None)
    p.set_fine_tuning(None)
    for u, v in zip(g.work(x[:nb * H]), p.work(x[:nb * H])):
        same_bytes(u, v, "switched off")


@pytest.mark.parametrize("flags", [0, G.FDC_PIPE_NO_FUSED], ids=["fused", "rotated"])
def test_no_drift_far_into_the_stream(flags):
    """first_block = 2^40 + 3: t is about 2^51, where a float (or double) phase accumulator has lost every bit of the phase"""
    N, R, nb = 4096, 2, 4
    H = N - N // R
    first = 2 ** 40 + 3
    x = signal(nb * H, 4)
    halo = signal(N // R, 5)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, flags=flags)
    for k, nu in enumerate(nus(len(EXAMPLE), 40)):
        p.set_fine_tuning(nu)
        got = work_span(p, halo, x, first, nb)
        p.set_fine_tuning(None)
        plain = work_span(p, halo, x, first, nb)
        for c, (u, v) in enumerate(zip(got, plain)):
            holds(u, v, nu[c], p.lout[c], first, "first_block 2^40 + 3, draw %d ch%d" % (k, c))


@pytest.mark.parametrize("N,chans", [(4096, EXAMPLE), (8192, MIXED)], ids=["fused", "rotated"])
def test_setting_semantics(N, chans):
    R, nb = 2, 3
    H = N - N // R
    x = signal(3 * nb * H, 6)
    nu = nus(len(chans), 50)[0]
    q = G.Pipeline(N, R, chans, max_blocks=nb)
    plain = [q.work(x[k * nb * H:(k + 1) * nb * H]) for k in range(3)]
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    p.set_fine_tuning(nu)
    a0 = p.work(x[:nb * H])
    p.set_fine_tuning(np.zeros(len(chans)))               # all zeros = off
    a1 = p.work(x[nb * H:2 * nb * H])
    assert "fine tuning" not in p.describe()
    p.set_fine_tuning(nu)
    a2 = p.work(x[2 * nb * H:])
    for c in range(len(chans)):
        holds(a0[c], plain[0][c], nu[c], p.lout[c], 0, "on, ch%d" % c)
        same_bytes(a1[c], plain[1][c], "off, ch%d" % c)
        holds(a2[c], plain[2][c], nu[c], p.lout[c], 2 * nb, "on again (the block counter went on), ch%d" % c)
    # the setting survives reset(); what is refused changes nothing
    p.reset()
    lib = _lib.lib()
    bad = [np.resize(nu, len(chans) + 1), np.resize(nu, len(chans) - 1), np.where(np.arange(len(chans)) == 1, np.nan, nu),
           np.where(np.arange(len(chans)) == 0, 0.5, nu), np.where(np.arange(len(chans)) == 1, -0.5, nu), np.full(len(chans), 0.75)]
    for b in bad:
        with pytest.raises(ValueError):
            p.set_fine_tuning(b)
        assert lib.fdc_pipeline_set_fine_tuning(p._h, np.ascontiguousarray(b).ctypes.data_as(C.POINTER(C.c_double)), len(b)) == -1
    with pytest.raises(ValueError):
        p.set_fine_tuning(np.zeros((len(chans), 1)))
    assert lib.fdc_pipeline_set_fine_tuning(None, None, len(chans)) == -1
    b0 = p.work(x[:nb * H])
    for c in range(len(chans)):
        same_bytes(b0[c], a0[c], "after reset() and the refused calls, ch%d" % c)


def test_entries_that_write_the_channels_as_cut_are_refused():
    N, R, nb = 4096, 2, 3
    H, ovl = N - N // R, N // R
    hip = C.CDLL("libamdhip64.so")
    x = signal(2 * nb * H, 7)
    kw = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01, max_blocks=nb)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    q = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, **kw)
    w = G.Waterfall(N, 1e6, R, 1, 0, -100.0, 0.0, 0, 0, max_items=nb)
    nu = nus(len(EXAMPLE), 60)[0]

    def dev(nbytes):
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(d, 0, C.c_size_t(nbytes)) == 0
        return d

    d_ring, d_out, d_spec, d_pow = dev(8 * (ovl + nb * H)), dev(8 * p.output_samples(nb)), dev(8 * nb * N), dev(4 * nb * N // 16)
    spec_items = np.zeros(nb * N, np.complex64)
    entries = [("work(sinks=)", lambda: p.work(x[nb * H:], sinks=bank)),
               ("work_spectrum", lambda: p.work_spectrum(spec_items)),
               ("work_waterfall", lambda: p.work_waterfall(x[nb * H:], w)),
               ("process_device(d_group_power=)", lambda: p.process_device(d_ring, 0, nb, d_out, d_spectrum=d_spec, d_group_power=d_pow))]
    try:
        p.set_fine_tuning(nu)
        a0, b0 = p.work(x[:nb * H]), q.work(x[:nb * H])
        for name, call in entries:
            with pytest.raises(G.FdcError) as e:
                call()
            assert e.value.status == -1, name
        # nothing moved: the stream goes on where it was
        a1, b1 = p.work(x[nb * H:]), q.work(x[nb * H:])
        for c in range(len(EXAMPLE)):
            holds(a0[c], b0[c], nu[c], p.lout[c], 0, "before the refusals, ch%d" % c)
            holds(a1[c], b1[c], nu[c], p.lout[c], nb, "after the refusals, ch%d" % c)
        p.set_fine_tuning(None)
        for name, call in entries:
            call()                                            # they work again
        p.synchronize()
    finally:
        for d in (d_ring, d_out, d_spec, d_pow):
            hip.hipFree(d)


def narrowed(y, scale, dtype):
    """numpy's statement of the narrowing (tests/test_iq_output_gpu.py): saturate(rint(y * scale)) in float32, NaN -> 0"""
    info = np.iinfo(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.rint(np.ascontiguousarray(y, np.complex64).view(np.float32) * np.float32(scale))
    t = np.clip(np.nan_to_num(t, nan=0, posinf=info.max, neginf=info.min), info.min, info.max)
    return t.astype(dtype).reshape(-1, 2)


@pytest.mark.parametrize("N,chans,want", [(4096, EXAMPLE, "fused"), (8192, MIXED, "rotated")], ids=["fused", "rotated"])
def test_with_integer_input_and_output(N, chans, want):
    R, nb = 2, 5
    H = N - N // R
    xi = iq(nb * H, np.int16, 8)
    xf = (xi.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64)
    nu = nus(len(chans), 70)[1]
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    p.set_fine_tuning(nu)
    yf = p.work(xf)                                          # the handle's float y'
    for fmt, dt, scale in (("sc16", np.int16, 3000.0), ("sc8", np.int8, 20.0), ("sc16", np.int16, 1e6)):
        p.reset()
        p.set_output_format(fmt, scale)
        got = p.work(xf)
        d = p.describe()
        for c, (u, v) in enumerate(zip(got, yf)):
            same_bytes(u, narrowed(v, scale, dt), "%s x %r: the turn comes before the narrowing, ch%d" % (fmt, scale, c))
        if not FORCED:
            assert ("fine tuning: " + want) in d and ("output %s: %s" % (fmt, "fused" if want == "fused" else "narrowed")) in d, d
        p.reset()
        gi = p.work_iq(xi, scale=2.0 ** -15)                 # integer in, integer out
        for c, (u, v) in enumerate(zip(gi, got)):
            same_bytes(u, v, "%s: work_iq against work on the widened input, ch%d" % (fmt, c))
    p.set_output_format(None)
    p.reset()
    for c, (u, v) in enumerate(zip(p.work_iq(xi, scale=2.0 ** -15), yf)):
        same_bytes(u, v, "float out: work_iq against work on the widened input, ch%d" % c)


def test_a_tone_lands_on_dc():
    """One 64-bin channel asked for 0.4 bin of N above a bin centre, 64 blocks of a unit tone at exactly that carrier through the hier block: with
    fine_tuning the largest bin of the FFT of the 2048 output samples is bin 0; without, the bin the formula predicts (nu * 2048 rounded, 13)."""
    N, R, nb = 4096, 2, 64
    H = N - N // R
    freq = (2600 + 0.4) / N                                 # internal units: cycles per input sample, DC at 0.5
    bw = 40.0 / N                                            # 40 occupied bins -> l = 64
    kw = dict(inptype=8, inpveclen=1, blocksize=N, relinvovl=R, throughput_channels=[[freq - 0.5, bw]], activity_controlled_channels=[],
              act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
              outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
              minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False, max_blocks=nb)
    n = np.arange(nb * H, dtype=np.float64)
    x = np.exp(2j * np.pi * (freq - 0.5) * n).astype(np.complex64)      # a carrier at spectrum position freq = frequency freq - 0.5
    on = G.FrequencyDomainChannelizer(fine_tuning=True, **kw)
    off = G.FrequencyDomainChannelizer(**kw)
    (f, l, lout, _p, _s), = on.channel_params
    assert l == 64 and lout == 32 and f + l // 2 == 2600
    assert on.fine_nu[0] == pytest.approx(0.4 / 64, abs=1e-12) and off.fine_nu is None
    ya, yb = on.work(x)[0], off.work(x)[0]
    assert ya.size == yb.size == 2048
    assert int(np.argmax(np.abs(np.fft.fft(ya)))) == 0
    assert int(np.argmax(np.abs(np.fft.fft(yb)))) == int(round(on.fine_nu[0] * 2048)) == 13


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
rng = np.random.default_rng(3)
x = (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H)).astype(np.complex64)
x2 = (rng.standard_normal(nb * 4096) + 1j * rng.standard_normal(nb * 4096)).astype(np.complex64)
xi = rng.integers(-32768, 32768, 2 * nb * H).astype(np.int16)
EXAMPLE = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]
MIXED = [(100, 256, 0.8, 1.0), (5001, 64, 0.6, 0.9)]
p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb)
pw = G.Pipeline(8192, 2, MIXED, max_blocks=nb)
po = G.Pipeline(8192, 2, MIXED, max_blocks=nb)
g = G.PipelineGroup(N, R, EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
# fine tuning is set before the first counted call; setting it again with other values reuses the tables
for h, n in ((p, 4), (pw, 2), (po, 2), (g, 4)):
    h.set_fine_tuning(np.linspace(-0.4, 0.3, n))
po.set_output_format("sc16", 100.0)
entries = {"fdc_pipeline_work (fused)": lambda: p.work(x),
           "fdc_pipeline_work_iq (fused)": lambda: (p.reset(), p.work_iq(xi, scale=2.0 ** -15), p.reset()),
           "fdc_pipeline_work (rotated)": lambda: pw.work(x2),
           "fdc_pipeline_work (rotated, sc16 out)": lambda: po.work(x2),
           "fdc_pipeline_group_work": lambda: g.work(x),
           "fdc_pipeline_set_fine_tuning again": lambda: (pw.set_fine_tuning([0.1, -0.2]), pw.work(x2))}
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
p.work(x)            # (the last entry on p ended with reset(), which clears the route of the stream before it)
assert "fine tuning: " in p.describe() and "fine tuning: rotated" in pw.describe(), (p.describe(), pw.describe())
assert not bad, bad
print("OK")
'''


def test_no_allocation_in_the_steady_state(tmp_path):
    shim = str(tmp_path / "libhipcount.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hip_alloc_counter.c"), "-o", shim,
                           "-ldl", "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([sys.executable, "-c", NO_ALLOC_CHILD, shim, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
