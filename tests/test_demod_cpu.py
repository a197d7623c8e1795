"""CPU tests of the channel demodulation (no GPU): the numpy models of tests/demod_model.py on hand-made rows, the zero rule and the cut rule on the
model, the float32 restatement inside the bound at every run length the GPU tests use, the ctypes prototypes of the three C-ABI entries against
include/fdc_amd.h, the Python checks made before any library call, and the hier block's keyword, refusals and acceptances."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup
import demod_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdc_pipeline_set_demod", "fdc_pipeline_demod", "fdc_pipeline_demod_device")
# the run lengths (nblocks * lout) the GPU tests reach, by what they reach in the kernel (tests/test_demod_routes_gpu.py)
RUNS = (1, 2, 3, 4, 5, 15, 16, 60, 128, 255, 256, 257, 260, 640, 896, 1024, 3072, 24576, 5 * 24576)


def f32bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32).tolist()


def test_models_on_hand_made_rows():
    two_pi = 2 * np.pi
    # a constant row: no turn; the first sample against a zero in front is the zero rule
    y = np.full(6, 2 - 1j, np.complex64)
    assert f32bits(M.fm32(y)) == [0] * 6
    assert M.fm32(y, front=2 - 1j).tolist() == [0.0] * 6 and M.theta64(y, 2 - 1j).tolist() == [0.0] * 6
    assert f32bits(M.mag32(y)) == f32bits(np.full(6, np.sqrt(np.float32(5.0)), np.float32))
    # a tone of known frequency: with gain 1 / (2 pi) the FM output is the frequency, in cycles per sample
    for n, nu in ((16, 0.125), (240, -0.31), (768, 0.004)):
        y = np.exp(2j * np.pi * nu * np.arange(n)).astype(np.complex64)
        d = M.fm32(y, front=np.complex64(np.exp(-2j * np.pi * nu)), gain=1 / two_pi)
        assert d.dtype == np.float32 and np.abs(d - nu).max() < 1e-6, (n, nu)
        assert np.abs(M.theta64(y, np.complex64(np.exp(-2j * np.pi * nu))) / two_pi - nu).max() < 1e-6
        assert np.abs(M.mag32(y, 3.0) - 3.0).max() < 1e-6
    # a zero row: +0.0 in bits in both modes, whatever stands in front and whatever the gain's sign (FM); MAG gives gain * 0
    z = np.zeros(5, np.complex64)
    assert f32bits(M.fm32(z, front=1 + 1j, gain=-2.0)) == [0] * 5 and f32bits(M.mag32(z)) == [0] * 5
    assert f32bits(M.mag32(z, -1.0)) == [0x80000000] * 5
    # signed zeros give zeros, not +-pi: (-0, -0) products compare equal to zero
    y = np.array([complex(-0.0, 0.0), complex(0.0, -0.0), 1], np.complex64)
    assert f32bits(M.fm32(y, front=-1))[:2] == [0, 0]
    # NaN propagates to the two samples whose product holds it, and to its own magnitude
    y = np.array([1, 1j, complex(np.nan, 0), 2, 1], np.complex64)
    d = M.fm32(y, front=1)
    assert np.isnan(d).tolist() == [False, False, True, True, False] and d[1] == np.float32(np.pi / 2) and d[4] == 0
    assert np.isnan(M.mag32(y)).tolist() == [False, False, True, False, False]
    # +-Inf: what IEEE arithmetic gives (Inf * 0 in a cross product is NaN), an infinite magnitude
    y = np.array([1, complex(np.inf, 0), 1], np.complex64)
    assert np.isnan(M.fm32(y, front=1)[1:]).all() and M.mag32(y)[1] == np.inf
    y = np.array([1 + 1j, complex(np.inf, np.inf)], np.complex64)
    assert np.isnan(M.fm32(y, front=1)[1]) and M.mag32(y, -1.0)[1] == -np.inf
    # lout = 1, one block: one sample, against the front alone
    assert M.fm32(np.array([1j], np.complex64), front=1).tolist() == [np.float32(np.pi / 2)]
    assert f32bits(M.fm32(np.array([1j], np.complex64))) == [0]
    assert M.fm_bound(0.0) == 5 * 2.0 ** -24 and M.fm_bound(1.0, -2.0) == 36 * 2.0 ** -24


def test_the_zero_rule_and_the_bound_check():
    rng = np.random.default_rng(3)
    y = (rng.standard_normal(64) + 1j * rng.standard_normal(64)).astype(np.complex64)
    y[10] = 0
    d = M.fm32(y, 0, 0.5)
    assert f32bits(d[[0, 10, 11]]) == [0, 0, 0]                     # stream start, a zero sample, the sample behind it
    r, outside = M.fm_ratio(d, y, 0, 0.5)
    assert not outside.any() and (r <= 1.0).all()
    # the check notices -0.0 and pi in the place of +0.0, a wrong sample, and samples below the bound's range
    bad = d.copy(); bad[10] = -0.0
    assert M.fm_ratio(bad, y, 0, 0.5)[0][10] == np.inf
    bad = d.copy(); bad[20] += np.float32(1e-5)
    assert M.fm_ratio(bad, y, 0, 0.5)[0][20] > 1.0
    with pytest.raises(AssertionError):
        M.fm_check(bad, y, 0, 0.5, "a wrong sample")
    q = (y * np.float32(1e-12)).astype(np.complex64)
    assert M.fm_ratio(M.fm32(q), q)[1][1:10].all()
    with pytest.raises(AssertionError):
        M.fm_check(M.fm32(q), q, 0, 1.0, "quiet")
    # modulo 2 pi |gain|: a product on the negative real axis may land on either side of the cut
    y = np.array([1, -1], np.complex64)
    assert M.fm_ratio(np.array([0, -np.pi], np.float32), y)[0][1] <= 1.0 and M.fm_ratio(np.array([0, np.pi], np.float32), y)[0][1] <= 1.0


def test_the_cut_rule():
    """however a stream is cut into calls that continue one another, the model gives the bits of one call; a call elsewhere starts anew"""
    rng = np.random.default_rng(5)
    lout, nch = [3, 8], 2
    y = [(rng.standard_normal(7 * lo) + 1j * rng.standard_normal(7 * lo)).astype(np.complex64) for lo in lout]
    one = M.fm_stream(M.Carry(nch), [(0, 7, y)], 0.3)[0]
    for cut in ((1,) * 7, (3, 4), (1, 1, 5)):
        calls, b = [], 0
        for n in cut:
            calls.append((b, n, [y[c][b * lout[c]:(b + n) * lout[c]] for c in range(nch)]))
            b += n
        got = M.fm_stream(M.Carry(nch), calls, 0.3)
        for c in range(nch):
            assert f32bits(np.concatenate([g[c] for g in got])) == f32bits(one[c]), (cut, c)
    # a call elsewhere in the stream: its first sample is +0, the rest is the one-call result; and the stream cannot be continued behind a restart
    cr = M.Carry(nch)
    got = M.fm_stream(cr, [(0, 3, [y[c][:3 * lout[c]] for c in range(nch)]), (4, 3, [y[c][4 * lout[c]:] for c in range(nch)])], 0.3)
    for c in range(nch):
        assert f32bits(got[1][c][:1]) == [0] and f32bits(got[1][c][1:]) == f32bits(one[c][4 * lout[c] + 1:])
    assert cr.next == 7
    cr.restart()
    assert cr.front(7).tolist() == [0, 0] and cr.next == -1
    # MAG has no state: any cut of the samples gives the same bits
    assert f32bits(np.concatenate([M.mag32(y[0][:5], 2.0), M.mag32(y[0][5:], 2.0)])) == f32bits(M.mag32(y[0], 2.0))


@pytest.mark.parametrize("n", RUNS)
def test_the_float32_restatement_is_inside_the_bound(n):
    """seeded unit-variance noise, a tone in noise, and a tone next to the negative real axis, at every run length the GPU tests use"""
    rng = np.random.default_rng(n)
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    tone = (np.exp(2j * np.pi * 0.2 * np.arange(n)) * 30).astype(np.complex64) + noise
    edge = np.exp(2j * np.pi * 0.4999999 * np.arange(n)).astype(np.complex64)
    for what, y in (("noise", noise), ("a tone in noise", tone), ("a tone at half the rate", edge)):
        for gain in (1.0, -1 / (2 * np.pi), 1000.0):
            M.fm_check(M.fm32(y, noise[0], gain), y, noise[0], gain, "%s, %d samples, gain %g" % (what, n, gain))


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    ctype = {"fdc_pipeline *p": C.c_void_p, "const fdc_pipeline *p": C.c_void_p, "int32_t mode": C.c_int32, "float gain": C.c_float,
             "int32_t *mode": C.POINTER(C.c_int32), "float *gain": C.POINTER(C.c_float), "const void *d_in": C.c_void_p, "void *d_out": C.c_void_p,
             "const void *d_carry_in": C.c_void_p, "void *d_carry_out": C.c_void_p, "int nblocks": C.c_int, "void *stream": C.c_void_p}
    for name in NAMES:
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int, name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert re.search(r"enum \{ FDC_DEMOD_OFF = 0, FDC_DEMOD_FM = 1, FDC_DEMOD_MAG = 2 \};", hdr)
    assert "(5 + 13 |theta|) 2^-24" in hdr
    assert (G.channelizer.DEMOD_FM, G.channelizer.DEMOD_MAG) == (1, 2)


def test_every_symbol_is_exported():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    # null handles are argument errors, not crashes
    assert lib.fdc_pipeline_set_demod(None, 1, 1.0) == -1
    assert lib.fdc_pipeline_demod(None, None, None) == -1
    assert lib.fdc_pipeline_demod_device(None, 1, 1.0, None, None, None, None, 1, None) == -1
    assert callable(Pipeline.demod_device)
    assert callable(Pipeline.set_demod) and callable(Pipeline.demod)
    assert not hasattr(PipelineGroup, "set_demod")              # there is no group setter


class _Fake(Pipeline):
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]

    def __del__(self):
        pass


@pytest.mark.parametrize("mode, gain", [("am", 1.0), (1, 1.0), ("fm", 0.0), ("fm", np.nan), ("mag", np.inf), ("mag", 1e39), ("FM ", 1.0)])
def test_argument_checks_before_the_library(mode, gain):
    with pytest.raises(ValueError):
        _Fake().set_demod(mode, gain)


def test_the_output_arrays_follow_the_setting():
    p = _Fake()
    assert [o.dtype for o in p._new_outs(3)] == [np.complex64, np.complex64]
    p._demod = G.channelizer.DEMOD_FM
    outs = p._new_outs(3)
    assert [(o.dtype, o.shape) for o in outs] == [(np.float32, (384,)), (np.float32, (192,))]
    assert p._check_outs(outs, 3) is outs
    with pytest.raises(ValueError) as e:
        p._check_outs([np.empty(384, np.complex64), np.empty(192, np.complex64)], 3)
    assert "float32" in str(e.value)
    with pytest.raises(ValueError):
        p._check_outs([np.empty(384, np.float32), np.empty(191, np.float32)], 3)


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)


@pytest.mark.parametrize("change", [
    dict(inpveclen=4096),
    dict(activity_controlled_channels=[[0.2, 0.01]]),
    dict(activity_detection_segments=[[0.1, 0.3]]),
    dict(waterfall=object()),
    dict(iq_output="sc16", iq_output_scale=32768.0),
    dict(demod="am"),
    dict(demod_gain=0.0),
    dict(demod_gain=float("nan")),
], ids=["inpveclen > 1", "power-activation sinks", "detection segments", "waterfall", "iq_output", "unknown mode", "zero gain", "NaN gain"])
def test_hier_block_refusals(change):
    kw = dict(KW, inptype=8, demod="fm")
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "demod" in str(e.value)


def test_demod_is_keyword_only():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    assert par["demod"].kind is inspect.Parameter.KEYWORD_ONLY and par["demod"].default is None
    assert par["demod_gain"].kind is inspect.Parameter.KEYWORD_ONLY and par["demod_gain"].default == 1.0
    assert list(par).index("demod_gain") > list(par).index("demod") > list(par).index("lag1")


@pytest.mark.parametrize("change", [
    dict(inptype=8, demod="fm"),
    dict(inptype=8, demod="mag", demod_gain=-2.0),
    dict(inptype=8, demod="fm", iq_input="sc16", iq_scale=2.0 ** -15),
    dict(inptype=8, demod="fm", demod_gain=1 / (2 * np.pi), fine_tuning=True, levels=True, gains=[2.0], lag1=True),
    dict(inptype=4, demod="mag"),
], ids=["fm", "mag", "integer input", "fine tuning, levels, gains and lag1", "Float input"])
def test_hier_block_acceptances(change):
    """demod combines with the other settings: every check of the constructor is passed and it gets as far as creating the handle, which fails for
    want of a device where there is none"""
    kw = dict(KW)
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.demod == change["demod"] and fdc.pipeline.demod()[0] == change["demod"]
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)
