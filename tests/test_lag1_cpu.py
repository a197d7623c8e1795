"""CPU tests of the channel lag-1 correlation (no GPU): the two numpy models of tests/lag1_model.py on hand-made rows, the float32 model inside the bound
of the float64 model at every row length the GPU tests use, lag1_frequency, the Python checks made before any library call, the hier block's refusals and
acceptances, and the ctypes prototypes of the five C-ABI entries against include/fdc_amd.h."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup
from lag1_model import LOUTS, agrees, bound, lanes_log2, model32, model64, ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdc_pipeline_set_lag1", "fdc_pipeline_lag1", "fdc_pipeline_lag1_device", "fdc_pipeline_group_set_lag1", "fdc_pipeline_group_lag1")


def c64(*v):
    return np.array(v, np.complex64)


def bits(s):
    return np.ascontiguousarray(s, np.complex64).view(np.uint32).tolist()


def test_models_on_hand_made_rows():
    # lout = 1: no term, (+0, +0); two rows
    s64, m = model64(c64(3 - 4j, 1j), 1)
    assert s64.tolist() == [0, 0] and m.tolist() == [0, 0]
    assert bits(model32(c64(3 - 4j, 1j), 1)) == [0, 0, 0, 0]
    # lout = 2: the second term of pair 0 only: y[1] conj(y[0]) = (1 + 2j)(3 + 4j) = -5 + 10j
    y = c64(3 - 4j, 1 + 2j)
    assert model64(y, 2)[0].tolist() == [-5 + 10j] and model64(y, 2)[1].tolist() == [5.0 * np.sqrt(5.0)]
    assert model32(y, 2).tolist() == [-5 + 10j]
    # lout = 3: pair 1 has its first term and not its second.  y[1] conj(y[0]) + y[2] conj(y[1]) = (-5 + 10j) + (2j)(1 - 2j) = -1 + 12j
    y = c64(3 - 4j, 1 + 2j, 2j)
    assert model64(y, 3)[0].tolist() == [-1 + 12j] and model32(y, 3).tolist() == [-1 + 12j]
    # a constant row: lout - 1 times |y|^2, no imaginary part
    y = np.full(12, 2 - 1j, np.complex64)
    assert model64(y, 12)[0].tolist() == [55 + 0j] and model32(y, 12).tolist() == [55 + 0j] and model64(y, 12)[1].tolist() == [pytest.approx(55.0)]
    # the block boundary is not crossed: two rows of 6 give 2 x 5 terms, not 11
    assert model64(y, 6)[0].tolist() == [25, 25] and model32(y, 6).tolist() == [25, 25]
    # a pure tone: arg S = 2 pi nu, |S| = lout - 1
    for lout, nu in ((16, 0.125), (240, -0.31), (768, 0.004)):
        y = np.exp(2j * np.pi * nu * np.arange(lout)).astype(np.complex64)
        for s in (model64(y, lout)[0], model32(y, lout)):
            assert abs(np.angle(s[0]) / (2 * np.pi) - nu) < 1e-6 and abs(abs(s[0]) - (lout - 1)) < 1e-3 * lout, (lout, nu, s)
    # NaN and +-Inf: what IEEE arithmetic gives, in the row that holds them and in no other
    y = c64(1, 1j, complex(np.nan, 0), 2, 1, 1j, -1, -1j)
    for s in (model64(y, 4)[0], model32(y, 4)):
        assert np.isnan(s[0].real) and np.isnan(s[0].imag) and s[1] == 3j
    y = c64(1, complex(np.inf, 0), 1, 1, 1, complex(0, -np.inf), 0, 1)
    for s in (model64(y, 4)[0], model32(y, 4)):
        assert s[0].real == np.inf and np.isnan(s[0].imag)          # Inf * 0 in the cross products
        assert np.isnan(s[1].real) and np.isnan(s[1].imag)          # -Inf * 0
    assert bound(128) == 136 * 2.0 ** -24
    assert [lanes_log2(lo) for lo in (1, 2, 3, 4, 8, 12, 15, 128, 129, 24576)] == [0, 0, 1, 1, 2, 3, 3, 6, 6, 6]


def test_the_float32_model_follows_the_stated_order():
    """model32 against a scalar restatement of the order, one row at a time: lanes, pairs, the two terms of a pair, the butterfly"""
    rng = np.random.default_rng(7)
    f = np.float32
    for lout in (1, 2, 3, 7, 8, 12, 15, 128, 130, 192, 259, 768):
        y = (rng.standard_normal(lout) + 1j * rng.standard_normal(lout)).astype(np.complex64)
        lanes = 1 << lanes_log2(lout)
        acc = [[f(0), f(0)] for _ in range(lanes)]

        def add(a, k, b):
            ax, ay, bx, by = f(y[k].real), f(y[k].imag), f(y[b].real), f(y[b].imag)
            a[0] = f(a[0] + f(f(ax * bx) + f(ay * by)))
            a[1] = f(a[1] + f(f(ay * bx) - f(ax * by)))
        for i in range((lout + 1) // 2):
            if i >= 1:
                add(acc[i % lanes], 2 * i, 2 * i - 1)
            if 2 * i + 1 < lout:
                add(acc[i % lanes], 2 * i + 1, 2 * i)
        d = 1
        while d < lanes:
            acc = [[f(acc[k][0] + acc[k ^ d][0]), f(acc[k][1] + acc[k ^ d][1])] for k in range(lanes)]
            d <<= 1
        assert bits(model32(y, lout)) == bits(np.complex64(complex(acc[0][0], acc[0][1]))), lout


@pytest.mark.parametrize("lout", LOUTS)
def test_the_float32_model_is_inside_the_bound(lout):
    """seeded random rows, tones in noise and rows whose terms cancel (white noise: |S| far below M), at every row length the GPU tests use"""
    rng = np.random.default_rng(lout)
    nrows = 64 if lout <= 1024 else 4
    noise = (rng.standard_normal(nrows * lout) + 1j * rng.standard_normal(nrows * lout)).astype(np.complex64)
    tone = (np.exp(2j * np.pi * 0.2 * np.arange(nrows * lout)) * 30).astype(np.complex64) + noise
    for what, y in (("noise", noise), ("a tone in noise", tone), ("loud", noise * np.float32(1e12)), ("quiet", noise * np.float32(1e-12))):
        r = ratio(model32(y, lout), y, lout)
        print("%s, lout %d: the float32 model's largest error is %.3g of the bound" % (what, lout, r.max()))
        assert (r <= 1.0).all(), (what, lout, r.max())
        agrees(model32(y, lout), y, lout, what)


def test_lag1_frequency():
    nu = np.array([[0.25, -0.25, 0.0], [0.4999, -0.1, 1e-9]])
    s = (3.0 * np.exp(2j * np.pi * nu)).astype(np.complex128)
    f = G.lag1_frequency(s)
    assert f.dtype == np.float64 and f.shape == nu.shape and np.abs(f - nu).max() < 1e-15
    assert G.lag1_frequency(np.complex64(1j)) == 0.25 and G.lag1_frequency(np.zeros(3, np.complex64)).tolist() == [0, 0, 0]
    assert G.lag1_frequency([1 + 0j, -1j]).tolist() == [0.0, -0.25]
    # in the unit of set_fine_tuning: a tone nu above the centre, turned by exp(-2 pi i nu t), is left with nothing
    y = np.exp(2j * np.pi * 0.03 * np.arange(64))
    est = G.lag1_frequency(model64(y.astype(np.complex64), 64)[0][0])
    turned = (y * np.exp(-2j * np.pi * est * np.arange(64))).astype(np.complex64)
    assert abs(est - 0.03) < 1e-7 and abs(G.lag1_frequency(model64(turned, 64)[0][0])) < 1e-7


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    ctype = {"fdc_pipeline *p": C.c_void_p, "fdc_pipeline_group *g": C.c_void_p, "int32_t on": C.c_int32, "float *dst": C.POINTER(C.c_float),
             "int nblocks": C.c_int}
    for name in NAMES:
        ret = "void \\*" if name.endswith("_device") else "int "
        m = re.search(r"^%s%s\(([^)]*)\);" % (ret, name), hdr, re.M)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is (C.c_void_p if name.endswith("_device") else C.c_int), name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert "S[m][c] = sum_{j = 1 .. lout_c - 1}  y[j] conj(y[j - 1])" in hdr and "(lout_c + 8) 2^-24 M" in hdr


def test_every_symbol_is_exported():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    # null handles are argument errors, not crashes
    assert lib.fdc_pipeline_set_lag1(None, 1) == -1
    assert lib.fdc_pipeline_lag1(None, None, 0) == -1
    assert lib.fdc_pipeline_lag1_device(None) is None
    assert lib.fdc_pipeline_group_set_lag1(None, 1) == -1
    assert lib.fdc_pipeline_group_lag1(None, None, 0) == -1
    for cls in (Pipeline, PipelineGroup):
        assert callable(cls.set_lag1) and callable(cls.lag1)
    assert callable(Pipeline.lag1_device)


class _Fake:
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]
        self._last_nb = None


@pytest.mark.parametrize("method", [Pipeline.lag1, PipelineGroup.lag1])
def test_argument_checks_before_the_library(method):
    with pytest.raises(ValueError):
        method(_Fake())                       # no call yet
    with pytest.raises(ValueError):
        method(_Fake(), -1)


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)


@pytest.mark.parametrize("change", [
    dict(inpveclen=4096),
    dict(activity_controlled_channels=[[0.2, 0.01]]),
    dict(activity_detection_segments=[[0.1, 0.3]]),
    dict(waterfall=object()),
], ids=["inpveclen > 1", "power-activation sinks", "detection segments", "waterfall"])
def test_hier_block_refusals(change):
    kw = dict(KW, inptype=8, lag1=True)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "lag1" in str(e.value)


def test_lag1_is_keyword_only():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    assert par["lag1"].kind is inspect.Parameter.KEYWORD_ONLY and par["lag1"].default is False
    assert list(par).index("lag1") > list(par).index("gains")


@pytest.mark.parametrize("change", [
    dict(inptype=8),
    dict(inptype=8, iq_output="sc16", iq_output_scale=32768.0),
    dict(inptype=8, iq_input="sc16", iq_scale=2.0 ** -15, iq_output="sc8", iq_output_scale=100.0),
    dict(inptype=8, fine_tuning=True, levels=True, gains=[2.0]),
    dict(inptype=4),
], ids=["alone", "sc16 output", "integer in and out", "fine tuning, levels and gains", "Float input"])
def test_hier_block_acceptances(change):
    """lag1=True combines with the other settings: every check of the constructor is passed and it gets as far as creating the handle, which fails for
    want of a device where there is none"""
    kw = dict(KW, lag1=True)
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.lag1_on and fdc.lag1 is None
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)
