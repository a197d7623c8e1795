"""CPU tests of the channel levels (no GPU): the numpy model of the definition (what the GPU tests compare the device with) on hand-made rows, the
Python checks made before any library call, the hier block's refusals and acceptances, and the ctypes prototypes of the five C-ABI entries against
include/fdc_amd.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdc_pipeline_set_levels", "fdc_pipeline_levels", "fdc_pipeline_levels_device", "fdc_pipeline_group_set_levels", "fdc_pipeline_group_levels")


def model(y, lout):
    """The definition on one channel's float32 samples (complex64, nblocks * lout of them): per block the float64 sum of squares of the float32 components
    (P64) and the float32 maximum of their absolute values with fmax semantics.  Returns (P64[nblocks], peak[nblocks])."""
    v = np.ascontiguousarray(y, np.complex64).view(np.float32).reshape(-1, 2 * lout)
    with np.errstate(invalid="ignore", over="ignore"):
        p64 = (v.astype(np.float64) ** 2).sum(axis=1)
        peak = np.fmax.reduce(np.abs(v), axis=1)
    return p64, peak


def power_bound(lout):
    """|power - P64| <= (lout + 8) 2^-24 P64: a term has at most three roundings, any-order float32 summation of n non-negative terms is within
    (n - 1) 2^-24 / (1 - (n - 1) 2^-24) (DESIGN.md "Channel levels")"""
    return (lout + 8) * 2.0 ** -24


def agrees(lev, y, lout, what):
    """one channel of a call: lev = float32[nblocks, 2] from the device, y the samples the same call returned.  Prints the figure before it asserts."""
    p64, peak = model(y, lout)
    assert lev.shape == (p64.size, 2) and lev.dtype == np.float32, (what, lev.shape, lev.dtype)
    err = np.abs(lev[:, 0].astype(np.float64) - p64)
    worst = float((err / np.where(p64 > 0, p64, 1.0)).max()) / power_bound(lout)
    print("%s: lout %d, largest power error %.3g of its bound" % (what, lout, worst))
    assert (err <= power_bound(lout) * p64).all(), (what, int(np.argmax(err - power_bound(lout) * p64)))
    assert lev[:, 1].tobytes() == peak.astype(np.float32).tobytes(), (what, lev[:, 1], peak)


def test_model_on_hand_made_rows():
    p, k = model(np.zeros(4, np.complex64), 4)
    assert p.tolist() == [0.0] and k.tolist() == [0.0] and k.dtype == np.float32
    p, k = model(np.array([3 - 4j], np.complex64), 1)
    assert p.tolist() == [25.0] and k.tolist() == [4.0]
    # a row with -0.0: |-0.0| = 0.0, the sum stays +0.0 and the peak is +0.0 (not -0.0)
    row = np.array([complex(-0.0, 0.0), complex(0.0, -0.0)], np.complex64)
    p, k = model(row, 2)
    assert p.tolist() == [0.0] and k.tobytes() == np.float32(0.0).tobytes()
    # two blocks of three samples; fmax passes a NaN component over, the sum does not
    y = np.array([1 + 1j, 2 - 0.5j, -3j, complex(np.nan, 2.0), 0.25, -7 + 1j], np.complex64)
    p, k = model(y, 3)
    assert p[0] == 1 + 1 + 4 + 0.25 + 9 and np.isnan(p[1])
    assert k.tolist() == [3.0, 7.0]
    # a row of NaN only keeps NaN; infinity is a value like any other
    p, k = model(np.array([complex(np.nan, np.nan), complex(np.inf, -1.0)], np.complex64), 1)
    assert np.isnan(k[0]) and k[1] == np.inf and p[1] == np.inf
    # the float32 components are squared and summed in float64: 2^-80 does not vanish
    p, _ = model(np.array([complex(2.0 ** -40, 0.0)], np.complex64), 1)
    assert p[0] == 2.0 ** -80
    assert power_bound(128) == 136 * 2.0 ** -24


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
    assert "peak * |scale| >= 32767.5 (sc16) or >= 127.5 (sc8) means some component of that row saturated in the narrowing" in hdr


def test_every_symbol_is_exported():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    # null handles are argument errors, not crashes
    assert lib.fdc_pipeline_set_levels(None, 1) == -1
    assert lib.fdc_pipeline_levels(None, None, 0) == -1
    assert lib.fdc_pipeline_levels_device(None) is None
    assert lib.fdc_pipeline_group_set_levels(None, 1) == -1
    assert lib.fdc_pipeline_group_levels(None, None, 0) == -1
    for cls in (Pipeline, PipelineGroup):
        assert callable(cls.set_levels) and callable(cls.levels)
    assert callable(Pipeline.levels_device)


class _Fake:
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]
        self._last_nb = None


@pytest.mark.parametrize("method", [Pipeline.levels, PipelineGroup.levels])
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
    kw = dict(KW, inptype=8, levels=True)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "levels" in str(e.value)


def test_levels_is_keyword_only():
    import inspect
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    assert par["levels"].kind is inspect.Parameter.KEYWORD_ONLY and par["levels"].default is False
    assert list(par).index("levels") > list(par).index("payload_scale")


@pytest.mark.parametrize("change", [
    dict(inptype=8),
    dict(inptype=8, iq_output="sc16", iq_output_scale=32768.0),
    dict(inptype=8, iq_input="sc16", iq_scale=2.0 ** -15, iq_output="sc8", iq_output_scale=100.0),
    dict(inptype=8, fine_tuning=True),
    dict(inptype=4),
], ids=["alone", "sc16 output", "integer in and out", "fine tuning", "Float input"])
def test_hier_block_acceptances(change):
    """levels=True combines with the other settings: every check of the constructor is passed and it gets as far as creating the handle, which fails for
    want of a device where there is none"""
    kw = dict(KW, levels=True)
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.levels_on and fdc.levels is None
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)
