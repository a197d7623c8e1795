"""CPU tests of complex integer output (no GPU): the Python checks of set_output_format made before any library call, the output-buffer checks,
the hier block's refusals, and the ctypes prototypes of the new C-ABI entries against include/fdc_amd.h."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Fake:
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self, oq=0):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self._oq, self._oq_scale = oq, np.float32(1.0)


@pytest.mark.parametrize("method", [Pipeline.set_output_format, PipelineGroup.set_output_format])
def test_argument_checks_before_the_library(method):
    for fmt in ("sc12", "SC16", "fc64", 1, 0, b"sc16", "complex64"):
        with pytest.raises(ValueError):
            method(_Fake(), fmt)
    for bad in (0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e39, "x", None):      # 1e39: infinite in float32
        with pytest.raises(ValueError):
            method(_Fake(), "sc16", bad)


def test_output_arrays_follow_the_format():
    f = types.SimpleNamespace(lout=[128, 64])
    for code, dt in ((0, np.complex64), (G.IQ_SC16, np.int16), (G.IQ_SC8, np.int8)):
        f._oq = code
        outs = Pipeline._new_outs(f, 3)
        assert [o.dtype for o in outs] == [np.dtype(dt)] * 2
        assert [o.shape for o in outs] == ([(384,), (192,)] if code == 0 else [(384, 2), (192, 2)])
        assert Pipeline._check_outs(f, outs, 3) is outs
    f._oq = G.IQ_SC16
    for bad in ([np.empty(384, np.complex64), np.empty(192, np.complex64)],          # wrong dtype
                [np.empty((384, 2), np.int8), np.empty((192, 2), np.int8)],
                [np.empty((383, 2), np.int16), np.empty((192, 2), np.int16)],        # wrong size
                [np.empty((384, 2), np.int16)],                                      # one per channel
                [np.empty((384, 4), np.int16)[:, :2], np.empty((192, 2), np.int16)]):   # not contiguous
        with pytest.raises(ValueError):
            Pipeline._check_outs(f, bad, 3)
    assert Pipeline._check_outs(f, [np.empty(768, np.int16), np.empty(384, np.int16)], 3) is not None   # flat interleaved is fine


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)


@pytest.mark.parametrize("change", [
    dict(iq_output="sc12"),
    dict(iq_output="fc32"),
    dict(iq_output="sc16", inpveclen=4096),
    dict(iq_output="sc16", activity_controlled_channels=[[0.2, 0.01]]),
    dict(iq_output="sc8", activity_detection_segments=[[0.1, 0.3]]),
    dict(iq_output="sc16", waterfall=object()),
    dict(iq_output="sc16", iq_output_scale=0.0),
    dict(iq_output="sc8", iq_output_scale=float("nan")),
    dict(iq_output="sc16", iq_input="sc16", activity_controlled_channels=[[0.2, 0.01]]),
], ids=["unknown format", "fc32 is not an integer output", "inpveclen > 1", "power-activation sinks", "detection segments", "waterfall", "zero scale",
        "NaN scale", "with iq_input and sinks"])
def test_hier_block_refusals(change):
    kw = dict(KW, inptype=8)
    kw.update(change)
    with pytest.raises(ValueError):
        G.FrequencyDomainChannelizer(**kw)


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    ctype = {"fdc_pipeline *p": C.c_void_p, "fdc_pipeline_group *g": C.c_void_p, "int32_t format": C.c_int32, "float scale": C.c_float}
    for name in ("fdc_pipeline_set_output_format", "fdc_pipeline_group_set_output_format"):
        m = re.search(r"\bint %s\(([^)]*)\);" % name, hdr)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int, name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert re.search(r"FDC_OQ_FC32\s*=\s*0", hdr) and re.search(r"FDC_OQ_SC16\s*=\s*1", hdr) and re.search(r"FDC_OQ_SC8\s*=\s*2", hdr)
    assert G.OQ_FC32 == 0
