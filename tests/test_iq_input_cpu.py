"""CPU tests of complex integer input (no GPU): the Python checks that run before any library call, the hier block's refusals, and the
ctypes prototypes of the new C-ABI entries against include/fdc_amd.h."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup, iq_format

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake(H=2048):
    # a handle-less stand-in: the checks below must raise before anything touches the library or the handle
    return types.SimpleNamespace(H=H, N=4096, ovl=4096 - H, lout=[128], _h=None)


def test_dtype_selects_the_format():
    assert iq_format(np.zeros(4, np.int16)) == G.IQ_SC16 == 1
    assert iq_format(np.zeros(4, np.int8)) == G.IQ_SC8 == 2
    for dt in (np.float32, np.complex64, np.uint8, np.uint16, np.int32):
        with pytest.raises(TypeError):
            iq_format(np.zeros(4, dt))


@pytest.mark.parametrize("method", [Pipeline.work_iq, PipelineGroup.work_iq])
def test_argument_checks_before_the_library(method):
    f = fake()
    with pytest.raises(TypeError):
        method(f, np.zeros(2 * 2048, np.float32))
    with pytest.raises(TypeError):
        method(f, np.zeros(2 * 2048, np.uint8))
    with pytest.raises(TypeError):
        method(f, [0] * 4096)
    with pytest.raises(ValueError):
        method(f, np.zeros((2048, 3), np.int16))        # (n, 2) only
    with pytest.raises(ValueError):
        method(f, np.zeros((2, 2048, 2), np.int16))
    with pytest.raises(ValueError):
        method(f, np.zeros(2 * 2048 + 1, np.int16))     # odd interleaved length
    with pytest.raises(ValueError):
        method(f, np.zeros(2 * 2047, np.int16))         # not a whole number of items
    for bad in (0.0, float("nan"), float("inf"), -float("inf"), 1e39):      # 1e39: infinite in float32
        with pytest.raises(ValueError):
            method(f, np.zeros(2 * 2048, np.int16), scale=bad)


def test_process_device_iq_format_names():
    with pytest.raises(ValueError):
        Pipeline.process_device_iq(fake(), "u8", 1.0, 0, 0, 1, 0)
    with pytest.raises(ValueError):
        Pipeline.process_device_iq(fake(), 3, 1.0, 0, 0, 1, 0)


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)


@pytest.mark.parametrize("change", [
    dict(iq_input="sc12"),
    dict(iq_input="sc16", inpveclen=4096),
    dict(iq_input="sc16", activity_controlled_channels=[[0.2, 0.01]]),
    dict(iq_input="sc8", activity_detection_segments=[[0.1, 0.3]]),
    dict(iq_input="sc16", waterfall=object()),
    dict(iq_input="sc16", iq_scale=0.0),
    dict(iq_input="sc8", iq_scale=float("nan")),
    dict(iq_input="sc16", inptype=4),
], ids=["unknown format", "inpveclen > 1", "power-activation sinks", "detection segments", "waterfall", "zero scale", "NaN scale", "float input type"])
def test_hier_block_refusals(change):
    kw = dict(KW, inptype=8)
    kw.update(change)
    with pytest.raises(ValueError):
        G.FrequencyDomainChannelizer(**kw)


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    ctype = {"fdc_pipeline *": C.c_void_p, "fdc_pipeline_group *": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float, "const void *": C.c_void_p,
             "int": C.c_int, "int64_t": C.c_int64, "void *const *": C.POINTER(C.c_void_p), "void *": C.c_void_p}
    for name in ("fdc_pipeline_work_iq", "fdc_pipeline_work_span_iq", "fdc_pipeline_process_device_iq", "fdc_pipeline_group_work_iq"):
        m = re.search(r"\bint %s\(([^)]*)\);" % name, hdr)
        assert m, name
        args = [re.sub(r"\b\w+$", "", a.strip()).strip() for a in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int, name
        assert len(argtypes) == len(args), (name, args)
        for a, t in zip(args, argtypes):
            assert ctype[a] == t, (name, a, t)
    assert re.search(r"FDC_IQ_SC16\s*=\s*1", hdr) and re.search(r"FDC_IQ_SC8\s*=\s*2", hdr)
