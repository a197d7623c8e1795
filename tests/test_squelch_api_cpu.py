"""CPU tests of the channel squelch's host side (no GPU): the ctypes prototypes of the five C-ABI entries against include/fdc_amd.h, null handles, the
Python checks made before any library call, squelch_thresholds, and the hier block's keywords, refusals and acceptances.  (The rule itself:
tests/test_squelch_cpu.py; the device against it, in bytes: tests/test_squelch_gpu.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup
import squelch_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdc_pipeline_set_squelch", "fdc_pipeline_squelch_setting", "fdc_pipeline_squelch", "fdc_pipeline_squelch_device",
         "fdc_pipeline_squelch_pass_device")


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    fp = C.POINTER(C.c_float)
    ctype = {"fdc_pipeline *p": C.c_void_p, "const fdc_pipeline *p": C.c_void_p, "const float *open_thr": fp, "const float *close_thr": fp, "int n": C.c_int,
             "int32_t hang": C.c_int32, "float *open_thr": fp, "float *close_thr": fp, "int32_t *hang": C.POINTER(C.c_int32), "uint8_t *dst": C.c_void_p,
             "size_t capacity_bytes": C.c_size_t, "int nblocks": C.c_int, "const void *d_levels": C.c_void_p, "void *d_mask": C.c_void_p,
             "const void *d_state_in": C.c_void_p, "void *d_state_out": C.c_void_p, "void *stream": C.c_void_p}
    rtype = {"int": C.c_int, "void *": C.c_void_p}
    for name in NAMES:
        m = re.search(r"^(int|void \*)\s?%s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is rtype[m.group(1)], name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert "CHANNEL SQUELCH" in hdr


def test_every_symbol_is_exported_and_null_handles_are_argument_errors():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    thr = (C.c_float * 2)(1, 1)
    assert lib.fdc_pipeline_set_squelch(None, thr, thr, 2, 0) == -1
    assert lib.fdc_pipeline_set_squelch(None, None, None, 0, 0) == -1
    assert lib.fdc_pipeline_squelch_setting(None, None, None, None) == -1
    buf = np.full(16, 7, np.uint8)
    assert lib.fdc_pipeline_squelch(None, buf.ctypes.data, buf.nbytes, 1) == -1 and (buf == 7).all()
    assert lib.fdc_pipeline_squelch_pass_device(None, None, None, None, None, 1, None) == -1
    assert lib.fdc_pipeline_squelch_device(None) is None
    for m in ("set_squelch", "squelch_setting", "squelch", "squelch_device", "squelch_pass_device"):
        assert callable(getattr(Pipeline, m)), m
    assert not hasattr(PipelineGroup, "set_squelch")            # no group setter


class _Fake(Pipeline):
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]

    def __del__(self):
        pass


@pytest.mark.parametrize("open_thr, close_thr, hang", [
    ([1.0], None, 0), ([1.0, 2.0, 3.0], None, 0), ([[1.0, 2.0]], None, 0), (1.0, [1.0], 0),
    (np.nan, None, 0), ([1.0, np.inf], None, 0), (1e39, None, 0), (-1.0, None, 0), (1.0, -0.5, 0), (1.0, np.nan, 0),
    (1.0, 2.0, 0), ([1.0, 2.0], [1.0, 2.5], 0),
    (1.0, None, -1), (1.0, None, 65536), (1.0, None, 1.5), (1.0, None, True), (1.0, None, None)],
    ids=["one value for two channels", "three values", "two dimensions", "one close value", "NaN", "Inf", "beyond float32", "negative", "negative close",
         "NaN close", "close above open", "close above open in one channel", "hang -1", "hang 65536", "hang 1.5", "hang True", "hang None"])
def test_argument_checks_before_the_library(open_thr, close_thr, hang):
    with pytest.raises(ValueError):
        _Fake().set_squelch(open_thr, close_thr, hang)


def test_accepted_arguments():
    f = G.channelizer._squelch_args
    assert f(2, None, "nonsense", -5) == (None, None, 0)                # off: the other arguments are ignored
    o, c, h = f(3, 2.0, None, np.int64(65535))
    assert o.dtype == np.float32 and o.tolist() == [2.0] * 3 and c.tolist() == [2.0] * 3 and h == 65535 and o.flags.c_contiguous
    o, c, h = f(2, [4.0, 0.0], 0.0, 0)
    assert o.tolist() == [4.0, 0.0] and c.tolist() == [0.0, 0.0] and h == 0
    o, c, h = f(0, 1.0, 0.5, 3)                                         # a plan without channels
    assert o.size == 0 and c.size == 0


def test_squelch_thresholds():
    o, c = G.squelch_thresholds([128, 256, 512], -20.0, -23.0)
    mo, mc = S.db_thresholds([128, 256, 512], -20.0, -23.0)
    assert o.tobytes() == mo.tobytes() and c.tobytes() == mc.tobytes() and o.dtype == np.float32
    assert np.allclose(o, [1.28, 2.56, 5.12]) and (c < o).all()
    o, c = G.squelch_thresholds([100, 100], [0.0, 10.0])
    assert o.tolist() == [100.0, 1000.0] and c.tobytes() == o.tobytes()
    with pytest.raises(ValueError):
        G.squelch_thresholds([100], -20.0, -10.0)
    G.channelizer._squelch_args(3, *G.squelch_thresholds([128, 256, 512], -20.0, -23.0), 4)


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)


@pytest.mark.parametrize("change, word", [
    (dict(levels=False), "squelch_db needs levels"),
    (dict(squelch_db=None, squelch_hang=2), "need squelch_db"),
    (dict(squelch_db=None, squelch_close_db=-30.0), "need squelch_db"),
    (dict(squelch_close_db=-10.0), "close"),
    (dict(squelch_db=np.nan), "finite"),
    (dict(squelch_hang=-1), "hang"),
    (dict(squelch_hang=70000), "hang"),
    (dict(squelch_db=[-20.0, -20.0]), ""),
    (dict(devices=[0, 0]), "one device"),
    (dict(inpveclen=4096), "levels"),
    (dict(waterfall=object()), "levels"),
], ids=["without levels", "hang without db", "close without db", "close above open", "NaN", "hang -1", "hang 70000", "two values for one channel",
        "two devices", "inpveclen > 1", "waterfall"])
def test_hier_block_refusals(change, word):
    kw = dict(KW, inptype=8, levels=True, squelch_db=-20.0)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert word in str(e.value)


def test_the_keywords_are_keyword_only():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    for name, default in (("squelch_db", None), ("squelch_close_db", None), ("squelch_hang", 0)):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default == default, name
    assert list(par).index("squelch_db") > list(par).index("audio_scale")
    assert callable(G.FrequencyDomainChannelizer.set_squelch)


@pytest.mark.parametrize("change", [
    dict(inptype=8, levels=True, squelch_db=-20.0),
    dict(inptype=8, levels=True, squelch_db=[-20.0], squelch_close_db=-26.0, squelch_hang=3, demod="fm", audio_decim=4, audio_taps=G.lowpass_taps(4, 16)),
    dict(inptype=4, levels=True, squelch_db=-3.0, squelch_hang=65535, fine_tuning=True, gains=[2.0], lag1=True),
], ids=["levels alone", "with the audio", "Float input with the other settings"])
def test_hier_block_acceptances(change):
    """every check of the constructor is passed and it gets as far as creating the handle, which fails for want of a device where there is none"""
    kw = dict(KW)
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.pipeline.squelch_setting()[2] == change.get("squelch_hang", 0)
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)
