"""CPU tests of the tone squelch's host side (no GPU): the ctypes prototypes of the five C-ABI entries against include/fdc_amd.h, null handles, the
Python checks made before any library call, the helper tone_squelch_thresholds, and the hier block's keywords, refusals and acceptances.  (The
definition: tests/test_tone_squelch_cpu.py; the device against it, in bytes: tests/test_tone_squelch_gpu.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdc_pipeline_set_tone_squelch", "fdc_pipeline_tone_squelch_setting", "fdc_pipeline_tone_squelch", "fdc_pipeline_tone_squelch_device",
         "fdc_pipeline_tone_squelch_pass_device")


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ctype = {"fdc_pipeline *p": C.c_void_p, "const fdc_pipeline *p": C.c_void_p, "const int32_t *tone": i32, "int32_t *tone": i32,
             "const float *open_thr": f32, "const float *close_thr": f32, "const float *ratio": f32, "float *open_thr": f32, "float *close_thr": f32,
             "float *ratio": f32, "int n": C.c_int, "int32_t guard": C.c_int32, "int32_t hang_frames": C.c_int32, "int32_t *guard": i32,
             "int32_t *hang_frames": i32, "uint8_t *dst": C.c_void_p, "size_t capacity_bytes": C.c_size_t, "int nblocks": C.c_int, "int32_t *nframes": i32,
             "const void *d_frames": C.c_void_p, "void *d_dec": C.c_void_p, "const void *d_state_in": C.c_void_p, "void *d_state_out": C.c_void_p,
             "void *d_mask": C.c_void_p, "int32_t fill": C.c_int32, "void *stream": C.c_void_p}
    rtype = {"int": C.c_int, "void *": C.c_void_p}
    for name in NAMES:
        m = re.search(r"^(int|void \*)\s?%s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is rtype[m.group(1)], name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert "TONE SQUELCH" in hdr and "COMBINED mask" in hdr          # fdc_pipeline_squelch's change of meaning is said there


def test_every_symbol_is_exported_and_null_handles_are_argument_errors():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    t = (C.c_int32 * 2)(0, 0)
    f = (C.c_float * 2)(1.0, 1.0)
    assert lib.fdc_pipeline_set_tone_squelch(None, t, f, f, f, 2, 0, 0) == -1
    assert lib.fdc_pipeline_set_tone_squelch(None, None, None, None, None, 0, 0, 0) == -1
    g, h = C.c_int32(-7), C.c_int32(-7)
    assert lib.fdc_pipeline_tone_squelch_setting(None, None, None, None, None, C.byref(g), C.byref(h)) == -1 and (g.value, h.value) == (-7, -7)
    buf = np.full(16, 7, np.uint8)
    nf = C.c_int32(-3)
    assert lib.fdc_pipeline_tone_squelch(None, buf.ctypes.data, buf.nbytes, 1, C.byref(nf)) == -1 and (buf == 7).all() and nf.value == -3
    assert lib.fdc_pipeline_tone_squelch_pass_device(None, None, None, None, None, None, 0, 1, None) == -1
    assert lib.fdc_pipeline_tone_squelch_device(None) is None
    for m in ("set_tone_squelch", "tone_squelch_setting", "tone_squelch", "tone_squelch_device", "tone_squelch_pass_device"):
        assert callable(getattr(Pipeline, m)), m
    assert not hasattr(PipelineGroup, "set_tone_squelch")              # no group setter
    assert callable(G.tone_squelch_thresholds)


class _Fake(Pipeline):
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]

    def __del__(self):
        pass


@pytest.mark.parametrize("kw", [
    dict(tone=[0, 1, 2], open_thr=1.0), dict(tone=[0.0, 1.0], open_thr=1.0), dict(tone=[[0, 1]], open_thr=1.0), dict(tone=-2, open_thr=1.0),
    dict(tone=64, open_thr=1.0), dict(tone=0), dict(tone=0, open_thr=[1.0, 2.0, 3.0]), dict(tone=0, open_thr=np.nan), dict(tone=0, open_thr=np.inf),
    dict(tone=0, open_thr=1e39), dict(tone=0, open_thr=-1.0), dict(tone=0, open_thr=1.0, close_thr=2.0), dict(tone=0, open_thr=1.0, close_thr=-0.5),
    dict(tone=0, open_thr=1.0, ratio=-1.0), dict(tone=0, open_thr=1.0, ratio=np.nan), dict(tone=0, open_thr=1.0, ratio=[1.0]),
    dict(tone=0, open_thr=1.0, guard=-1), dict(tone=0, open_thr=1.0, guard=64), dict(tone=0, open_thr=1.0, guard=1.0), dict(tone=0, open_thr=1.0, guard=True),
    dict(tone=0, open_thr=1.0, hang=-1), dict(tone=0, open_thr=1.0, hang=65536), dict(tone=0, open_thr=1.0, hang=None)],
    ids=["three tones for two channels", "float tones", "two dimensions", "tone -2", "tone 64", "no thresholds", "three thresholds", "NaN", "Inf",
         "beyond float32", "negative", "close above open", "negative close", "negative ratio", "NaN ratio", "one ratio for two", "guard -1", "guard 64",
         "guard 1.0", "guard True", "hang -1", "hang 65536", "hang None"])
def test_argument_checks_before_the_library(kw):
    with pytest.raises(ValueError):
        _Fake().set_tone_squelch(**kw)


def test_accepted_arguments():
    f = G.channelizer._tone_squelch_args
    assert f(2, None, "nonsense", None, -5, "x", None) == (None, None, None, None, 0, 0)        # off: the other arguments are ignored
    t, o, c, r, g, h = f(3, 5, 2.0, None, 0.0, 63, 65535)                                       # scalars broadcast, close defaults to open
    assert t.dtype == np.int32 and t.tolist() == [5] * 3 and o.dtype == np.float32 and o.tolist() == [2.0] * 3 and c.tolist() == [2.0] * 3
    assert r.tolist() == [0.0] * 3 and (g, h) == (63, 65535) and all(a.flags.c_contiguous for a in (t, o, c, r))
    t, o, c, r, g, h = f(2, np.array([-1, 63]), [4.0, 0.0], [4.0, 0.0], np.float64(2.5), np.int64(0), 0)
    assert t.tolist() == [-1, 63] and o.tolist() == [4.0, 0.0] and c.tolist() == [4.0, 0.0] and r.tolist() == [2.5, 2.5]
    t, o, c, r, g, h = f(0, np.zeros(0, np.int32), 1.0, None, 0.0, 0, 0)                        # a plan without channels
    assert t.shape == (0,) and o.shape == (0,)


def test_the_helper():
    # the |Z|^2 of a tone of that amplitude: tone_amplitude inverts it exactly
    r, S, W, lout = 25000.0, 16, 4, 128
    f = G.ctcss_tones()[:8]
    thr = G.tone_squelch_thresholds(0.25, lout, W, S, f, r)
    assert thr.dtype == np.float32 and thr.shape == (8,)
    assert np.allclose(G.tone_amplitude(np.sqrt(thr.astype(np.float64)), W * lout, f, r, S), 0.25, rtol=1e-6)
    assert G.tone_squelch_thresholds(2.0, 10, 1, 1, 0.0, r) == np.float32((2.0 * 10 / 2.0) ** 2)           # f = 0: no droop
    per = G.tone_squelch_thresholds([0.1, 0.2], [128, 64], W, S, 100.0, r)                                 # one value per channel
    assert per.shape == (2,) and np.isclose(per[0] / per[1], (0.1 * 128) ** 2 / (0.2 * 64) ** 2)
    assert G.tone_squelch_thresholds(0.0, lout, W, S, 100.0, r) == 0.0
    for bad in (lambda: G.tone_squelch_thresholds(-1.0, lout, W, S, 100.0, r), lambda: G.tone_squelch_thresholds(np.nan, lout, W, S, 100.0, r),
                lambda: G.tone_squelch_thresholds(1.0, lout, W, S, 100.0, 0.0)):
        with pytest.raises(ValueError):
            bad()


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)
INC = np.arange(1, 6, dtype=np.uint32)
ON = dict(inptype=8, demod="fm", tones=INC, levels=True, squelch_db=-3.0, tone_squelch=2, tone_open=4.0)


@pytest.mark.parametrize("change, word", [
    (dict(tones=None), "needs tones and squelch_db"),
    (dict(squelch_db=None), "needs tones and squelch_db"),
    (dict(tone_squelch=5), "selects tone 5 of 5"),
    (dict(tone_squelch=-2), "-1 .. 63"),
    (dict(tone_squelch=[0, 1]), "one per channel"),
    (dict(tone_open=None), "open thresholds"),
    (dict(tone_close=5.0), "close threshold"),
    (dict(tone_ratio=-1.0), "not negative"),
    (dict(tone_guard=64), "guard"),
    (dict(tone_hang=70000), "hang"),
    (dict(tone_squelch=None), "need tone_squelch"),
    (dict(tone_squelch=None, tone_open=None, tone_hang=2), "need tone_squelch"),
], ids=["without tones", "without squelch_db", "tone 5 of 5", "tone -2", "two tones for one channel", "no open threshold", "close above open",
        "negative ratio", "guard 64", "hang 70000", "thresholds without tone_squelch", "hang without tone_squelch"])
def test_hier_block_refusals(change, word):
    kw = dict(KW, **ON)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert word in str(e.value)


def test_the_keywords_are_keyword_only():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    for name, default in (("tone_squelch", None), ("tone_open", None), ("tone_close", None), ("tone_ratio", 0.0), ("tone_guard", 0), ("tone_hang", 0)):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default == default, name
    assert list(par).index("tone_squelch") > list(par).index("tone_frame")


@pytest.mark.parametrize("change", [
    dict(),
    dict(tone_squelch=[-1], tone_close=1.0, tone_ratio=2.0, tone_guard=1, tone_hang=3, audio_decim=4, audio_taps=G.lowpass_taps(4, 16), audio_packed=True),
], ids=["the least", "with the packed audio"])
def test_hier_block_acceptances(change):
    """every check of the constructor is passed and it gets as far as creating the handle, which fails for want of a device where there is none"""
    kw = dict(KW, **ON)
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.pipeline.tone_squelch_setting()[4:] == (change.get("tone_guard", 0), change.get("tone_hang", 0))
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)
