"""CPU tests of the channel audio's host side (no GPU): the ctypes prototypes of the six C-ABI entries against include/fdc_amd.h, null handles, the
Python checks made before any library call, the hier block's keywords, refusals and acceptances, and the slicing of the block-major audio matrix into
channels against tests/audio_model.py.  (The model itself is held to its bound by tests/test_audio_cpu.py; the device pass to the model, in bits, by
tests/test_audio_gpu.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup
import audio_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdc_pipeline_set_audio", "fdc_pipeline_audio_setting", "fdc_pipeline_audio_row", "fdc_pipeline_audio", "fdc_pipeline_audio_device",
         "fdc_pipeline_audio_pass_device")


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    ctype = {"fdc_pipeline *p": C.c_void_p, "const fdc_pipeline *p": C.c_void_p, "int32_t decim": C.c_int32, "const float *taps": C.POINTER(C.c_float),
             "int32_t ntaps": C.c_int32, "int32_t format": C.c_int32, "float scale": C.c_float, "int32_t *decim": C.POINTER(C.c_int32),
             "int32_t *ntaps": C.POINTER(C.c_int32), "int32_t *format": C.POINTER(C.c_int32), "float *scale": C.POINTER(C.c_float),
             "float *taps": C.POINTER(C.c_float), "void *dst": C.c_void_p, "size_t capacity_bytes": C.c_size_t, "int nblocks": C.c_int,
             "const void *d_in": C.c_void_p, "void *d_out": C.c_void_p, "const void *d_hist_in": C.c_void_p, "void *d_hist_out": C.c_void_p,
             "void *stream": C.c_void_p}
    rtype = {"int": C.c_int, "int64_t": C.c_int64, "void *": C.c_void_p}
    for name in NAMES:
        m = re.search(r"^(int|int64_t|void \*)\s?%s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is rtype[m.group(1)], name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert re.search(r"enum \{ FDC_AUDIO_F32 = 0, FDC_AUDIO_S16 = 1 \};", hdr)
    assert (G.AUDIO_F32, G.AUDIO_S16) == (0, 1)


def test_every_symbol_is_exported_and_null_handles_are_argument_errors():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    taps = (C.c_float * 4)(1, 0, 0, 0)
    assert lib.fdc_pipeline_set_audio(None, 2, taps, 4, 0, 1.0) == -1
    assert lib.fdc_pipeline_set_audio(None, 0, None, 0, 0, 1.0) == -1
    assert lib.fdc_pipeline_audio_setting(None, None, None, None, None, None) == -1
    buf = np.full(16, 7, np.uint8)
    assert lib.fdc_pipeline_audio(None, buf.ctypes.data, buf.nbytes, 1) == -1 and (buf == 7).all()
    assert lib.fdc_pipeline_audio_pass_device(None, None, None, None, None, 1, None) == -1
    assert lib.fdc_pipeline_audio_row(None) == 0 and lib.fdc_pipeline_audio_device(None) is None
    for m in ("set_audio", "audio_setting", "audio", "audio_device", "audio_pass_device"):
        assert callable(getattr(Pipeline, m)), m
    assert not hasattr(PipelineGroup, "set_audio")              # no group setter: the group entries do not serve the demodulation


class _Fake(Pipeline):
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]

    def __del__(self):
        pass


GOOD = np.ones(8, np.float32)


@pytest.mark.parametrize("decim, taps, fmt, scale", [
    (0, GOOD, "f32", 1.0), (65, GOOD, "f32", 1.0), (1.5, GOOD, "f32", 1.0), (True, GOOD, "f32", 1.0), (-1, GOOD, "f32", 1.0),
    (4, np.zeros(0, np.float32), "f32", 1.0), (4, np.ones(257, np.float32), "f32", 1.0), (4, None, "f32", 1.0),
    (4, [1.0, np.nan], "f32", 1.0), (4, [np.inf], "f32", 1.0), (4, [1e39], "f32", 1.0),
    (4, GOOD, "s8", 1.0), (4, GOOD, 1, 1.0), (4, GOOD, None, 1.0),
    (4, GOOD, "s16", 0.0), (4, GOOD, "s16", np.nan), (4, GOOD, "s16", np.inf), (4, GOOD, "s16", 1e39)],
    ids=["decim 0", "decim 65", "decim 1.5", "decim True", "decim -1", "no taps", "257 taps", "taps None", "NaN tap", "Inf tap", "a tap beyond float32",
         "format s8", "format 1", "format None", "scale 0", "scale NaN", "scale Inf", "scale beyond float32"])
def test_argument_checks_before_the_library(decim, taps, fmt, scale):
    with pytest.raises(ValueError):
        _Fake().set_audio(decim, taps, fmt, scale)


def test_accepted_arguments():
    f = G.channelizer._audio_args
    assert f(None, None, "nonsense", 0.0)[0] == 0                       # off: the other arguments are ignored
    d, h, code, sc = f(64, np.arange(256.0), "S16", -3)
    assert (d, h.dtype, h.size, code, float(sc)) == (64, np.float32, 256, G.AUDIO_S16, -3.0)
    d, h, code, sc = f(np.int64(1), [0.5], "f32", np.nan)               # the scale is ignored for f32
    assert (d, h.tolist(), code, float(sc)) == (1, [0.5], G.AUDIO_F32, 1.0)


def test_outs_is_refused_while_the_audio_is_on():
    p = _Fake()
    p._audio = 4
    outs = [np.empty(3 * lo, np.float32) for lo in p.lout]
    x = np.zeros(3 * p.H, np.complex64)
    for call in (lambda: p.work(x, outs=outs), lambda: p.work_iq(np.zeros((3 * p.H, 2), np.int16), outs=outs)):
        with pytest.raises(ValueError) as e:
            call()
        assert "audio" in str(e.value)


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)
TAPS = G.lowpass_taps(4, 16)


@pytest.mark.parametrize("change, word", [
    (dict(demod=None), "audio_decim needs demod"),
    (dict(audio_taps=None), "audio_taps"),
    (dict(audio_decim=None), "audio_taps needs audio_decim"),
    (dict(audio_decim=0), "decimation"),
    (dict(audio_decim=65), "decimation"),
    (dict(audio_taps=np.ones(300)), "taps"),
    (dict(audio_taps=[np.nan]), "finite"),
    (dict(audio_format="s8"), "format"),
    (dict(audio_format="s16", audio_scale=0.0), "scale"),
    (dict(inpveclen=4096), "demod"),
    (dict(activity_detection_segments=[[0.1, 0.3]]), "demod"),
    (dict(waterfall=object()), "demod"),
    (dict(iq_output="sc16", iq_output_scale=32768.0), "demod"),
    (dict(devices=[0, 0]), "demod"),
], ids=["without demod", "without taps", "taps without decim", "decim 0", "decim 65", "300 taps", "NaN tap", "format", "scale 0", "inpveclen > 1",
        "detection segments", "waterfall", "iq_output", "two devices"])
def test_hier_block_refusals(change, word):
    kw = dict(KW, inptype=8, demod="fm", audio_decim=4, audio_taps=TAPS)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert word in str(e.value)


def test_the_keywords_are_keyword_only():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    for name, default in (("audio_decim", None), ("audio_taps", None), ("audio_format", "f32"), ("audio_scale", 1.0)):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default == default, name
    assert list(par).index("audio_decim") > list(par).index("demod_gain")


@pytest.mark.parametrize("change", [
    dict(inptype=8, demod="fm", audio_decim=4, audio_taps=TAPS),
    dict(inptype=8, demod="mag", audio_decim=1, audio_taps=[1.0], audio_format="s16", audio_scale=-100.0),
    dict(inptype=4, demod="fm", audio_decim=2, audio_taps=TAPS, fine_tuning=True, levels=True, gains=[2.0], lag1=True),
], ids=["fm, f32", "mag, s16", "Float input with the other settings"])
def test_hier_block_acceptances(change):
    """every check of the constructor is passed and it gets as far as creating the handle, which fails for want of a device where there is none"""
    kw = dict(KW)
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.pipeline.audio_setting()[0] == change["audio_decim"]
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)


def test_slicing_the_matrix_into_channels_is_the_models_stream():
    """a hand-made [nb, A] matrix, lout = [8, 24], D = 4: row m holds block m, channel c the lout_c / D columns from its own prefix sum on; built from
    the model's audio of two calls (3 + 2 blocks), cut back it is the model's audio of every call"""
    lout, D, taps = [8, 24], 4, np.array([0.5, -0.25, 0.125, 1.0, 2.0], np.float32)
    rng = np.random.default_rng(1)
    d = [rng.standard_normal(5 * lo).astype(np.float32) for lo in lout]
    calls = [(0, 3, [d[c][:3 * lo] for c, lo in enumerate(lout)]), (3, 2, [d[c][3 * lo:] for c, lo in enumerate(lout)])]
    for fmt, scale, dt in (("f32", 1.0, np.float32), ("s16", 1000.0, np.int16)):
        want = A.audio_stream(A.History(2, taps.size), calls, taps, D, fmt, scale)
        for (first, nb, _ds), w in zip(calls, want):
            mat = np.empty((nb, 8), dt)
            assert sum(lo // D for lo in lout) == 8
            mat[:, 0:2] = w[0].reshape(nb, 2)
            mat[:, 2:8] = w[1].reshape(nb, 6)
            got = G.audio_channels(mat, lout, D)
            assert [g.dtype for g in got] == [dt, dt] and [g.shape for g in got] == [(nb * 2,), (nb * 6,)]
            for c in range(2):
                assert got[c].tobytes() == w[c].tobytes(), (fmt, first, c)
        # and the two calls together are one call of five blocks, in bits (the history links them)
        one = A.audio_stream(A.History(2, taps.size), [(0, 5, d)], taps, D, fmt, scale)[0]
        for c in range(2):
            assert np.concatenate([w[c] for w in want]).tobytes() == one[c].tobytes()
    with pytest.raises(ValueError):
        G.audio_channels(np.zeros((2, 7), np.float32), lout, D)
    assert G.audio_channels(np.zeros((0, 0), np.float32), [], 3) == []
