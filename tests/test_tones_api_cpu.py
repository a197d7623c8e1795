"""CPU tests of the channel tones' host side (no GPU): the ctypes prototypes of the six C-ABI entries against include/fdc_amd.h, null handles, the
Python checks made before any library call, the helpers (ctcss_tones, tone_increments, tone_amplitude, tone_table), and the hier block's keywords,
refusals and acceptances.  (The definition: tests/test_tones_cpu.py; the device against it, in bytes: tests/test_tones_gpu.py.)"""
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
NAMES = ("fdc_pipeline_set_tones", "fdc_pipeline_tones_setting", "fdc_pipeline_tones", "fdc_pipeline_tones_device", "fdc_pipeline_tones_pass_device",
         "fdc_tone_table")


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    i32, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    ctype = {"fdc_pipeline *p": C.c_void_p, "const fdc_pipeline *p": C.c_void_p, "const uint32_t *inc": u32, "uint32_t *inc": u32, "int nchan": C.c_int,
             "int ntones": C.c_int, "int32_t group": C.c_int32, "int32_t frame_blocks": C.c_int32, "int32_t *ntones": i32, "int32_t *group": i32,
             "int32_t *frame_blocks": i32, "void *dst": C.c_void_p, "size_t capacity_bytes": C.c_size_t, "int nblocks": C.c_int, "int32_t *nframes": i32,
             "const void *d_in": C.c_void_p, "void *d_frames": C.c_void_p, "const void *d_carry_in": C.c_void_p, "void *d_carry_out": C.c_void_p,
             "int64_t first_block": C.c_int64, "int32_t fill": C.c_int32, "void *stream": C.c_void_p, "float *dst": C.POINTER(C.c_float)}
    rtype = {"int": C.c_int, "void *": C.c_void_p}
    for name in NAMES:
        m = re.search(r"^(int|void \*)\s?%s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is rtype[m.group(1)], name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert "CHANNEL TONES" in hdr


def test_every_symbol_is_exported_and_null_handles_are_argument_errors():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    inc = (C.c_uint32 * 2)(1, 1)
    assert lib.fdc_pipeline_set_tones(None, inc, 2, 1, 16, 32) == -1
    assert lib.fdc_pipeline_set_tones(None, None, 0, 0, 0, 0) == -1
    assert lib.fdc_pipeline_tones_setting(None, None, None, None, None) == -1
    buf = np.full(16, 7, np.uint8)
    nf = C.c_int32(-3)
    assert lib.fdc_pipeline_tones(None, buf.ctypes.data, buf.nbytes, 1, C.byref(nf)) == -1 and (buf == 7).all() and nf.value == -3
    assert lib.fdc_pipeline_tones_pass_device(None, None, None, None, None, 0, 0, 1, None) == -1
    assert lib.fdc_pipeline_tones_device(None) is None
    assert lib.fdc_tone_table(None) == -1
    for m in ("set_tones", "tones_setting", "tones", "tones_device", "tones_pass_device"):
        assert callable(getattr(Pipeline, m)), m
    assert not hasattr(PipelineGroup, "set_tones")              # no group setter
    for name in ("tone_table", "ctcss_tones", "tone_increments", "tone_amplitude"):
        assert callable(getattr(G, name)), name


class _Fake(Pipeline):
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]

    def __del__(self):
        pass


ONE = np.ones((2, 3), np.uint32)


@pytest.mark.parametrize("inc, group, frame", [
    (np.ones((3, 3), np.uint32), 16, 32), (np.ones((2, 0), np.uint32), 16, 32), (np.ones((2, 65), np.uint32), 16, 32), (np.ones((1, 2, 3), np.uint32), 16, 32),
    (np.ones((2, 3), np.float32), 16, 32), (np.array([[-1, 1, 1], [1, 1, 1]]), 16, 32), (np.array([[1 << 32, 1, 1], [1, 1, 1]], np.int64), 16, 32),
    (ONE, 0, 32), (ONE, -4, 32), (ONE, 1.5, 32), (ONE, True, 32), (ONE, None, 32),
    (ONE, 16, 0), (ONE, 16, 4097), (ONE, 16, 2.0), (ONE, 16, None)],
    ids=["three rows for two channels", "no tone", "65 tones", "three dimensions", "floats", "negative", "beyond 32 bits", "group 0", "group -4",
         "group 1.5", "group True", "group None", "frame 0", "frame 4097", "frame 2.0", "frame None"])
def test_argument_checks_before_the_library(inc, group, frame):
    with pytest.raises(ValueError):
        _Fake().set_tones(inc, group, frame)


def test_accepted_arguments():
    f = G.channelizer._tones_args
    assert f(2, None, "nonsense", -5) == (None, 0, 0)                   # off: the other arguments are ignored
    a, s, w = f(3, [5, 6], np.int64(1), 4096)                           # one row for all channels
    assert a.dtype == np.uint32 and a.shape == (3, 2) and a.tolist() == [[5, 6]] * 3 and (s, w) == (1, 4096) and a.flags.c_contiguous
    a, s, w = f(2, np.array([[0, 0xFFFFFFFF], [7, 8]], np.uint64), 24576, 1)
    assert a.tolist() == [[0, 0xFFFFFFFF], [7, 8]] and (s, w) == (24576, 1)
    a, s, w = f(0, np.zeros((0, 4), np.uint32), 16, 32)                 # a plan without channels
    assert a.shape == (0, 4)
    a, s, w = f(2, np.ones(64, np.int64), 16, 32)
    assert a.shape == (2, 64)


def test_the_helpers():
    f = G.ctcss_tones()
    assert f.shape == (50,) and f.dtype == np.float64 and f[0] == 67.0 and f[-1] == 254.1 and (np.diff(f) > 0).all()
    assert {100.0, 123.0, 151.4, 206.5, 229.1}.issubset(set(f.tolist())) and len(set(f.tolist())) == 50
    inc = G.tone_increments(f, 25000.0, 16)
    assert inc.dtype == np.uint32 and inc.shape == (50,)
    assert inc[0] == int(np.rint(67.0 * 16 / 25000.0 * 2.0 ** 32)) and (np.diff(inc.astype(np.int64)) > 0).all()
    assert G.tone_increments(0.0, 8000.0, 1) == 0 and G.tone_increments(2000.0, 8000.0, 1) == 1 << 30
    assert G.tone_increments(-2000.0, 8000.0, 1) == 3 << 30 and G.tone_increments(4000.0, 8000.0, 1) == 1 << 31            # negative: wraps; Nyquist
    two = G.tone_increments([[100.0, 200.0], [100.0, 200.0]], [25000.0, 12500.0], 4)                                       # one rate per row
    assert two.shape == (2, 2) and (np.abs(two[1].astype(np.int64) - 2 * two[0].astype(np.int64)) <= 1).all()
    for bad in (lambda: G.tone_increments(5000.0, 8000.0, 1), lambda: G.tone_increments(100.0, 8000.0, 0), lambda: G.tone_increments(np.nan, 8000.0, 1),
                lambda: G.tone_increments(100.0, 0.0, 1), lambda: G.tone_increments(300.0, 8000.0, 16)):
        with pytest.raises(ValueError):
            bad()
    # tone_amplitude undoes n / 2 and the droop: exact on the analytic |Z| of a tone
    r, S, n = 25000.0, 16, 32 * 128
    x = np.pi * f / r
    droop = np.sin(x * S) / (S * np.sin(x))
    Z = 0.25 * (n / 2) * droop * np.exp(1j * 0.3)
    assert np.allclose(G.tone_amplitude(Z, n, f, r, S), 0.25, rtol=1e-12)
    assert np.allclose(G.tone_amplitude(np.array([3.0 + 4.0j]), 10, 0.0, r, S), 1.0)          # f = 0: no droop
    tab = G.tone_table()
    assert tab.shape == (1024, 2) and tab.dtype == np.float32 and tab[256].tolist() == [0.0, 1.0]


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)
INC = np.arange(1, 6, dtype=np.uint32)


@pytest.mark.parametrize("change, word", [
    (dict(demod=None), "tones needs demod"),
    (dict(tones=np.ones(65, np.uint32)), "1 .. 64"),
    (dict(tones=np.ones((2, 3), np.uint32)), "rows"),
    (dict(tones=[0.5, 1.5]), "integers"),
    (dict(tone_group=0), "group"),
    (dict(tone_frame=5000), "frame"),
    (dict(devices=[0, 0]), "one device"),
    (dict(inpveclen=4096), "demod"),
], ids=["without demod", "65 tones", "two rows for one channel", "floats", "group 0", "frame 5000", "two devices", "inpveclen > 1"])
def test_hier_block_refusals(change, word):
    kw = dict(KW, inptype=8, demod="fm", tones=INC)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert word in str(e.value)


def test_the_keywords_are_keyword_only():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    for name, default in (("tones", None), ("tone_group", 16), ("tone_frame", 32)):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default == default, name
    assert list(par).index("tones") > list(par).index("squelch_hang")
    assert callable(G.FrequencyDomainChannelizer.set_tones)


@pytest.mark.parametrize("change", [
    dict(inptype=8, demod="fm", tones=INC),
    dict(inptype=8, demod="mag", tones=INC[None, :], tone_group=8, tone_frame=4096, audio_decim=4, audio_taps=G.lowpass_taps(4, 16)),
    dict(inptype=4, demod="fm", tones=G.tone_increments(G.ctcss_tones(), 25000.0, 16), levels=True, squelch_db=-3.0, fine_tuning=True, gains=[2.0], lag1=True),
], ids=["demod alone", "with the audio", "Float input with the other settings"])
def test_hier_block_acceptances(change):
    """every check of the constructor is passed and it gets as far as creating the handle, which fails for want of a device where there is none"""
    kw = dict(KW)
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.pipeline.tones_setting()[1:] == (change.get("tone_group", 16), change.get("tone_frame", 32))
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)
