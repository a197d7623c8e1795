"""CPU tests of the packed audio's host side (no GPU): the ctypes prototypes of the four C-ABI entries against include/fdc_amd.h, null handles, the
Python checks made before any library call, and the hier block's keyword, refusals and acceptances.  (The definition: tests/test_audio_pack_cpu.py;
the device against it, in bytes: tests/test_audio_pack_gpu.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup
from test_squelch_api_cpu import KW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdc_pipeline_set_audio_packing", "fdc_pipeline_audio_packing", "fdc_pipeline_audio_packed", "fdc_pipeline_audio_pack_offsets_device")


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    ctype = {"fdc_pipeline *p": C.c_void_p, "const fdc_pipeline *p": C.c_void_p, "int on": C.c_int, "void *dst": C.c_void_p,
             "size_t capacity_bytes": C.c_size_t, "int nblocks": C.c_int, "int64_t *count": C.POINTER(C.c_int64), "const void *d_mask": C.c_void_p,
             "const void *d_base_in": C.c_void_p, "void *d_off": C.c_void_p, "void *d_total_out": C.c_void_p, "void *stream": C.c_void_p}
    for name in NAMES:
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int, name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert "PACKED AUDIO" in hdr


def test_every_symbol_is_exported_and_null_handles_write_nothing():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.fdc_pipeline_set_audio_packing(None, 1) == -1 and lib.fdc_pipeline_set_audio_packing(None, 0) == -1
    assert lib.fdc_pipeline_audio_packing(None) == -1
    buf = np.full(16, 7, np.uint8)
    count = C.c_int64(-12345)
    assert lib.fdc_pipeline_audio_packed(None, buf.ctypes.data, buf.nbytes, 1, C.byref(count)) == -1 and (buf == 7).all() and count.value == -12345
    assert lib.fdc_pipeline_audio_packed(None, None, 0, 1, None) == -1
    assert lib.fdc_pipeline_audio_pack_offsets_device(None, None, None, None, None, 1, None) == -1
    for m in ("set_audio_packing", "audio_packing", "audio_packed", "audio_pack_offsets_device"):
        assert callable(getattr(Pipeline, m)), m
    assert not hasattr(PipelineGroup, "set_audio_packing")             # no group setter
    assert callable(G.audio_pack_offsets) and callable(G.unpack_audio)


class _Fake(Pipeline):
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self, packing):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]
        self._packing = packing
        self._last_nb = 3

    def audio_setting(self):
        raise AssertionError("the library was asked")

    def __del__(self):
        pass


def test_python_checks_before_the_library():
    with pytest.raises(ValueError) as e:
        _Fake(True).audio()                                           # the matrix getter while the packing is on
    assert "packing" in str(e.value)
    with pytest.raises(ValueError) as e:
        _Fake(True).audio(2)
    assert "packing" in str(e.value)
    with pytest.raises(ValueError) as e:
        _Fake(False).audio_packed()                                   # the packed getter while it is off
    assert "packing is off" in str(e.value)
    with pytest.raises(ValueError):
        _Fake(True).audio_packed(-1)
    f = _Fake(True)
    f._last_nb = None
    with pytest.raises(ValueError):
        f.audio_packed()
    for bad in (None, "yes", 1.0, [1]):
        with pytest.raises(ValueError):
            _Fake(False).set_audio_packing(bad)


@pytest.mark.parametrize("change, word", [
    (dict(audio_decim=None, audio_taps=None), "audio_packed needs audio_decim and squelch_db"),
    (dict(squelch_db=None), "audio_packed needs audio_decim and squelch_db"),
    (dict(audio_packed=1), "audio_packed is a bool"),
    (dict(audio_packed="on"), "audio_packed is a bool"),
    (dict(levels=False), "squelch_db needs levels"),
    (dict(demod=None), "audio_decim needs demod"),
], ids=["without the audio", "without the squelch", "an int", "a string", "without levels", "without demod"])
def test_hier_block_refusals(change, word):
    kw = dict(KW, inptype=8, levels=True, squelch_db=-20.0, demod="fm", audio_decim=4, audio_taps=G.lowpass_taps(4, 16), audio_packed=True)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert word in str(e.value)


def test_the_keyword_is_keyword_only_and_off_by_default():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    assert par["audio_packed"].kind is inspect.Parameter.KEYWORD_ONLY and par["audio_packed"].default is False
    assert list(par).index("audio_packed") > list(par).index("squelch_hang")


@pytest.mark.parametrize("change", [
    dict(audio_packed=True),
    dict(audio_packed=False),
    dict(audio_packed=True, audio_format="s16", audio_scale=9000.0, squelch_close_db=-26.0, squelch_hang=3, fine_tuning=True, gains=[2.0]),
], ids=["on", "off", "with the other settings"])
def test_hier_block_acceptances(change):
    """every check of the constructor is passed and it gets as far as creating the handle, which fails for want of a device where there is none"""
    kw = dict(KW, inptype=8, levels=True, squelch_db=-20.0, demod="fm", audio_decim=4, audio_taps=G.lowpass_taps(4, 16))
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.pipeline.audio_packing() == change["audio_packed"]
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)
