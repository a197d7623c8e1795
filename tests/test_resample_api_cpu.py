"""CPU tests of the audio resampler's host side (no GPU): the ctypes prototypes of the five C-ABI entries against include/fdc_amd.h, null handles, the
Python checks made before any library call, audio_resample_ratio, resampler_taps, the hier block's keywords, and the slicing of a hand-made padded
matrix into the channels' valid samples.  (The model is held to its bound by tests/test_resample_cpu.py; the device pass to the model, in bits, by
tests/test_resample_gpu.py.)"""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd.channelizer import Pipeline, PipelineGroup
import audio_model as A
import resample_model as RS
from test_audio_api_cpu import KW, _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdc_pipeline_set_audio_resampler", "fdc_pipeline_audio_resampler_setting", "fdc_pipeline_audio_first_block", "fdc_audio_resampler_counts",
         "fdc_pipeline_audio_resampler_pass_device")


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    i32, pi32, pf = C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ctype = {"fdc_pipeline *p": C.c_void_p, "const fdc_pipeline *p": C.c_void_p, "int32_t up": i32, "int32_t down": i32, "const float *taps": pf,
             "int32_t ntaps": i32, "int32_t format": i32, "float scale": C.c_float, "int32_t *up": pi32, "int32_t *down": pi32, "int32_t *ntaps": pi32,
             "int32_t *format": pi32, "float *scale": pf, "float *taps": pf, "int32_t taps_capacity": i32, "int32_t lout": i32,
             "int64_t first_block": C.c_int64, "int32_t nblocks": i32, "int32_t *counts": pi32, "int nblocks": C.c_int, "const void *d_in": C.c_void_p,
             "void *d_out": C.c_void_p, "const void *d_hist_in": C.c_void_p, "void *d_hist_out": C.c_void_p, "const void *d_mask": C.c_void_p,
             "void *stream": C.c_void_p}
    rtype = {"int": C.c_int, "int64_t": C.c_int64}
    for name in NAMES:
        m = re.search(r"^(int|int64_t)\s%s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is rtype[m.group(1)], name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert (G.channelizer.RESAMPLER_MAX_UP, G.channelizer.RESAMPLER_MAX_DOWN, G.channelizer.RESAMPLER_MAX_PHASE_TAPS) == (64, 128, 256)


def test_every_symbol_is_exported_and_null_handles_are_argument_errors():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    taps = (C.c_float * 4)(1, 0, 0, 0)
    assert lib.fdc_pipeline_set_audio_resampler(None, 1, 2, taps, 4, 0, 1.0) == -1
    assert lib.fdc_pipeline_set_audio_resampler(None, 0, 0, None, 0, 0, 1.0) == -1
    assert lib.fdc_pipeline_audio_resampler_setting(None, None, None, None, None, None, None, 0) == -1
    assert lib.fdc_pipeline_audio_resampler_pass_device(None, None, None, None, None, 0, 1, None, None) == -1
    assert lib.fdc_pipeline_audio_first_block(None) == -1
    for m in ("set_audio_resampler", "audio_resampler_setting", "audio_resampler_pass_device", "audio_first_block"):
        assert callable(getattr(Pipeline, m)), m
    assert not hasattr(PipelineGroup, "set_audio_resampler")    # no group setter: the group entries do not serve the demodulation


GOOD = np.ones(8, np.float32)


@pytest.mark.parametrize("up, down, taps, fmt, scale", [
    (0, 1, GOOD, "f32", 1.0), (65, 1, GOOD, "f32", 1.0), (1.5, 1, GOOD, "f32", 1.0), (True, 3, GOOD, "f32", 1.0), (-1, 1, GOOD, "f32", 1.0),
    (1, 0, GOOD, "f32", 1.0), (1, 129, GOOD, "f32", 1.0), (1, None, GOOD, "f32", 1.0), (3, 2.0, GOOD, "f32", 1.0),
    (2, 4, GOOD, "f32", 1.0), (48, 24, GOOD, "f32", 1.0), (64, 128, GOOD, "f32", 1.0),
    (3, 2, np.zeros(0, np.float32), "f32", 1.0), (1, 2, np.ones(257, np.float32), "f32", 1.0), (3, 2, np.ones(3 * 256 + 1, np.float32), "f32", 1.0),
    (3, 2, None, "f32", 1.0), (3, 2, [1.0, np.nan], "f32", 1.0), (3, 2, [np.inf], "f32", 1.0), (3, 2, [1e39], "f32", 1.0),
    (3, 2, GOOD, "s8", 1.0), (3, 2, GOOD, 1, 1.0), (3, 2, GOOD, None, 1.0),
    (3, 2, GOOD, "s16", 0.0), (3, 2, GOOD, "s16", np.nan), (3, 2, GOOD, "s16", np.inf), (3, 2, GOOD, "s16", 1e39)],
    ids=["up 0", "up 65", "up 1.5", "up True", "up -1", "down 0", "down 129", "down None", "down 2.0", "2/4", "48/24", "64/128", "no taps",
         "257 taps at up 1", "769 taps at up 3", "taps None", "NaN tap", "Inf tap", "a tap beyond float32", "format s8", "format 1", "format None",
         "scale 0", "scale NaN", "scale Inf", "scale beyond float32"])
def test_argument_checks_before_the_library(up, down, taps, fmt, scale):
    with pytest.raises(ValueError):
        _Fake().set_audio_resampler(up, down, taps, fmt, scale)


def test_a_ratio_that_is_not_reduced_names_the_reduced_one():
    with pytest.raises(ValueError) as e:
        _Fake().set_audio_resampler(48, 50, GOOD)
    assert "24 / 25" in str(e.value)


def test_accepted_arguments():
    f = G.channelizer._resampler_args
    assert f(None, None, None, "nonsense", 0.0)[:2] == (0, 0)               # off: the other arguments are ignored
    u, d, h, code, sc = f(64, 127, np.arange(64 * 256.0), "S16", -3)
    assert (u, d, h.dtype, h.size, code, float(sc)) == (64, 127, np.float32, 16384, G.AUDIO_S16, -3.0)
    u, d, h, code, sc = f(np.int64(1), np.int32(1), [0.5], "f32", np.nan)   # the scale is ignored for f32
    assert (u, d, h.tolist(), code, float(sc)) == (1, 1, [0.5], G.AUDIO_F32, 1.0)
    assert f(3, 2, np.ones(3 * 256), "f32", 1.0)[2].size == 768


def test_outs_is_refused_while_the_resampler_is_on():
    p = _Fake()
    p._audio = 8
    outs = [np.empty(3 * lo, np.float32) for lo in p.lout]
    with pytest.raises(ValueError) as e:
        p.work(np.zeros(3 * p.H, np.complex64), outs=outs)
    assert "audio" in str(e.value)


def test_audio_resample_ratio():
    assert G.audio_resample_ratio(25000, 8000) == (8, 25) and G.audio_resample_ratio(25000, 16000) == (16, 25)
    assert G.audio_resample_ratio(25000, 48000) == (48, 25) and G.audio_resample_ratio(25e3, 48e3) == (48, 25)
    assert G.audio_resample_ratio(6.4e6 * 256 / 65536, 8000) == (8, 25)                     # the headline geometry's channel rate
    assert G.audio_resample_ratio(Fraction(75000, 3), 8000) == (8, 25)
    assert G.audio_resample_ratio(48000, 48000) == (1, 1) and G.audio_resample_ratio(128, 64) == (1, 2) and G.audio_resample_ratio(1, 64) == (64, 1)
    for rin, rout in ((25000, 44100), (1, 65), (129, 1), (25000, 0), (0, 8000), (-1, 8000), (float("nan"), 8000), (float("inf"), 8000), ("x", 8000)):
        with pytest.raises(ValueError):
            G.audio_resample_ratio(rin, rout)
    u, d = G.audio_resample_ratio(25000, 8000)
    assert isinstance(u, int) and isinstance(d, int)


def test_resampler_taps():
    for up, down in ((8, 25), (48, 25), (1, 8), (64, 1), (1, 1)):
        h = G.resampler_taps(up, down)
        assert h.dtype == np.float32 and h.size == 16 * up
        assert abs(float(h.astype(np.float64).sum()) - up) < 1e-5 * up
        assert np.array_equal(h, h[::-1])                                   # linear phase
        # every phase has about unit DC gain: the interpolation does not ripple at DC by more than the window's stopband lets through
        kp, hp = RS.phase_taps(h, up)
        assert kp == 16 and np.abs(hp.astype(np.float64).sum(axis=1) - 1.0).max() < 0.02
        # the cutoff: -6 dB at 0.5 / max(up, down) cycles per upsampled sample, where the window's main lobe (4 / ntaps wide) is narrower than that
        fc = 0.5 / max(up, down)
        gain = abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * fc * np.arange(h.size)))) / up
        assert 0.45 < gain < 0.55 or 4.0 / h.size > fc or fc == 0.5, (up, down, gain)         # (at 1 / 1 the cutoff is the Nyquist frequency itself)
    assert 4.0 / (16 * 48) < 0.5 / 48 and 4.0 / (16 * 64) < 0.5 / 64                 # (two of the ratios above are held to it)
    assert G.resampler_taps(8, 25, 4).size == 32 and G.resampler_taps(8, 25, cutoff=0.01).size == 128
    for args in ((8, 24), (0, 1), (8, 25, 0), (8, 25, 257), (8, 25, 16, 0.0), (8, 25, 16, 0.6), (8, 25, 2.5)):
        with pytest.raises(ValueError):
            G.resampler_taps(*args)
    # the setter takes what the designer gives, at the largest ratio too
    G.channelizer._resampler_args(64, 127, G.resampler_taps(64, 127, 256), "f32", 1.0)


TAPS = G.resampler_taps(8, 25, 4)


@pytest.mark.parametrize("change, word", [
    (dict(demod=None), "need demod"),
    (dict(audio_decim=4), "two forms"),
    (dict(audio_down=None), "go together"),
    (dict(audio_up=None), "go together"),
    (dict(audio_up=None, audio_down=None), "audio_taps needs"),
    (dict(audio_up=16, audio_down=50), "8 / 25"),
    (dict(audio_up=65), "interpolation"),
    (dict(audio_down=129), "decimation"),
    (dict(audio_taps=np.ones(8 * 256 + 1)), "taps per phase"),
    (dict(audio_taps=[np.nan]), "finite"),
    (dict(audio_format="s8"), "format"),
    (dict(audio_format="s16", audio_scale=0.0), "scale"),
    (dict(audio_packed=True, levels=True, squelch_db=-20.0), "audio_packed needs audio_decim"),
    (dict(devices=[0, 0]), "demod"),
], ids=["without demod", "with audio_decim", "up alone", "down alone", "taps alone", "not reduced", "up 65", "down 129", "too many taps", "NaN tap",
        "format", "scale 0", "packed", "two devices"])
def test_hier_block_refusals(change, word):
    kw = dict(KW, inptype=8, demod="fm", audio_up=8, audio_down=25, audio_taps=TAPS)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert word in str(e.value), str(e.value)


def test_the_keywords_are_keyword_only():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    for name in ("audio_up", "audio_down"):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default is None, name
    assert list(par).index("audio_up") > list(par).index("audio_decim")


@pytest.mark.parametrize("change", [
    dict(inptype=8, demod="fm", audio_up=8, audio_down=25, audio_taps=TAPS),
    dict(inptype=8, demod="mag", audio_up=48, audio_down=25, audio_format="s16", audio_scale=-100.0),
], ids=["fm, f32", "mag, s16, the default taps"])
def test_hier_block_acceptances(change):
    """every check of the constructor is passed and it gets as far as creating the handle, which fails for want of a device where there is none"""
    kw = dict(KW)
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.pipeline.audio_resampler_setting()[:2] == (change["audio_up"], change["audio_down"]) and fdc.pipeline.audio_setting() is None
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)


def test_slicing_a_padded_matrix_gives_the_valid_samples():
    """a hand-made matrix at (3, 4), lout = [6, 2], first_block 5: W = [5, 2], the counts alternate; cut back it is the model's outputs, and the two
    calls together are the one call's"""
    louts, up, down, first = [6, 2], 3, 4, 5
    taps = np.array([0.5, -0.25, 0.125, 1.0, 2.0, -1.0, 0.75], np.float32)
    kp = RS.ceil_div(taps.size, up)
    rng = np.random.default_rng(1)
    d = [rng.standard_normal(5 * lo).astype(np.float32) for lo in louts]
    calls = [(first, 3, [d[c][:3 * lo] for c, lo in enumerate(louts)]), (first + 3, 2, [d[c][3 * lo:] for c, lo in enumerate(louts)])]
    assert G.audio_block_counts(6, up, down, first, 5).tolist() == [4, 5, 4, 5, 4] and G.audio_block_counts(2, up, down, first, 5).tolist() == [1, 2, 1, 2, 1]
    for fmt, scale, dt in (("f32", 1.0, np.float32), ("s16", 1000.0, np.int16)):
        hist = A.History(2, kp)
        hist.next = first
        mats = RS.stream(hist, calls, taps, up, down, louts, fmt, scale)
        got = []
        for (f0, nb, ds), mat in zip(calls, mats):
            assert mat.shape == (nb, 7) and mat.dtype == dt
            # the pads are zero bits, behind the cell's outputs
            c0 = G.audio_block_counts(6, up, down, f0, nb)
            assert all(mat[m, c0[m]:5].tobytes() == bytes(mat.itemsize * (5 - c0[m])) for m in range(nb))
            got.append(G.audio_resampled_channels(mat, louts, up, down, f0))
            for c, lo in enumerate(louts):
                assert got[-1][c].dtype == dt
        for c, lo in enumerate(louts):
            one = RS.audio32(d[c], taps, up, down, lo, first, fmt, scale)
            assert np.concatenate([g[c] for g in got]).tobytes() == one.tobytes(), (fmt, c)
    with pytest.raises(ValueError):
        G.audio_resampled_channels(np.zeros((2, 6), np.float32), louts, up, down, 0)
    with pytest.raises(ValueError):
        G.audio_resampled_channels(np.zeros((2, 7), np.float32), louts, 6, 8, 0)
    assert G.audio_resampled_channels(np.zeros((0, 0), np.float32), [], 3, 2, 0) == []
    for args in ((0, 3, 2, 0, 1), (8, 3, 2, -1, 1), (8, 3, 2, 0, -1), (8, 4, 2, 0, 1), (8.0, 3, 2, 0, 1)):
        with pytest.raises(ValueError):
            G.audio_block_counts(*args)
