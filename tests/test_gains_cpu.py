"""CPU tests of the channel gains (no GPU): numpy's statement of the definition (what the GPU tests compare the device with) on hand-made rows, the
seeded draw of gains the GPU tests use, the Python checks made before any library call, the hier block's refusals and acceptances, and the ctypes
prototypes of the three C-ABI entries against include/fdc_amd.h."""
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
NAMES = ("fdc_pipeline_set_gains", "fdc_pipeline_gains", "fdc_pipeline_group_set_gains")


def gained(y, g):
    """The definition on one channel's samples: every float32 component times the float32 gain, rounded once (include/fdc_amd.h, CHANNEL GAINS)"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (np.ascontiguousarray(y, np.complex64).view(np.float32) * np.float32(g)).view(np.complex64)


def draw_gains(nchan, seed):
    """one gain per channel: magnitudes 2^u, u uniform in [-8, 8], random signs; where the plan has room, one exact 1.0, one 0.0 and one power of two"""
    rng = np.random.default_rng(7000 + seed)
    g = (np.exp2(rng.uniform(-8.0, 8.0, nchan)) * rng.choice([-1.0, 1.0], nchan)).astype(np.float32)
    special = [np.float32(1.0), np.float32(0.0), np.float32(2.0 ** int(rng.integers(-8, 9)))]
    if nchan == 1:
        g[0] = np.float32(-0.37)
    else:
        # one channel keeps a drawn gain (a plan of two or three takes as many of the special values as leave it one)
        for c, v in zip(rng.permutation(nchan)[:min(len(special), nchan - 1)], special):
            g[c] = v
    return g


def test_gained_on_hand_made_rows():
    f = lambda v: np.array(v, np.complex64)
    # -0.0 keeps its sign under a positive gain and loses it under a negative one; g = 0 gives signed zeros
    y = f([complex(-0.0, 0.0), complex(1.5, -2.0)])
    assert gained(y, 2.0).view(np.uint32).tolist() == [0x80000000, 0, 0x40400000, 0xC0800000]
    assert gained(y, -2.0).view(np.uint32).tolist() == [0, 0x80000000, 0xC0400000, 0x40800000]
    assert gained(y, 0.0).view(np.uint32).tolist() == [0x80000000, 0, 0, 0x80000000]
    # NaN stays NaN, infinity keeps its sign, 0 * inf is NaN
    r = gained(f([complex(np.nan, 1.0), complex(np.inf, -np.inf)]), -3.0).view(np.float32)
    assert np.isnan(r[0]) and r[1] == -3.0 and r[2] == -np.inf and r[3] == np.inf
    assert np.isnan(gained(f([complex(np.inf, 0.0)]), 0.0).view(np.float32)[0])
    # one rounding in float32: 1/3 * 3 is 1 exactly in float32 (not in the reals), and the gain is taken as float32
    third = np.float32(1.0) / np.float32(3.0)
    assert gained(f([complex(third, 0)]), 3.0).real[0] == np.float32(1.0)
    assert gained(f([1.0]), 0.1).real[0] == np.float32(0.1)
    # a product that is subnormal is kept (no flush to zero): 2^-120 * 2^-20 = 2^-140; below the smallest subnormal it rounds to zero
    s = gained(f([complex(2.0 ** -120, -(2.0 ** -120))]), 2.0 ** -20).view(np.float32)
    assert s[0] == np.float32(2.0 ** -140) and s[1] == -np.float32(2.0 ** -140) and s[0] != 0
    assert gained(f([complex(2.0 ** -120, 0)]), 2.0 ** -40).real[0] == 0.0
    # a product above the largest float32 is infinite
    assert gained(f([complex(3e38, 0)]), 2.0).real[0] == np.inf
    assert gained(y, 1.0).tobytes() == y.tobytes() and gained(y, 2.0).dtype == np.complex64


def test_the_draw_of_gains():
    for n in (1, 2, 3, 4, 64, 255):
        g = draw_gains(n, n)
        assert g.dtype == np.float32 and g.shape == (n,) and np.isfinite(g).all()
        mag = np.abs(g[g != 0])
        assert (mag >= 2.0 ** -8).all() and (mag <= 2.0 ** 8).all()
        assert (g != 1.0).any()
        if n >= 4:
            assert (g == 1.0).any() and (g == 0.0).any() and (g < 0).any()
            assert any(v != 0 and v != 1 and np.frexp(v)[0] == 0.5 for v in np.abs(g)) or (g == 1.0).sum() >= 2
    assert draw_gains(64, 1).tobytes() == draw_gains(64, 1).tobytes() and draw_gains(64, 1).tobytes() != draw_gains(64, 2).tobytes()


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    ctype = {"fdc_pipeline *p": C.c_void_p, "const fdc_pipeline *p": C.c_void_p, "fdc_pipeline_group *g": C.c_void_p,
             "const float *gain": C.POINTER(C.c_float), "float *dst": C.POINTER(C.c_float), "int n": C.c_int}
    for name in NAMES:
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int, name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
    assert "CHANNEL GAINS" in hdr and "cut -> fine tuning -> GAIN -> levels -> sc16 / sc8 narrowing" in hdr
    assert "an AGC that sets the next call's output" not in hdr


def test_every_symbol_is_exported():
    lib = G.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    # null handles are argument errors, not crashes
    one = (C.c_float * 1)(2.0)
    assert lib.fdc_pipeline_set_gains(None, one, 1) == -1 and lib.fdc_pipeline_set_gains(None, None, 0) == -1
    assert lib.fdc_pipeline_gains(None, one, 1) == -1
    assert lib.fdc_pipeline_group_set_gains(None, one, 1) == -1
    assert one[0] == 2.0
    for cls in (Pipeline, PipelineGroup):
        assert callable(cls.set_gains)
    assert callable(Pipeline.gains) and callable(G.FrequencyDomainChannelizer.set_gains)


class _Fake:
    """a handle-less stand-in: the checks below must raise before anything touches the library or the handle"""
    def __init__(self):
        self.H, self.N, self.ovl, self.lout, self._h = 2048, 4096, 2048, [128, 64], None
        self.channels = [(0, 256, .8, 1.), (512, 128, .8, 1.)]


@pytest.mark.parametrize("method", [Pipeline.set_gains, PipelineGroup.set_gains])
@pytest.mark.parametrize("bad", [[1.0], [1.0, 2.0, 3.0], [[1.0, 2.0]], [np.nan, 1.0], [1.0, np.inf], [-np.inf, 1.0], [1e39, 1.0]],
                         ids=["too few", "too many", "two dimensions", "NaN", "Inf", "-Inf", "infinite as float32"])
def test_argument_checks_before_the_library(method, bad):
    with pytest.raises(ValueError):
        method(_Fake(), bad)


KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05], [-0.2, 0.1]], activity_controlled_channels=[],
          act_contr_threshold=0.0, fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False,
          outputpath="", threaded=False, activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0,
          minchanflankpuffer=0.2, verbose=0, pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False)


@pytest.mark.parametrize("change", [
    dict(inpveclen=4096),
    dict(activity_controlled_channels=[[0.2, 0.01]]),
    dict(activity_detection_segments=[[0.1, 0.3]]),
    dict(waterfall=object()),
    dict(gains=[1.0]),
    dict(gains=[1.0, np.nan]),
    dict(gains=[np.inf, 2.0]),
], ids=["inpveclen > 1", "power-activation sinks", "detection segments", "waterfall", "wrong count", "NaN", "Inf"])
def test_hier_block_refusals(change):
    kw = dict(KW, inptype=8, gains=[2.0, 0.5])
    kw.update(change)
    with pytest.raises(ValueError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "gains" in str(e.value)


def test_hier_block_set_gains_keeps_the_constructor_refusals():
    """set_gains() of a block that was built with sink blocks (or items, or a waterfall) raises before it touches the handle; None is always accepted"""
    class _NoHandle:
        def set_gains(self, g):
            assert g is None
    fdc = object.__new__(G.FrequencyDomainChannelizer)
    fdc.throughput_channels, fdc.pipeline, fdc.gains = [[0.1, 0.05], [-0.2, 0.1]], _NoHandle(), None
    fdc._gains_refusal = "gains cannot go with activity-controlled channels or detection segments"
    with pytest.raises(ValueError) as e:
        fdc.set_gains([2.0, 0.5])
    assert "gains" in str(e.value)
    with pytest.raises(ValueError):
        fdc.set_gains([2.0])
    fdc.set_gains(None)
    assert fdc.gains is None


def test_gains_is_keyword_only():
    par = inspect.signature(G.FrequencyDomainChannelizer.__init__).parameters
    assert par["gains"].kind is inspect.Parameter.KEYWORD_ONLY and par["gains"].default is None
    assert list(par).index("gains") == list(par).index("levels") + 1


@pytest.mark.parametrize("change", [
    dict(inptype=8),
    dict(inptype=8, iq_output="sc16", iq_output_scale=32768.0),
    dict(inptype=8, iq_input="sc16", iq_scale=2.0 ** -15, iq_output="sc8", iq_output_scale=100.0),
    dict(inptype=8, fine_tuning=True),
    dict(inptype=8, levels=True),
    dict(inptype=8, levels=True, fine_tuning=True, iq_output="sc8", iq_output_scale=100.0),
    dict(inptype=4),
], ids=["alone", "sc16 output", "integer in and out", "fine tuning", "levels", "everything", "Float input"])
def test_hier_block_acceptances(change):
    """gains= combines with the other settings: every check of the constructor is passed and it gets as far as creating the handle, which fails for
    want of a device where there is none"""
    kw = dict(KW, gains=[2.0, -0.5])
    kw.update(change)
    if G.lib().fdc_device_count() > 0:
        fdc = G.FrequencyDomainChannelizer(**kw)
        assert fdc.gains.tolist() == [2.0, -0.5] and fdc.pipeline.gains().tolist() == [2.0, -0.5]
        return
    with pytest.raises(G.FdcError) as e:
        G.FrequencyDomainChannelizer(**kw)
    assert "FDC_ERR_NO_DEVICE" in str(e.value)
