"""CPU tests of fine tuning (no GPU): the 64-bit phase increment against exact rational arithmetic, the hier block's fine_nu against the formula
written out here, its refusals, and the ctypes prototypes against include/fdc_amd.h."""
import ctypes as C
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(inpveclen=1, blocksize=4096, relinvovl=2, throughput_channels=[[0.1, 0.05]], activity_controlled_channels=[], act_contr_threshold=0.0,
          fs=1.0, centerfrequency=0.0, freqmode=G.FREQMODE.normalized, windowtype=1, msgoutput=False, fileoutput=False, outputpath="", threaded=False,
          activity_detection_segments=[], act_det_threshold=0.0, minchandist=0.0, act_det_deactivation_delay=0, minchanflankpuffer=0.2, verbose=0,
          pow_act_deactivation_delay=0, pow_act_maxblocks=0, act_det_maxblocks=0, debug=False, max_blocks=4)


def exact_increment(nu):
    return int(round(Fraction(nu) * 2 ** 64)) % 2 ** 64          # round(Fraction) goes half to even


def test_increment_is_the_exactly_rounded_product():
    rng = np.random.default_rng(2024)
    nus = [float(v) for v in rng.uniform(-0.5, 0.5, 150)] + [float(v) for v in rng.uniform(-1, 1, 50) * 2.0 ** rng.integers(-60, -2, 50)]
    nus += [2.0 ** -40, -2.0 ** -40, 0.5 - 2.0 ** -53, -(0.5 - 2.0 ** -53), 0.0, 2.0 ** -65, 3 * 2.0 ** -65, -2.0 ** -65]      # (the last three: ties)
    assert len(nus) >= 200
    for nu in nus:
        assert abs(nu) < 0.5
        assert G.fine_tuning_increment(nu) == exact_increment(nu), nu


@pytest.mark.parametrize("nu", [float("nan"), 0.5, -0.5, 0.75, float("inf"), -float("inf")])
def test_increment_refuses_what_is_not_inside_half_a_cycle(nu):
    with pytest.raises(ValueError):
        G.fine_tuning_increment(nu)
    inc = C.c_uint64(12345)
    assert _lib.lib().fdc_fine_tuning_increment(nu, C.byref(inc)) == -1 and inc.value == 12345
    assert _lib.lib().fdc_fine_tuning_increment(0.25, None) == -1


def _mirror(monkeypatch, **change):
    """G.FrequencyDomainChannelizer with Pipeline replaced by a recorder: no device"""
    chan = sys.modules[G.FrequencyDomainChannelizer.__module__]
    seen = {}

    class FakePipeline:
        def __init__(self, *a, **kw):
            seen["channels"] = a[2]

        def set_fine_tuning(self, nu):
            seen["nu"] = np.array(nu, dtype=np.float64)

    monkeypatch.setattr(chan, "Pipeline", FakePipeline)
    kw = dict(KW, inptype=8)
    kw.update(change)
    return G.FrequencyDomainChannelizer(**kw), seen


def formula(N, freq, f, l):
    """nu = (freq N - (f + l/2)) / l, the numerator wrapped to the representative nearest zero modulo N; exact rational arithmetic"""
    d = Fraction(freq) * N - (f + Fraction(l, 2))
    d -= N * math.floor(d / N + Fraction(1, 2))
    return float(d / l)


def test_hier_block_fine_nu_against_the_formula(monkeypatch):
    N = 4096
    # user frequencies (normalized mode: internal = user + 0.5): an ordinary channel; one whose carrier rounds to bin N = bin 0, so that its slice starts
    # below zero and is wrapped (get_opt_channelparams then clamps every wrapped slice to [N - l, N)); one clamped at the upper edge; one exactly on a bin
    user = [[0.1003, 0.05], [0.5 - 0.3 / N, 0.05], [0.4901, 0.05], [1000.0 / N - 0.5, 0.01]]
    fdc, seen = _mirror(monkeypatch, throughput_channels=user, fine_tuning=True)
    assert len(fdc.fine_nu) == 4
    kinds = []
    for (u, bw), nu, (f, l, _lo, _p, _s), ch in zip(user, fdc.fine_nu, fdc.channel_params, seen["channels"]):
        freq = fdc.get_freq(u)
        assert (f, l) == tuple(ch[:2])
        assert nu == pytest.approx(formula(N, freq, f, l), abs=1e-12), (u, f, l)
        assert abs(nu) < 0.5
        centre = int(G.channelizer._round_half_away(freq * N)) % N
        kinds.append("wrapped" if centre - l // 2 < 0 else "clamped" if centre - l // 2 + l > N else "plain")
    assert kinds == ["plain", "wrapped", "clamped", "plain"], kinds
    assert fdc.fine_nu[3] == 0.0 and 0.0 < abs(fdc.fine_nu[0]) <= 0.5 / fdc.channel_params[0][1] + 1e-12
    # the wrapped slice: the numerator is taken modulo N (the carrier at N - 0.3 is 0.3 bin below bin 0 = l/2 - 0.3 above the centre of [N - l, N))
    l1 = fdc.channel_params[1][1]
    assert fdc.channel_params[1][0] == N - l1 and fdc.fine_nu[1] == pytest.approx(0.5 - 0.3 / l1, abs=1e-9)
    assert fdc.fine_nu[2] > 0.25                                  # clamped: the carrier is far from the centre of its slice
    np.testing.assert_array_equal(seen["nu"], np.array(fdc.fine_nu))
    # off by default: nothing is set
    fdc, seen = _mirror(monkeypatch, throughput_channels=user)
    assert fdc.fine_nu is None and "nu" not in seen


@pytest.mark.parametrize("change", [
    dict(inpveclen=4096),
    dict(activity_controlled_channels=[[0.2, 0.01]]),
    dict(activity_detection_segments=[[0.1, 0.3]]),
    dict(waterfall=object()),
    dict(throughput_channels=[[-0.49999, 0.05]]),
], ids=["inpveclen > 1", "power-activation sinks", "detection segments", "waterfall", "carrier outside its clamped slice"])
def test_hier_block_refusals(change, monkeypatch):
    kw = dict(KW, inptype=8, fine_tuning=True)
    kw.update(change)
    with pytest.raises(ValueError):
        G.FrequencyDomainChannelizer(**kw)


def test_the_clamped_refusal_is_the_half_cycle_rule(monkeypatch):
    # the carrier at 0.04 bin: the slice is wrapped, then clamped to [N - l, N): the carrier lies l/2 + 0.04 bins from its centre
    fdc, _ = _mirror(monkeypatch, throughput_channels=[[-0.49999, 0.05]])
    f, l = fdc.channel_params[0][:2]
    assert f + l == 4096 and abs(formula(4096, fdc.get_freq(-0.49999), f, l)) >= 0.5


def test_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdc_amd.h")).read()
    ctype = {"fdc_pipeline *p": C.c_void_p, "fdc_pipeline_group *g": C.c_void_p, "const double *nu": C.POINTER(C.c_double), "int n": C.c_int,
             "double nu": C.c_double, "uint64_t *inc": C.POINTER(C.c_uint64)}
    for name in ("fdc_fine_tuning_increment", "fdc_pipeline_set_fine_tuning", "fdc_pipeline_group_set_fine_tuning"):
        m = re.search(r"\bint %s\(([^)]*)\);" % name, hdr)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int, name
        assert [ctype[a] for a in args] == list(argtypes), (name, args)
        assert hasattr(G.lib(), name)
    assert callable(G.Pipeline.set_fine_tuning) and callable(G.PipelineGroup.set_fine_tuning) and callable(G.fine_tuning_increment)
