"""GPU tests (-m gpu) of the channel demodulation on every plan, together with fine tuning and the gains, and inside its kernel (tests/test_demod_gpu.py
covers the setting itself and the call forms; its helpers and the models of tests/demod_model.py are used here).

One piece of device code demodulates: k_chan_demod (csrc/fdc_postpass.hip), once behind the last launch group of an enqueue-path call over the call's
whole float staging, behind the rotation, the gain pass and the copies of channels with the same slice.  Each case here is a plan, a route of the passes
in front of it, or an index, an offset or a branch of the kernel.

crossed() is the cross the plans go through: float and sc16 input x fine tuning off and on x gains off and on; for each of these eight the complex
float samples of the call with the setting off are THE reference of both modes (FM: every sample inside its bound; MAG: numpy's float32 bits)."""
import functools

import numpy as np
import pytest

import gr_fdc_amd as G
from test_demod_gpu import CYCLES, MODES, bits, checked, demod_hold
from test_fine_tuning_gpu import BANK, FORCED, signal
from test_fine_tuning_routes_gpu import ALIAS_N, LONG, TINY, TINY_R, alias_plan, edge_nus
from test_fused4096_gpu import plans as fused_plans
from test_iq_input_gpu import iq, plans as iq_plans, same_bytes
from test_iq_output_gpu import EXTRA

pytestmark = pytest.mark.gpu
IQ_SCALE = 2.0 ** -14


@functools.lru_cache(maxsize=4)
def stream(n, seed):
    """the float input of the cases that share one (read only)"""
    x = signal(n, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=4)
def istream(n, seed):
    """the sc16 input likewise"""
    x = iq(n, np.int16, seed)
    x.setflags(write=False)
    return x


def draw_gains(nchan, seed):
    """one finite gain per channel, neither 1 nor a power of two: of both signs, within a factor of 4 of one"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.25, 4.0, nchan) * rng.choice([-1.0, 1.0], nchan)).astype(np.float32)


def crossed(p, nb, H, seed, what, keep=False, inputs=("fc32", "sc16"), fines=(False, True), gains=(False, True)):
    """the cross of the module's docstring on handle p at nb blocks; returns the describe() strings it saw"""
    nchan = len(p.lout)
    xf, xi = stream(nb * H, seed), istream(nb * H, seed + 1)
    nu, g = edge_nus(nchan, seed), draw_gains(nchan, seed)
    calls = {"fc32": (lambda: p.work(xf, want_spectrum=True)[0]) if keep else (lambda: p.work(xf)),
             "sc16": (lambda: p.work_iq(xi, scale=IQ_SCALE, want_spectrum=True)[0]) if keep else (lambda: p.work_iq(xi, scale=IQ_SCALE))}
    seen = []
    for ifmt in inputs:
        call = calls[ifmt]
        for fine in fines:
            for gain in gains:
                case = "%s, %d blocks, %s in, fine tuning %s, gains %s" % (what, nb, ifmt, "on" if fine else "off", "on" if gain else "off")
                p.set_fine_tuning(nu if fine else None)
                p.set_gains(g if gain else None)
                p.set_demod(None)
                p.reset()
                ref = call()
                for mode, dg in MODES:
                    p.set_demod(mode, dg)
                    p.reset()
                    got = call()
                    d = p.describe()
                    demod_hold(ref, got, mode, dg, "%s, %s" % (case, mode))
                    assert ("demod: %s" % mode) in d and ("fine tuning: " in d) == fine and ("gains: " in d) == gain and "; output " not in d, (case, d)
                    seen.append(d)
    p.set_fine_tuning(None)
    p.set_gains(None)
    p.set_demod(None)
    return seen


# ---- 1. path 5: k_f4096 (or its FINE form) writes float into the staging, the pass behind it ----------------------------------------------------------------

F4 = list(fused_plans().items())


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("k", range(len(F4)), ids=[name for name, _ in F4])
def test_every_plan_of_the_one_launch_kernel(k, R):
    """The plans of test_fused4096_gpu.py at 1 and 5 blocks: lout = l - l / R from 8 to 768"""
    name, chans = F4[k]
    N = 4096
    H = N - N // R
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=5)
    for nb in (1, 5):
        seen = crossed(p, nb, H, 100 + R, "%s R=%d" % (name, R))
        assert FORCED or (p.path() == 5 and all("fine tuning: fused" in d for d in seen if "fine tuning" in d)), (name, p.path())


# ---- 2. every other path -----------------------------------------------------------------------------------------------------------------------------------

OTHERS = [c for c in iq_plans() if "k_f4096" not in c[0]] + EXTRA


@pytest.mark.parametrize("k", range(len(OTHERS)), ids=[c[0] for c in OTHERS])
def test_the_pass_behind_every_other_route(k):
    """paths 0 and 1, path 2 (two launches), path 3 (k_blk256 on the grid / OFF / HALF / R = 4, k_blk512, k_blk1024, k_blknar), path 4 (a split plan with a
    remainder), and the keep_spectrum handles"""
    name, N, R, chans, flags, _r_in, keep = OTHERS[k]
    H, nb = N - N // R, (3 if N >= 65536 else 5)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
    path = p.path()
    seen = crossed(p, nb, H, 200 + N // 4096 + R, name, keep=keep)
    assert p.path() == path
    if not FORCED and path != 5:
        for route in ("fine tuning: rotated", "gains: with the rotation", "gains: pass"):
            assert any(route in d for d in seen), (name, route)


def test_copies_of_channels_with_the_same_slice():
    """bank_alias: a channel with an earlier channel's slice is a device-to-device copy of that channel's rows in the float staging, made in front of
    the pass: the same demodulated bits, and its own carry"""
    N, R, nb = ALIAS_N, 2, 5
    H = N - N // R
    plan = alias_plan(N)
    first = len(set(plan))
    x = stream(nb * H, 200 + N // 4096 + R)
    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
    for mode, dg in MODES:
        _y, got = checked(p, lambda: p.work(x), mode, dg, "slots twice")
        parts = []
        p.reset()
        for a, b in ((0, 2), (2, 5)):
            parts.append(p.work(x[a * H:b * H]))
        for c in range(len(plan)):
            same_bytes(np.concatenate([q[c] for q in parts]), got[c], "2 + 3 blocks, ch%d" % c)
        for c in range(first, len(plan)):
            same_bytes(got[c], got[c - first], "ch%d is a copy of ch%d" % (c, c - first))
    if not FORCED:
        assert p.path() == 3 and "copies of channels with the same slice" in p.describe(), p.describe()
    crossed(p, nb, H, 200 + N // 4096 + R, "slots twice", inputs=("fc32",))


def test_short_groups_under_the_default_dispatch():
    """Without FDC_BLOCK_MIN_BLOCKS (conftest.py sets 1) a launch group of fewer than 96 blocks takes the two-launch form: 100 blocks in groups of 96 run
    96 on the block kernel and 4 on stage 1 + stage 2, and the pass runs once behind both over the call's 100 blocks"""
    N, R, nb = 16384, 2, 100
    H = N - N // R
    saved = G.defaults.pop("FDC_BLOCK_MIN_BLOCKS", None)
    try:
        p = G.Pipeline(N, R, BANK, windowtype=1, max_blocks=nb, chunk_blocks=96)
    finally:
        if saved is not None:
            G.defaults["FDC_BLOCK_MIN_BLOCKS"] = saved
    assert p.chunk_blocks() == 96
    seen = crossed(p, nb, H, 22, "96 + 4 blocks", inputs=("fc32",), fines=(True,), gains=(True,))
    seen += crossed(p, nb, H, 22, "96 + 4 blocks", inputs=("sc16",), fines=(False,), gains=(False,))
    assert FORCED or p.path() == 3, seen[0]


def test_chunk_blocks_below_the_call():
    """a bank in launch groups of 2 of a call of 5 (mbase = 0, 2, 4) against the same call in one group: one pass over the whole call either way"""
    N, R, nb = 16384, 2, 5
    H = N - N // R
    x = stream(nb * H, 30)
    for mode, dg in MODES:
        res = []
        for chunk in (0, 2):
            p = G.Pipeline(N, R, BANK, windowtype=1, max_blocks=nb, chunk_blocks=chunk)
            res.append(checked(p, lambda: p.work(x), mode, dg, "chunk_blocks %d" % chunk)[1])
            assert chunk == 0 or p.chunk_blocks() == 2
        for c in range(len(BANK)):
            same_bytes(res[1][c], res[0][c], "chunk_blocks 2 against 0, ch%d" % c)
    crossed(p, nb, H, 30, "bank, chunk_blocks 2")


# ---- 3. inside k_chan_demod -----------------------------------------------------------------------------------------------------------------------------------

def runs_of(p, nb):
    """(offset, length) of every channel's run of a call of nb blocks, in elements"""
    return [(p.channel_offset(c, nb), nb * lo) for c, lo in enumerate(p.lout)]


def grid_waves(p, nb):
    """the waves launch_chan_demod gives every channel: 4 gx, gx = max(1, min(ceil(trips / 4), ceil(2048 / channels))), trips = ceil(mean run / 256)"""
    nc = len(p.lout)
    trips = max(1, (nb * sum(p.lout) // nc + 255) // 256)
    return 4 * max(1, min((trips + 3) // 4, (2048 + nc - 1) // nc))


@pytest.mark.parametrize("R", TINY_R)
def test_both_branches_and_tiny_rows(R):
    """lout = 1, 2, 3 (R = 4: l = 4) and 15 (R = 16: l = 16); runs whose float offset nblocks * out_off is no multiple of 4 (the narrow branch: 8-byte loads,
    4-byte stores) beside runs where it is (two 16-byte loads, one 16-byte store), the last lane of a wide run with fewer than four samples; runs shorter
    than a lane's four samples (1 block), runs that end inside a wave, runs with a wave boundary inside (lane 0's extra load); at 5 blocks, at 4 (every
    offset a multiple of 4) and at 1"""
    N = 8192
    H = N - N // R
    plan = TINY + ([(600, 4, 1., 1.)] if R == 4 else [])
    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=5)
    assert 1 in p.lout and 2 in p.lout and (R != 4 or 3 in p.lout) and (R != 16 or 15 in p.lout), p.lout
    kinds = set()
    for nb in (5, 4, 1):
        for off, n in runs_of(p, nb):
            kinds.add(("wide" if off % 4 == 0 else "narrow", "short" if n < 4 else "inside a wave" if n <= 256 else "several waves",
                       "whole lanes" if n % 4 == 0 else "ragged"))
        crossed(p, nb, H, 200 + N // 4096 + R + nb, "tiny rows R=%d" % R, inputs=("fc32", "sc16") if nb == 5 else ("fc32",))
    for need in (("wide", "several waves"), ("narrow", "several waves"), ("narrow", "inside a wave"), ("wide", "inside a wave")):
        assert any(k[:2] == need for k in kinds), (need, sorted(kinds))
    assert any(k[0] == "narrow" and k[1] == "short" for k in kinds) or any(k[0] == "wide" and k[1] == "short" for k in kinds), sorted(kinds)
    assert any(k[0] == "wide" and k[2] == "ragged" for k in kinds) or R != 16, sorted(kinds)
    assert FORCED or p.path() == 0
    # lout = 1: one sample a block, each against the block before; the first of the stream is +0.0
    p.set_demod("fm", CYCLES)
    p.reset()
    d = p.work(stream(5 * H, 1))[p.lout.index(1)]
    assert d.shape == (5,) and bits(d[:1]).tolist() == [0] and (d[1:] != 0).all()
    p.set_demod(None)


def test_runs_that_end_inside_a_wave_and_on_a_wave():
    """lout = 128, 256, 512 (the example plan) at 1, 2, 3 and 5 blocks: runs of exactly 256 samples and multiples (a run boundary on a wave boundary), of
    128 and 384 (inside a wave), on the spectrum path and on path 5; every count cut into single blocks gives the same bits"""
    N, R = 4096, 2
    H = N - N // R
    chans = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]
    for flags in (0, G.FDC_PIPE_NO_FUSED):
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=5, flags=flags)
        assert p.lout == [128, 256, 512, 256]
        for nb in (1, 2, 3, 5):
            x = stream(5 * H, 40)[:nb * H]
            for mode, dg in MODES:
                _y, got = checked(p, lambda: p.work(x), mode, dg, "lout 128, 256, 512, flags %d, %d blocks" % (flags, nb))
                p.reset()
                parts = [p.work(x[j * H:(j + 1) * H]) for j in range(nb)]
                for c in range(len(chans)):
                    same_bytes(np.concatenate([q[c] for q in parts]), got[c], "%d single blocks, ch%d" % (nb, c))
            p.set_demod(None)


def test_rows_of_24576_samples_and_a_second_trip_of_the_grid_stride_loop():
    """lout = 6144, 12288 and 24576 (channels above 4096 bins) at 3 blocks: the grid is sized for the mean run, so the longest run takes every wave of
    its channel through the loop more than once; the element in front of a wave's 256 samples is the last one of another wave's, of the trip before"""
    N, R, nb = 32768, 4, 3
    H = N - N // R
    p = G.Pipeline(N, R, LONG, windowtype=1, max_blocks=nb)
    assert max(p.lout) == 24576
    assert nb * max(p.lout) > 256 * grid_waves(p, nb) >= nb * min(p.lout), (grid_waves(p, nb), p.lout)
    crossed(p, nb, H, 200 + N // 4096 + R, "long rows", inputs=("fc32",))
    x = stream(nb * H, 200 + N // 4096 + R)
    for mode, dg in MODES:
        _y, got = checked(p, lambda: p.work(x), mode, dg, "long rows")
        p.reset()
        parts = [p.work(x[:H]), p.work(x[H:])]
        for c in range(len(LONG)):
            same_bytes(np.concatenate([q[c] for q in parts]), got[c], "1 + 2 blocks, ch%d" % c)
