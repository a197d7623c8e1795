"""GPU tests (-m gpu) of the channel lag-1 correlation on every plan, together with every other setting, and inside its kernel (tests/test_lag1_gpu.py
covers the setting itself and the call forms; its helpers and the models of tests/lag1_model.py are used here).

One piece of device code sums it: k_chan_lag1 (csrc/fdc_postpass.hip), a pass of its own over a launch group's final float results, behind the rotation,
the gain pass and the copies of channels with the same slice, in front of whatever narrows; where the gain pass narrows and leaves the float results as
they were cut, the pass multiplies what it reads.  Each case here is a plan, a route of the passes in front of it, or an index, an offset or a branch of
the kernel.

crossed() is the cross the plans go through: float and sc16 input x fine tuning off and on x gains off and on, and for each of these eight the float
samples of the call with lag-1 off are THE reference (the models of tests/lag1_model.py on every row of every channel: the bound against float64, the bits
of the float32 model); then levels off and on x float, sc16 and sc8 output with lag-1 on, whose six results are bit-equal to each other and whose outputs
are the reference's bytes, or its narrowed bytes."""
import functools

import numpy as np
import pytest

import gr_fdc_amd as G
from test_fine_tuning_gpu import BANK, FORCED, narrowed, signal
from test_fine_tuning_routes_gpu import ALIAS_N, LONG, TINY, TINY_R, alias_plan, edge_nus, int_scale
from test_fused4096_gpu import plans as fused_plans
from test_iq_input_gpu import iq, plans as iq_plans, same_bytes
from test_iq_output_gpu import EXTRA
from test_lag1_gpu import checked, lag1_hold

pytestmark = pytest.mark.gpu
OUT = ((None, None), ("sc16", np.int16), ("sc8", np.int8))
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


def crossed(p, nb, H, seed, what, keep=False, inputs=("fc32", "sc16"), fines=(False, True), gains=(False, True), levels=(False, True), outs=OUT):
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
                p.set_levels(False)
                p.set_lag1(False)
                p.set_output_format(None)
                p.reset()
                ref = call()
                s0 = None
                for lev in levels:
                    for ofmt, odt in outs:
                        scale = int_scale(ref, odt) if ofmt else 1.0
                        p.set_output_format(ofmt, scale)
                        p.set_levels(lev)
                        p.set_lag1(True)
                        p.reset()
                        got = call()
                        s, d = p.lag1(), p.describe()
                        this = "%s, levels %s, %s out" % (case, "on" if lev else "off", ofmt or "fc32")
                        for c, (u, v) in enumerate(zip(got, ref)):
                            same_bytes(u, narrowed(v, scale, odt) if ofmt else v, "%s, ch%d" % (this, c))
                        if s0 is None:
                            lag1_hold(p, ref, s, this)
                            s0 = s
                        else:
                            same_bytes(s, s0, this + ": S against the first of the six")
                        assert "lag1: pass" in d and ("fine tuning: " in d) == fine and ("gains: " in d) == gain and ("levels: " in d) == lev, (this, d)
                        assert not ofmt or ("output %s: narrowed" % ofmt) in d, (this, d)
                        seen.append(d)
    for h in (p.set_fine_tuning, p.set_gains, p.set_output_format):
        h(None)
    p.set_levels(False)
    p.set_lag1(False)
    return seen


# ---- 1. path 5: k_f4096 (or its FINE form) writes float, the pass behind it --------------------------------------------------------------------------------

F4 = list(fused_plans().items())


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("k", range(len(F4)), ids=[name for name, _ in F4])
def test_every_plan_of_the_one_launch_kernel(k, R):
    """The plans of test_fused4096_gpu.py at 1 and 5 blocks: lout = l - l / R from 8 to 768, rows of a few lanes to rows of six trips of a wave"""
    name, chans = F4[k]
    N = 4096
    H = N - N // R
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=5)
    for nb in (1, 5):
        seen = crossed(p, nb, H, 100 + R, "%s R=%d" % (name, R))
        assert FORCED or (p.path() == 5 and all("fine tuning: fused" in d for d in seen if "fine tuning" in d)), (name, p.path())


@pytest.mark.parametrize("R", [2, 4])
def test_launch_groups_of_path_5(R):
    """chunk_blocks = 2: five blocks are three launches at mbase 0, 2, 4; the row is the block of the CALL"""
    N, nb = 4096, 5
    H = N - N // R
    chans = fused_plans()["narrow channels: 128 and 64 bins beside the example"]
    x = stream(nb * H, 100 + R)
    res = []
    for chunk in (0, 2):
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, chunk_blocks=chunk)
        assert chunk == 0 or p.chunk_blocks() == 2
        _got, s, d = checked(p, lambda: p.work(x), "chunk_blocks %d R=%d" % (chunk, R))
        assert FORCED or p.path() == 5, d
        res.append(s)
        if chunk:
            crossed(p, nb, H, 100 + R, "chunk_blocks 2, R=%d" % R)
    same_bytes(res[1], res[0], "chunk_blocks 2 against 0")


# ---- 2. every other path -----------------------------------------------------------------------------------------------------------------------------------

OTHERS = [c for c in iq_plans() if "k_f4096" not in c[0]] + EXTRA


@pytest.mark.parametrize("k", range(len(OTHERS)), ids=[c[0] for c in OTHERS])
def test_the_pass_behind_every_other_route(k):
    """paths 0 and 1, path 2 (two launches), path 3 (k_blk256 on the grid / OFF / HALF / R = 4, k_blk512, k_blk1024, k_blknar), path 4 (a split plan with a
    remainder), and the keep_spectrum handles.  Off path 5 the cross reaches the rotation route (fine tuning on: the rotation multiplies and sums the
    levels too), the in-place gain route (float output) and the narrowing gain route (integer output, which leaves the float results as they were cut)."""
    name, N, R, chans, flags, _r_in, keep = OTHERS[k]
    H, nb = N - N // R, (3 if N >= 65536 else 5)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
    path = p.path()
    seen = crossed(p, nb, H, 200 + N // 4096 + R, name, keep=keep)
    assert p.path() == path
    if not FORCED and path != 5:
        for route in ("fine tuning: rotated", "gains: with the rotation", "gains: pass", "gains: with the narrowing", "levels: with the rotation",
                      "levels: with the gains", "levels: pass"):
            assert any(route in d for d in seen), (name, route)


def test_copies_of_channels_with_the_same_slice():
    """bank_alias: a channel with an earlier channel's slice is a device-to-device copy of that channel's rows, made in front of the passes; it has its own
    entry, with the same bits — and with its own gain and fine tuning, which the cross gives it, its own value"""
    N, R, nb = ALIAS_N, 2, 5
    H = N - N // R
    plan = alias_plan(N)
    first = len(set(plan))
    x = stream(nb * H, 200 + N // 4096 + R)
    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
    got, s, d = checked(p, lambda: p.work(x), "slots twice")
    for c in range(first, len(plan)):
        same_bytes(got[c], got[c - first], "ch%d is a copy of ch%d" % (c, c - first))
        same_bytes(s[:, c], s[:, c - first], "S of ch%d and ch%d" % (c, c - first))
    if not FORCED:
        assert p.path() == 3 and "copies of channels with the same slice" in d, d
    crossed(p, nb, H, 200 + N // 4096 + R, "slots twice")


def test_short_groups_under_the_default_dispatch():
    """Without FDC_BLOCK_MIN_BLOCKS (conftest.py sets 1) a launch group of fewer than 96 blocks takes the two-launch form: 100 blocks in groups of 96 run
    96 on the block kernel and 4 on stage 1 + stage 2, with the pass at mbase = 96 behind them"""
    N, R, nb = 16384, 2, 100
    H = N - N // R
    saved = G.defaults.pop("FDC_BLOCK_MIN_BLOCKS", None)
    try:
        p = G.Pipeline(N, R, BANK, windowtype=1, max_blocks=nb, chunk_blocks=96)
    finally:
        if saved is not None:
            G.defaults["FDC_BLOCK_MIN_BLOCKS"] = saved
    assert p.chunk_blocks() == 96
    seen = crossed(p, nb, H, 22, "96 + 4 blocks")
    assert FORCED or p.path() == 3, seen[0]


def test_chunk_blocks_below_the_call():
    """a bank in launch groups of 2 of a call of 5 (mbase = 0, 2, 4) against the same call in one group"""
    N, R, nb = 16384, 2, 5
    H = N - N // R
    x = stream(nb * H, 30)
    res = []
    for chunk in (0, 2):
        p = G.Pipeline(N, R, BANK, windowtype=1, max_blocks=nb, chunk_blocks=chunk)
        _got, s, _d = checked(p, lambda: p.work(x), "chunk_blocks %d" % chunk)
        res.append(s)
        if chunk:
            assert p.chunk_blocks() == 2
            crossed(p, nb, H, 30, "bank, chunk_blocks 2")
    same_bytes(res[1], res[0], "chunk_blocks 2 against 0")


# ---- 3. inside k_chan_lag1 ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", TINY_R)
def test_the_8_byte_branch_and_tiny_rows(R):
    """lout = 1 (no term: (+0, +0)), lout = 2 (the second term of pair 0 only), odd lout (R = 16: lout = 15 from l = 16, the 8-byte branch and a last pair
    without its second term), rows of 6 to 15 samples (several rows per wave: lane sub = 0 of every row has no predecessor), rows of two and three steps of
    a wave (lout = 192 and 240: the first term of lane 0's pair looks back at the pair of lane 63 of the step before) and of more than one trip (lout =
    768 to 960: at the pair behind a trip), and even lout behind an odd offset (16 bytes per lane only where the channel's run is 16-byte aligned)"""
    N, nb = 8192, 5
    H = N - N // R
    p = G.Pipeline(N, R, TINY, windowtype=1, max_blocks=nb)
    off = [p.channel_offset(c, nb) for c in range(len(TINY))]
    assert 1 in p.lout and 2 in p.lout and any(1 < lo <= 32 for lo in p.lout) and max(p.lout) > 512, p.lout
    assert (R == 16) == (15 in p.lout) and (R == 4) == (768 in p.lout and 192 in p.lout and 12 in p.lout) and (R != 16 or 8 in p.lout), p.lout
    assert R == 16 or any(lo % 2 == 0 and o % 2 for lo, o in zip(p.lout, off)), (p.lout, off)
    crossed(p, nb, H, 200 + N // 4096 + R, "tiny rows R=%d" % R)
    assert FORCED or p.path() == 0
    # lout = 1 and its neighbours' bits: +0, not -0
    p.set_lag1(True)
    p.reset()
    p.work(stream(nb * H, 200 + N // 4096 + R))
    assert np.ascontiguousarray(p.lag1()[:, p.lout.index(1)]).view(np.uint32).tolist() == [0] * (2 * nb)
    p.set_lag1(False)


def test_one_pair_per_lane_and_rows_of_two_steps():
    """lout = 128 (exactly one pair for each of 64 lanes: the four-rows-a-trip branch at its limit), 256 (two steps of a wave) and 512, on the spectrum
    path and on path 5 (the example plan: l = 256, 512, 1024 at R = 2)"""
    N, R, nb = 4096, 2, 5
    H = N - N // R
    chans = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]
    for flags in (0, G.FDC_PIPE_NO_FUSED):
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags)
        assert p.lout == [128, 256, 512, 256]
        crossed(p, nb, H, 40, "lout 128, 256, 512, flags %d" % flags)


def test_rows_longer_than_a_wave():
    """lout = 6144, 12288 and 24576 (channels above 4096 bins): every lane of a wave takes 48 to 192 sample pairs of a row, four a trip; the predecessor
    of the first pair of a trip is the last sample of the trip before"""
    N, R, nb = 32768, 4, 3
    H = N - N // R
    p = G.Pipeline(N, R, LONG, windowtype=1, max_blocks=nb)
    assert max(p.lout) == 24576 and min(p.lout) // 2 > 64
    crossed(p, nb, H, 200 + N // 4096 + R, "long rows")


def test_more_blocks_than_one_trip_of_the_grid_stride_loop():
    """launch_chan_lag1 gives gx = max(1, min(ceil(nb / 4), ceil(2048 / channels))) workgroups of four waves to every channel; a wave takes 64 >> lg rows
    a step and four steps a trip, lg = min(6, ceil(log2(ceil(lout / 2)))): 256 channels of lout = 128 and 140 blocks are more than 128 rows a trip.
    (lag-1 alone, and on top of fine tuning, gains and levels with sc16 output: two calls of this size, not the cross)"""
    N, R, nb = 65536, 2, 140
    H = N - N // R
    chans = [(256 * c, 256, 0.88, 1.0) for c in range(256)]
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb)
    nc = len(chans)
    gx = max(1, min((nb + 3) // 4, (2048 + nc - 1) // nc))
    for lo in set(p.lout):
        npair = (lo + 1) // 2
        rows = 64 >> min(6, 0 if npair <= 1 else (npair - 1).bit_length())
        assert nb > 4 * 4 * gx * rows, (gx, rows)
    x = signal(nb * H, 23)
    checked(p, lambda: p.work(x), "140 blocks of the full bank")
    p.set_fine_tuning(edge_nus(nc, 9))
    p.set_gains(draw_gains(nc, 9))
    ref, s, _d = checked(p, lambda: p.work(x), "140 blocks, fine tuning and gains")
    p.set_output_format("sc16", int_scale(ref, np.int16))
    p.set_levels(True)
    p.set_lag1(True)
    p.reset()
    p.work(x)
    same_bytes(p.lag1(), s, "140 blocks, fine tuning, gains, levels, sc16 output")
    assert FORCED or p.path() == 3
