"""GPU tests (-m gpu) of the channel levels on every plan, inside the two kernels that sum them, and together with the other settings
(tests/test_levels_gpu.py covers the setting itself and the call forms; its helpers and the model of tests/test_levels_cpu.py are used here).

Two pieces of device code sum levels: k_chan_levels, one pass over a launch group's float results behind the channel kernels of every plan (path 5
included), and k_fine_rotate<true>, the rotation's pass when fine tuning is on too, off path 5 (csrc/fdc_postpass.hip; launched per launch group by
process_device_impl).  Each case here is an index, an offset or a dispatch decision of one of them.  Every comparison is against the model applied to the
float32 outputs of the same call: the bound for power, bit-equality for peak; the outputs are byte-equal to the same handle's with levels off."""
import functools

import numpy as np
import pytest

import gr_fdc_amd as G
from test_fine_tuning_gpu import BANK, FORCED, narrowed, signal
from test_fine_tuning_routes_gpu import ALIAS_N, LONG, TINY, TINY_R, alias_plan, edge_nus, int_scale
from test_fused4096_gpu import EXAMPLE, plans as fused_plans
from test_iq_input_gpu import iq, plans as iq_plans, same_bytes
from test_iq_output_gpu import EXTRA
from test_levels_gpu import checked, levels_hold, on_and_off

pytestmark = pytest.mark.gpu
FORMATS = (("sc16", np.int16, 32767.5), ("sc8", np.int8, 127.5))


@functools.lru_cache(maxsize=4)
def stream(n, seed):
    """the input of the cases that share one (read only)"""
    x = signal(n, seed)
    x.setflags(write=False)
    return x


# ---- 1. path 5: k_f4096 writes float, k_chan_levels behind it ---------------------------------------------------------------------------------------------

F4 = list(fused_plans().items())


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("k", range(len(F4)), ids=[name for name, _ in F4])
def test_every_plan_of_the_one_launch_kernel(k, R):
    """The 17 plans of test_fused4096_gpu.py at 1 and 5 blocks: lout = l - l / R from 8 to 768, rows of one lane to rows of six trips of a wave"""
    name, chans = F4[k]
    N = 4096
    H = N - N // R
    x = stream(5 * H, 100 + R)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=5)
    for nb in (1, 5):
        _got, _lev, d = checked(p, lambda: p.work(x[:nb * H]), "%s R=%d nb=%d" % (name, R, nb))
        assert "levels: pass" in d, d
        assert FORCED or p.path() == 5, (name, p.path())


@pytest.mark.parametrize("R", [2, 4])
def test_launch_groups_of_path_5(R):
    """chunk_blocks = 2: five blocks are three launches at mbase 0, 2, 4; the levels' row is the block of the CALL"""
    N, nb = 4096, 5
    H = N - N // R
    chans = fused_plans()["narrow channels: 128 and 64 bins beside the example"]
    x = stream(5 * H, 100 + R)
    levs = []
    for chunk in (0, 2):
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, chunk_blocks=chunk)
        assert chunk == 0 or p.chunk_blocks() == 2
        _got, lev, d = checked(p, lambda: p.work(x), "chunk_blocks %d R=%d" % (chunk, R))
        assert "levels: pass" in d and (FORCED or p.path() == 5), d
        levs.append(lev)
    same_bytes(levs[1], levs[0], "chunk_blocks 2 against 0")


def test_a_spectrum_call_between_plain_calls():
    """keep_spectrum: work, work(want_spectrum=True), work.  The middle call runs the spectrum path, the outer ones the one-launch kernel; each call's levels
    are of that call's samples, and the spectrum is what the handle returns with levels off."""
    N, R, nb = 4096, 4, 3
    H = N - N // R
    x = signal(3 * nb * H, 21)
    p = G.Pipeline(N, R, EXAMPLE, windowtype=1, max_blocks=nb, keep_spectrum=True)
    levs = []

    def three_calls():
        res = []
        for k in range(3):
            res.append(p.work(x[k * nb * H:(k + 1) * nb * H], want_spectrum=(k == 1)))
            if p.levels_device() is not None:
                levs.append(p.levels())
        return res

    got, _lev, _d, plain = on_and_off(p, three_calls)
    for k in range(3):
        a, b = (got[k][0], plain[k][0]) if k == 1 else (got[k], plain[k])
        for c, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, "call %d ch%d" % (k, c))
        levels_hold(p, a, levs[k], "call %d of three" % k)
    same_bytes(got[1][1], plain[1][1], "the spectrum of the middle call")
    assert np.abs(plain[1][1]).max() > 0 and len(levs) == 3


# ---- 2. every other path -----------------------------------------------------------------------------------------------------------------------------------

OTHERS = [c for c in iq_plans() if "k_f4096" not in c[0]] + EXTRA


@pytest.mark.parametrize("k", range(len(OTHERS)), ids=[c[0] for c in OTHERS])
def test_the_pass_behind_every_other_route(k):
    """paths 0 and 1, path 2 (two launches), path 3 (k_blk256 on the grid / OFF / HALF / R = 4, k_blk512, k_blk1024, k_blknar), path 4 (a split plan with a
    remainder), and the keep_spectrum handles"""
    name, N, R, chans, flags, _r_in, keep = OTHERS[k]
    H, nb = N - N // R, (3 if N >= 65536 else 5)
    x = stream(nb * H, 200 + N // 4096 + R)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
    path = p.path()
    if keep:
        got, lev, d, plain = on_and_off(p, lambda: p.work(x, want_spectrum=True))
        same_bytes(got[1], plain[1], "%s: the spectrum" % name)
        for c, (u, v) in enumerate(zip(got[0], plain[0])):
            same_bytes(u, v, "%s ch%d" % (name, c))
        levels_hold(p, got[0], lev, name)
    else:
        _got, _lev, d = checked(p, lambda: p.work(x), name)
    assert p.path() == path and "levels: pass" in d, (name, d)


def test_copies_of_channels_with_the_same_slice():
    """bank_alias: a channel with an earlier channel's slice is a device-to-device copy of that channel's rows; it has its own entry, with the same bits"""
    N, R, nb = ALIAS_N, 2, 5
    H = N - N // R
    plan = alias_plan(N)
    first = len(set(plan))
    x = stream(nb * H, 200 + N // 4096 + R)
    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
    got, lev, d = checked(p, lambda: p.work(x), "slots twice")
    for c in range(first, len(plan)):
        same_bytes(got[c], got[c - first], "ch%d is a copy of ch%d" % (c, c - first))
        same_bytes(lev[:, c], lev[:, c - first], "levels of ch%d and ch%d" % (c, c - first))
    if not FORCED:
        assert p.path() == 3 and "copies of channels with the same slice" in d, d


def test_short_groups_under_the_default_dispatch():
    """Without FDC_BLOCK_MIN_BLOCKS (conftest.py sets 1) a launch group of fewer than 96 blocks takes the two-launch form: 100 blocks in groups of 96 run
    96 on the block kernel and 4 on stage 1 + stage 2, levelled with mbase = 96.  The same with sc16 output (float, levels, narrow: one layout per call)."""
    N, R, nb = 16384, 2, 100
    H = N - N // R
    x = signal(nb * H, 22)
    saved = G.defaults.pop("FDC_BLOCK_MIN_BLOCKS", None)
    try:
        p = G.Pipeline(N, R, BANK, windowtype=1, max_blocks=nb, chunk_blocks=96)
    finally:
        if saved is not None:
            G.defaults["FDC_BLOCK_MIN_BLOCKS"] = saved
    assert p.chunk_blocks() == 96
    got, lev, d = checked(p, lambda: p.work(x), "96 + 4 blocks")
    assert FORCED or p.path() == 3, d
    scale = int_scale(got, np.int16)
    p.set_levels(True)
    p.set_output_format("sc16", scale)
    p.reset()
    gi = p.work(x)
    same_bytes(p.levels(), lev, "96 + 4 blocks, sc16 out: the levels")
    for c, (u, v) in enumerate(zip(gi, got)):
        same_bytes(u, narrowed(v, scale, np.int16), "96 + 4 blocks, sc16 out, ch%d" % c)
    assert "levels: pass" in p.describe() and "output sc16: narrowed" in p.describe(), p.describe()


# ---- 3. inside k_chan_levels (and k_fine_rotate<true> with fine tuning on) ------------------------------------------------------------------------------------

def both_routes(p, x, nu, what):
    """the pass alone, then (fine tuning on) the rotation's pass: each against the model on its own call's outputs"""
    _got, _lev, d = checked(p, lambda: p.work(x), what)
    assert "levels: pass" in d, d
    p.set_fine_tuning(nu)
    _got, _lev, d = checked(p, lambda: p.work(x), what + ", with fine tuning")
    p.set_fine_tuning(None)
    assert FORCED or "levels: with the rotation" in d, d


@pytest.mark.parametrize("R", TINY_R)
def test_the_8_byte_branch_and_tiny_rows(R):
    """16 bytes per lane only where lout is even and the channel's run is 16-byte aligned: odd lout, lout = 1 (a row of one lane, 64 rows per wave), rows of
    2 to 15 samples (several rows per wave) and even lout behind an odd offset"""
    N, nb = 8192, 5
    H = N - N // R
    x = stream(nb * H, 200 + N // 4096 + R)
    p = G.Pipeline(N, R, TINY, windowtype=1, max_blocks=nb)
    off = [p.channel_offset(c, nb) for c in range(len(TINY))]
    assert 1 in p.lout and any(lo % 2 for lo in p.lout) and any(1 < lo <= 32 for lo in p.lout), p.lout
    assert R == 16 or any(lo % 2 == 0 and o % 2 for lo, o in zip(p.lout, off)), (p.lout, off)
    both_routes(p, x, edge_nus(len(TINY), TINY_R.index(R) * 3), "tiny rows R=%d" % R)
    assert FORCED or p.path() == 0


def test_rows_longer_than_a_wave():
    """lout = 6144, 12288 and 24576 (channels above 4096 bins): every lane of a wave takes 48 to 192 sample pairs of a row, four a trip"""
    N, R, nb = 32768, 4, 3
    H = N - N // R
    x = stream(nb * H, 200 + N // 4096 + R)
    p = G.Pipeline(N, R, LONG, windowtype=1, max_blocks=nb)
    assert max(p.lout) == 24576 and min(p.lout) // 2 > 64
    both_routes(p, x, edge_nus(len(LONG), 8), "long rows")


def test_more_blocks_than_one_trip_of_the_grid_stride_loop():
    """launch_chan_levels gives gx = max(1, min(ceil(nb / 4), ceil(2048 / channels))) workgroups of four waves to every channel; a wave takes 64 >> lg rows
    a step and four steps a trip, lg = min(6, ceil(log2(ceil(lout / 2)))): 256 channels of lout = 128 and 140 blocks are more than 128 rows a trip (and
    k_fine_rotate<true> takes one step a trip)"""
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
    both_routes(p, signal(nb * H, 23), edge_nus(nc, 9), "140 blocks of the full bank")
    assert FORCED or p.path() == 3


# ---- 4. with the other settings ------------------------------------------------------------------------------------------------------------------------------

def loud_and_quiet(n, H, seed):
    """blocks 0 and 1 quiet, the rest a thousand times louder"""
    x = signal(n * H, seed)
    x[2 * H:] *= np.float32(1000.0)
    return x


@pytest.mark.parametrize("N,R,chans", [(16384, 2, BANK), (16384, 4, BANK), (4096, 2, EXAMPLE)], ids=["256-bin bank, R = 2", "256-bin bank, R = 4", "path 5"])
def test_integer_output_and_input(N, R, chans):
    """sc16 and sc8 output crossed with float and sc16 input.  The kernels that narrow in their own stores write float while levels are on ("narrowed"), and
    narrow themselves again once levels are off ("fused"); the narrow outputs are byte-equal either way.  The rows with peak * scale >= 32767.5 / 127.5 are
    exactly the rows where the narrow output holds a limit value: blocks 0 and 1 of the input are quiet, the others a thousand times louder."""
    nb = 5
    H = N - N // R
    xf = loud_and_quiet(nb, H, 40)
    xi = iq(nb * H, np.int16, 41)
    xi[:4 * H] //= 1000                                                    # (interleaved: the first two blocks)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb)
    for ifmt, call in (("float", lambda: p.work(xf)), ("sc16", lambda: p.work_iq(xi, scale=2.0 ** -15))):
        p.set_output_format(None)
        yf, lev, d = checked(p, call, "%s in, float out" % ifmt)
        assert FORCED or ifmt == "float" or "input sc16: fused" in d, d
        quiet = float(lev[:2, :, 1].max())
        for ofmt, odt, limit in FORMATS:
            scale = float(np.float32(0.05 * limit / quiet))                # the quiet rows peak at 5 % of the range, the loud ones far above it
            p.set_output_format(ofmt, scale)
            got, lev_i, d, plain = on_and_off(p, call)
            d_off = p.describe()
            same_bytes(lev_i, lev, "%s in, %s out: the levels are those of the float samples" % (ifmt, ofmt))
            info = np.iinfo(odt)
            for c, (u, v, w) in enumerate(zip(got, plain, yf)):
                same_bytes(u, v, "%s in, %s out, levels on against off, ch%d" % (ifmt, ofmt, c))
                same_bytes(u, narrowed(w, scale, odt), "%s in, %s out against the narrowed float samples, ch%d" % (ifmt, ofmt, c))
                at_limit = ((u == info.max) | (u == info.min)).reshape(nb, -1).any(axis=1)
                says = lev_i[:, c, 1] * np.float32(abs(scale)) >= np.float32(limit)
                assert (says == at_limit).all() and says.any() and not says.all(), (ifmt, ofmt, c, says, at_limit)
            assert ("output %s: narrowed" % ofmt) in d and "levels: pass" in d, d
            assert FORCED or ("output %s: fused" % ofmt) in d_off, d_off
    p.set_output_format(None)


@pytest.mark.parametrize("N,chans,route", [(16384, BANK, "with the rotation"), (4096, EXAMPLE, "pass")], ids=["bank", "path 5"])
def test_with_fine_tuning_the_levels_are_of_the_turned_samples(N, chans, route):
    """y' = the samples after fine tuning: off path 5 the rotation's pass sums them, on it k_f4096's FINE form writes them and k_chan_levels follows; with sc16
    output on top the turn and the levels come before the narrowing"""
    R, nb = 2, 5
    H = N - N // R
    x = stream(nb * H, 500 + N // 4096)
    nu = edge_nus(len(chans), 4)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb)
    plain = p.work(x)
    p.set_fine_tuning(nu)
    got, lev, d = checked(p, lambda: p.work(x), "fine tuning on")
    assert any(u.tobytes() != v.tobytes() for u, v in zip(got, plain))
    if not FORCED:
        assert ("levels: " + route) in d and ("fine tuning: " + ("rotated" if route != "pass" else "fused")) in d, d
    scale = int_scale(got, np.int16)
    p.set_output_format("sc16", scale)
    p.set_levels(True)
    p.reset()
    gi = p.work(x)
    same_bytes(p.levels(), lev, "sc16 out: the levels")
    for c, (u, v) in enumerate(zip(gi, got)):
        same_bytes(u, narrowed(v, scale, np.int16), "sc16 out, ch%d" % c)
    d = p.describe()
    assert "output sc16: narrowed" in d and (FORCED or ("levels: " + route) in d), d
