"""GPU tests (-m gpu) of the channel gains on every plan, inside the device code that applies them, and together with the other settings
(tests/test_gains_gpu.py covers the setting itself and the call forms; its helpers are used here).

Three routes apply a gain (csrc/fdc_postpass.hip; chosen per call and launched per launch group by process_device_impl): k_fine_rotate's GAIN forms where
the rotation's pass runs ("gains: with the rotation"), k_chan_gain in place on the float results ("gains: pass"), and k_chan_gain's sc16 / sc8 forms,
which read the float staging and store the narrow samples ("gains: with the narrowing").  Each case here is an index, an offset or a dispatch decision of
one of them.  Every comparison is in bytes against gained() / narrowed(gained()) of the same handle's gains-off float outputs; levels against the model
of tests/test_levels_cpu.py on the gained samples, and byte-equal between the routes that see the same samples."""
import functools

import numpy as np
import pytest

import gr_fdc_amd as G
from test_fine_tuning_gpu import BANK, FORCED, signal
from test_fine_tuning_routes_gpu import ALIAS_N, LONG, TINY, TINY_R, alias_plan, edge_nus, int_scale
from test_fused4096_gpu import EXAMPLE, plans as fused_plans
from test_gains_cpu import draw_gains, gained
from test_gains_gpu import ODT, checked, run, wanted
from test_iq_input_gpu import iq, plans as iq_plans, same_bytes
from test_iq_output_gpu import EXTRA

pytestmark = pytest.mark.gpu
FORMATS = (("sc16", np.int16, 32767.5), ("sc8", np.int8, 127.5))


@functools.lru_cache(maxsize=4)
def stream(n, seed):
    """the input of the cases that share one (read only)"""
    x = signal(n, seed)
    x.setflags(write=False)
    return x


def routes_hold(p, call, g, nu, what, fmt="sc16", modes=(False, True)):
    """The three routes on one handle, with levels off and on (modes): in place and narrowing on the samples as they are cut, then — fine tuning nu on —
    with the rotation, float and narrowed.  The levels of the two routes that see the same samples are byte-equal."""
    for fine in (False, True):
        p.set_fine_tuning(nu if fine else None)
        y, _l, d0 = run(p, call, None)
        assert "gains" not in d0, d0
        scale = int_scale(wanted(y, g), ODT[fmt])
        for levels in modes:
            levs = []
            for f, route in ((None, "pass"), (fmt, "with the narrowing")):
                _y, _got, lev, d = checked(p, call, g, "%s (fine %s, %s, levels %s)" % (what, fine, f, levels), f, scale, levels, y=y)
                levs.append(lev)
                if not FORCED:
                    assert ("gains: " + ("with the rotation" if fine else route)) in d, d
                    assert not levels or ("levels: " + ("with the rotation" if fine else "with the gains")) in d, d
                assert not f or ("output %s: narrowed" % f) in d, d
            if levels:
                same_bytes(levs[1], levs[0], what + ": the levels in front of the narrowing against the float route's")
    p.set_fine_tuning(None)


# ---- 1. path 5 -------------------------------------------------------------------------------------------------------------------------------------------

F4 = list(fused_plans().items())


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("k", range(len(F4)), ids=[name for name, _ in F4])
def test_every_plan_of_the_one_launch_kernel(k, R):
    """The 17 plans of test_fused4096_gpu.py at 1 and 5 blocks: k_f4096 writes float and k_chan_gain follows (float: pass; sc16: with the narrowing); with
    fine tuning k_f4096's FINE form turns the samples in its stores and the pass follows all the same"""
    name, chans = F4[k]
    N = 4096
    H = N - N // R
    x = stream(5 * H, 100 + R)
    g = draw_gains(len(chans), 100 + k)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=5)
    for nb in (1, 5):
        call = lambda: p.work(x[:nb * H])
        what = "%s R=%d nb=%d" % (name, R, nb)
        y, _got, _l, d = checked(p, call, g, what)
        scale = int_scale(wanted(y, g), np.int16)
        _y, _got, _l, di = checked(p, call, g, what + ", sc16", "sc16", scale, levels=True, y=y)
        p.set_fine_tuning(edge_nus(len(chans), k))
        _y, _got, _l, df = checked(p, call, g, what + ", fine tuning", levels=(nb == 5))
        p.set_fine_tuning(None)
        assert "gains: pass" in d and "gains: with the narrowing" in di and "output sc16: narrowed" in di, (d, di)
        if not FORCED:
            assert p.path() == 5 and "fine tuning: fused" in df and "gains: pass" in df, df


@pytest.mark.parametrize("R", [2, 4])
def test_launch_groups_of_path_5(R):
    """chunk_blocks = 2: five blocks are three launches at mbase 0, 2, 4"""
    N, nb = 4096, 5
    H = N - N // R
    chans = fused_plans()["narrow channels: 128 and 64 bins beside the example"]
    x = stream(5 * H, 100 + R)
    g = draw_gains(len(chans), 120)
    res = []
    for chunk in (0, 2):
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, chunk_blocks=chunk)
        assert chunk == 0 or p.chunk_blocks() == 2
        y, got, lev, d = checked(p, lambda: p.work(x), g, "chunk_blocks %d R=%d" % (chunk, R), levels=True)
        scale = int_scale(wanted(y, g), np.int8)
        _y, goti, levi, _d = checked(p, lambda: p.work(x), g, "chunk_blocks %d R=%d, sc8" % (chunk, R), "sc8", scale, levels=True, y=y)
        same_bytes(levi, lev, "sc8: the levels")
        res.append((got, goti, lev))
        assert FORCED or p.path() == 5, d
    for c in range(len(chans)):
        same_bytes(res[1][0][c], res[0][0][c], "chunk_blocks 2 against 0, ch%d" % c)
        same_bytes(res[1][1][c], res[0][1][c], "chunk_blocks 2 against 0, sc8, ch%d" % c)
    same_bytes(res[1][2], res[0][2], "chunk_blocks 2 against 0: the levels")


@pytest.mark.parametrize("fine", [False, True], ids=["as cut", "fine tuning"])
def test_a_spectrum_call_between_plain_calls(fine):
    """keep_spectrum: work, work(want_spectrum=True), work.  The middle call runs the spectrum path — with fine tuning on its rotation pass applies the
    gain — the outer ones the one-launch kernel and the pass; the spectrum is unchanged"""
    N, R, nb = 4096, 4, 3
    H = N - N // R
    x = signal(3 * nb * H, 21)
    g = draw_gains(len(EXAMPLE), 130)
    p = G.Pipeline(N, R, EXAMPLE, windowtype=1, max_blocks=nb, keep_spectrum=True)
    p.set_fine_tuning(edge_nus(len(EXAMPLE), 6) if fine else None)
    routes = []

    def three_calls():
        res = []
        for k in range(3):
            res.append(p.work(x[k * nb * H:(k + 1) * nb * H], want_spectrum=(k == 1)))
            routes.append(p.describe())
        return res

    plain, _l, _d = run(p, three_calls, None)
    del routes[:]
    got, _l, _d = run(p, three_calls, g)
    for k in range(3):
        a, b = (got[k][0], plain[k][0]) if k == 1 else (got[k], plain[k])
        for c, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, gained(v, g[c]), "call %d ch%d" % (k, c))
    same_bytes(got[1][1], plain[1][1], "the spectrum of the middle call")
    assert np.abs(plain[1][1]).max() > 0
    if not FORCED:
        assert "gains: pass" in routes[0] and "gains: pass" in routes[2], routes
        assert ("gains: " + ("with the rotation" if fine else "pass")) in routes[1], routes


# ---- 2. every other path ---------------------------------------------------------------------------------------------------------------------------------

OTHERS = [c for c in iq_plans() if "k_f4096" not in c[0]] + EXTRA


@pytest.mark.parametrize("fine", [False, True], ids=["as cut", "fine tuning"])
@pytest.mark.parametrize("k", range(len(OTHERS)), ids=[c[0] for c in OTHERS])
def test_every_other_route(k, fine):
    """paths 0 and 1, path 2 (two launches), path 3 (k_blk256 on the grid / OFF / HALF / R = 4, k_blk512, k_blk1024, k_blknar), path 4 (a split plan with a
    remainder), and the keep_spectrum handles: float and sc16 output, levels on"""
    name, N, R, chans, flags, _r_in, keep = OTHERS[k]
    H, nb = N - N // R, (3 if N >= 65536 else 5)
    x = stream(nb * H, 200 + N // 4096 + R)
    g = draw_gains(len(chans), 200 + k)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
    p.set_fine_tuning(edge_nus(len(chans), k) if fine else None)
    path = p.path()
    spectra = []

    def call():
        if not keep:
            return p.work(x)
        outs, spec = p.work(x, want_spectrum=True)
        spectra.append(spec)
        return outs

    y, _got, lev, d = checked(p, call, g, name, levels=True)
    scale = int_scale(wanted(y, g), np.int16)
    _y, _got, levi, di = checked(p, call, g, name + ", sc16", "sc16", scale, levels=True, y=y)
    same_bytes(levi, lev, name + ", sc16: the levels")
    for s in spectra[1:]:
        same_bytes(s, spectra[0], name + ": the spectrum")
    assert p.path() == path and "output sc16: narrowed" in di, (name, di)
    if not FORCED:
        assert ("gains: " + ("with the rotation" if fine else "pass")) in d, d
        assert ("gains: " + ("with the rotation" if fine else "with the narrowing")) in di, di


def test_copies_of_channels_with_the_same_slice():
    """bank_alias: a channel with an earlier channel's slice is a device-to-device copy of that channel's rows, made BEFORE the pass: a channel and its
    copy carry different gains"""
    N, R, nb = ALIAS_N, 2, 5
    H = N - N // R
    plan = alias_plan(N)
    first = len(set(plan))
    x = stream(nb * H, 200 + N // 4096 + R)
    g = draw_gains(len(plan), 300)
    assert all(g[c] != g[c - first] for c in range(first, len(plan)))
    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
    routes_hold(p, lambda: p.work(x), g, edge_nus(len(plan), 5), "slots twice", modes=(True,))
    if not FORCED:
        assert p.path() == 3 and "copies of channels with the same slice" in p.describe(), p.describe()


@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["float", "sc16"])
def test_short_groups_under_the_default_dispatch(fmt):
    """Without FDC_BLOCK_MIN_BLOCKS (conftest.py sets 1) a launch group of fewer than 96 blocks takes the two-launch form: 100 blocks in groups of 96 run
    96 on the block kernel and 4 on stage 1 + stage 2, gained with mbase = 96"""
    N, R, nb = 16384, 2, 100
    H = N - N // R
    x = signal(nb * H, 22)
    g = draw_gains(len(BANK), 310)
    saved = G.defaults.pop("FDC_BLOCK_MIN_BLOCKS", None)
    try:
        p = G.Pipeline(N, R, BANK, windowtype=1, max_blocks=nb, chunk_blocks=96)
    finally:
        if saved is not None:
            G.defaults["FDC_BLOCK_MIN_BLOCKS"] = saved
    assert p.chunk_blocks() == 96
    y, _l, _d = run(p, lambda: p.work(x), None)
    scale = int_scale(wanted(y, g), np.int16) if fmt else 1.0
    _y, _got, _lev, d = checked(p, lambda: p.work(x), g, "96 + 4 blocks", fmt, scale, levels=True, y=y)
    assert FORCED or p.path() == 3, d
    assert ("gains: " + ("with the narrowing" if fmt else "pass")) in d, d


# ---- 3. inside k_chan_gain and k_fine_rotate's GAIN forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["sc16", "sc8"])
@pytest.mark.parametrize("R", TINY_R)
def test_the_8_byte_branch_and_tiny_rows(R, fmt):
    """16 bytes per lane only where lout is even and the channel's run is 16-byte aligned: odd lout, lout = 1 (a row of one lane, 64 rows per wave), rows of
    2 to 15 samples (several rows per wave) and even lout behind an odd offset (8-byte loads, and narrow stores one sample at a time: the run of such a
    channel in the narrow output is not aligned for a pair)"""
    N, nb = 8192, 5
    H = N - N // R
    x = stream(nb * H, 200 + N // 4096 + R)
    g = draw_gains(len(TINY), 320 + R)
    p = G.Pipeline(N, R, TINY, windowtype=1, max_blocks=nb)
    off = [p.channel_offset(c, nb) for c in range(len(TINY))]
    assert 1 in p.lout and any(lo % 2 for lo in p.lout) and any(1 < lo <= 32 for lo in p.lout), p.lout
    assert R == 16 or any(lo % 2 == 0 and o % 2 for lo, o in zip(p.lout, off)), (p.lout, off)
    routes_hold(p, lambda: p.work(x), g, edge_nus(len(TINY), TINY_R.index(R) * 3), "tiny rows R=%d" % R, fmt)
    assert FORCED or p.path() == 0


def test_rows_longer_than_a_wave():
    """lout = 6144, 12288 and 24576 (channels above 4096 bins): every lane of a wave takes 48 to 192 sample pairs of a row, four a trip"""
    N, R, nb = 32768, 4, 3
    H = N - N // R
    x = stream(nb * H, 200 + N // 4096 + R)
    g = np.array([-2.7, 0.011, 93.0], np.float32)
    p = G.Pipeline(N, R, LONG, windowtype=1, max_blocks=nb)
    assert max(p.lout) == 24576 and min(p.lout) // 2 > 64
    routes_hold(p, lambda: p.work(x), g, edge_nus(len(LONG), 8), "long rows")


def test_more_blocks_than_one_trip_of_the_grid_stride_loop():
    """launch_chan_gain gives gx = max(1, min(ceil(nb / 4), ceil(2048 / channels))) workgroups of four waves to every channel; a wave takes 64 >> lg rows
    a step and four steps a trip, lg = min(6, ceil(log2(ceil(lout / 2)))): 256 channels of lout = 128 and 140 blocks are more than 128 rows a trip (and
    k_fine_rotate's forms take one step a trip)"""
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
    routes_hold(p, lambda: p.work(x), draw_gains(nc, 330), edge_nus(nc, 9), "140 blocks of the full bank")
    assert FORCED or p.path() == 3


# ---- 4. with integer input and output: the AGC loop in one step ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ifmt", ["sc16", "sc8"])
@pytest.mark.parametrize("N,R,chans", [(16384, 2, BANK), (16384, 4, BANK), (4096, 2, EXAMPLE)], ids=["256-bin bank, R = 2", "256-bin bank, R = 4", "path 5"])
def test_integer_input_and_output(N, R, chans, ifmt):
    """sc16 / sc8 input crossed with sc16 / sc8 output.  First call: drawn gains over a spread of 2^16, rows that saturate and rows that do not; the rows
    with peak * scale >= 32767.5 / 127.5 (the gained levels) are exactly the rows where the narrow output holds a limit value.  Second call: per-channel
    gains from the first call's levels put every channel's peak at half the range — no row at a limit value, every channel's peak above a quarter."""
    nb = 5
    H = N - N // R
    idt = ODT[ifmt]
    xi = iq(nb * H, idt, 41)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb)
    call = lambda: p.work_iq(xi, scale=1.0 / (np.iinfo(idt).max + 1))
    g = draw_gains(len(chans), 400 + N // 4096 + R)
    y, _got, lev0, d = checked(p, call, g, "%s in, float out" % ifmt, levels=True)
    assert FORCED or ("input %s: " % ifmt) in d, d
    top = np.abs(np.concatenate([v.view(np.float32) for v in y])).max()
    for ofmt, odt, limit in FORMATS:
        info = np.iinfo(odt)
        scale = float(np.float32(0.5 * limit / top))                         # gains off every row is inside the range; the gains push some out
        _y, got, lev, d = checked(p, call, g, "%s in, %s out" % (ifmt, ofmt), ofmt, scale, levels=True, y=y)
        same_bytes(lev, lev0, "%s in, %s out: the levels are those of the gained float samples" % (ifmt, ofmt))
        says = lev[:, :, 1] * np.float32(abs(scale)) >= np.float32(limit)
        at_limit = np.array([((u == info.max) | (u == info.min)).reshape(nb, -1).any(axis=1) for u in got]).T
        assert (says == at_limit).all() and says.any() and not says.all(), (ifmt, ofmt, says.sum(), at_limit.sum())
        assert "gains: with the narrowing" in d and ("output %s: narrowed" % ofmt) in d, d
        # the AGC step: the gains-off levels of one call give the gains of the next (the same input: the same peaks)
        _yy, l_off, _d = run(p, call, None, levels=True)
        peak = l_off[:, :, 1].max(axis=0)
        agc = (np.float32(0.5 * limit) / (peak * np.float32(scale))).astype(np.float32)
        _y, got2, lev2, _d = checked(p, call, agc, "%s in, %s out, gains from the levels" % (ifmt, ofmt), ofmt, scale, levels=True, y=y)
        for c, u in enumerate(got2):
            assert not ((u == info.max) | (u == info.min)).any(), (ifmt, ofmt, c)
            assert np.abs(u.astype(np.int32)).max() > 0.25 * limit, (ifmt, ofmt, c, int(np.abs(u.astype(np.int32)).max()))
        assert (lev2[:, :, 1] * np.float32(scale) < np.float32(limit)).all()
