"""GPU tests (-m gpu) of every route of the waterfall rows (csrc/fdc_waterfall.hip, the ROWS epilogue of csrc/fdc_fused4096.hip,
fdc_pipeline_work_waterfall): each kernel form, block length and level edge that tests/test_waterfall_gpu.py launches at one point only or
not at all.

1. every ROWS form of the one-launch kernel: k_f4096<WIDE, TEAMS, true> for <false, 1>, <true, 2> and <false, 2>, every plan of
   test_fused4096_gpu.plans() at R = 2, 4, 8, 16 (plan_fused4096 refuses none of them: every width is a power of two >= 16, so l % R == 0
   for every R here), calls of one block and of five, D = 1 and 2.  NOT covered: k_f4096<true, 1, true>.  A plan with a 512- or 1024-bin
   channel gets one block per workgroup only through the process-wide debug variable FDC_F4_TEAMS, read once in plan_fused4096; reaching it
   would take a process of its own, which this suite does not start for one kernel form.
2. launch groups (chunk_blocks) and host sub-batches (FDC_HOST_SUB) on the one-launch route: the row offset of a launch inside a call
3. the group-sum route (k_wf_from_groups) at r = 1, 2, 4, 16 groups per pixel, the group powers summed by the block kernel's epilogue and by
   k_group_power behind the two-pass transform (describe() names which)
4. the spectrum route (k_wf_from_spectrum) at every N below 16384, the N < 1024 branch included
5. the finish kernel's digitize on the standalone face: exact ties, decreasing and equal levels, special values, NaN containment, the block
   lengths blocklen_ok admits, passes that end inside a row, calls without some of the output buffers

Bounds (none taken from the code under test).  Rows summed from float32 bins: waterfall_model.row_bound(n), (n + 3) 2^-24 relative, n the bins
the device sums in float32 (see its docstring) — against the float64 model on the spectrum the same plan's debug-spectrum call returns.  The
standalone face gets the float32 powers themselves and sums in FP64: face_bound(N), one or two float32 roundings.  Against the oracle's spectrum:
max|got - m| <= 1e-5 m.max(), the suite's secondary check.  Colour index: numpy.digitize of the library's own float32 row everywhere; the
model's index wherever the model's pixel is further than 1e-5 (relative) from an edge, the excluded share capped at 1 % (NEAR_CAP; the CPU
suite checks the model's share of every stream used here).  rgb = table[index].  The same arithmetic in another launch shape: the same bytes.

Under a forced path of the suite (FDC_TEST_FORCE) sections 1 and 2 skip: the one-launch route does not exist there."""
import ctypes as C

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from gr_fdc_amd import waterfall as WF
from test_fused4096_gpu import plans
from test_waterfall_gpu import FORCED, check_rows, spectrum_rows
from waterfall_model import (NEAR_CAP, block_rows, colour_index, decimate, model_edges, noise_levels, noise_stream, power_stream, route_seed,
                             row_bound)

pytestmark = pytest.mark.gpu
LEVELS = (-45.0, -20.0)
ONE_ROUNDING = 2.0 ** -24          # an FP64 sum of float32 terms (error ~1e-16 per term) rounded once to float32: half an ulp, <= 2^-24 relative


def face_bound(N):
    """The standalone face gets the float32 powers themselves.  Both stages sum in FP64, and each hands on float32: the block rows ([blocks][1024]
    float32, the format every route writes) and the finished rows.  N <= 1024: a block-row pixel is one input value, exactly — one rounding.
    N > 1024: two roundings, (1 + 2^-24)^2 - 1."""
    return ONE_ROUNDING if N <= 1024 else 2 * ONE_ROUNDING * (1 + ONE_ROUNDING)


NO_F4 = "the one-launch route does not exist under a forced path"


def cat(parts):
    return WF.Rows(*[np.concatenate([getattr(r, f) for r in parts]) for f in WF.Rows._fields])


def check(got, model_rows, n, levels=LEVELS, loginput=0, scheme=0, what="", bound=None):
    """rows within row_bound(n) of the model, index and rgb by the rules of the module docstring, the share left out under the cap"""
    near = check_rows(got, model_rows, loginput=loginput, levels=levels, scheme=scheme, rel=row_bound(n) if bound is None else bound, what=what)
    print("%s: %d of %d pixels within 1e-5 of an edge" % (what, near, model_rows.size))
    assert near <= NEAR_CAP * model_rows.size, (what, near, model_rows.size)


def same_bytes(a, b, what):
    for f in WF.Rows._fields:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (what, f)


def same_channels(a, b, what):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert u.tobytes() == v.tobytes(), (what, c)


# ---- 1. every ROWS form of the one-launch kernel ---------------------------------------------------------------------------------------
PLANS = plans()
F4_R = (2, 4, 8, 16)


def f4_form(chans, R):
    """what plan_fused4096 makes of the plan (host only): 'one block', 'two blocks, wide' or 'two blocks, narrow'"""
    path, text, _a = G.plan_preview(4096, R, chans)
    assert path == 5, text
    wide = any(l >= 512 for (_f, l, _p, _s) in chans)
    if "one block per workgroup" in text:
        assert not wide, text                                              # <true, 1>: the debug variable only
        return "one block"
    assert "two blocks per workgroup" in text, text
    return "two blocks, wide" if wide else "two blocks, narrow"


@pytest.mark.parametrize("R", F4_R)
@pytest.mark.parametrize("name", list(PLANS))
def test_every_rows_form_of_the_one_launch_kernel(name, R):
    """calls of 1 and 5 blocks (one valid block in a two-block workgroup; an odd count), D = 1 and D = 2 (the second call finishes the group the
    first one left): channels = work() on a twin handle, byte for byte; rows against the two-launch form's spectrum of the same stream"""
    if FORCED:
        pytest.skip(NO_F4)
    N, chans = 4096, PLANS[name]
    H = N - N // R
    x = noise_stream(6 * H, route_seed(N, R, 6))
    calls = [x[:H], x[H:]]
    levels = noise_levels(N)
    p, q = G.Pipeline(N, R, chans, max_blocks=5), G.Pipeline(N, R, chans, max_blocks=5)
    s = G.Pipeline(N, R, chans, max_blocks=5, keep_spectrum=True, flags=G.FDC_PIPE_NO_FUSED)
    assert p.path() == 5 and q.path() == 5, p.describe()
    ref = [q.work(c) for c in calls]
    blocks = spectrum_rows(np.concatenate([s.work(c, want_spectrum=True)[1] for c in calls]), N)
    for D in (1, 2):
        p.reset()
        w = G.Waterfall(N, 1e6, R, D, 0, *levels, D, 0, max_items=5)
        parts = []
        for k, c in enumerate(calls):
            outs, rows = p.work_waterfall(c, w)
            same_channels(outs, ref[k], "%s R=%d D=%d call %d" % (name, R, D, k))
            parts.append(rows)
        assert [r.power.shape[0] for r in parts] == ([1, 5] if D == 1 else [0, 3])
        check(cat(parts), decimate(blocks, D), 4, levels=levels, scheme=D, what="%s R=%d D=%d" % (name, R, D))
    d = p.describe()
    assert "k_f4096 epilogue" in d, d
    form = f4_form(chans, R)
    assert ("one block per workgroup" in d) == (form == "one block"), (form, d)


def test_every_reachable_rows_form_is_among_the_cases():
    """the parametrisation above launches <false, 1, true>, <true, 2, true> and <false, 2, true> (two blocks per workgroup without a 512- or
    1024-bin channel: a plan whose one-block schedule does not fit four waves), at every R"""
    if FORCED:
        pytest.skip(NO_F4)
    for R in F4_R:
        forms = {f4_form(chans, R) for chans in PLANS.values()}
        assert forms == {"one block", "two blocks, wide", "two blocks, narrow"}, (R, forms)


# ---- 2. launch groups and sub-batches on the one-launch route -----------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 4])
def test_row_offset_of_launch_groups_and_sub_batches(R):
    """7 blocks, D = 3: one launch; chunk_blocks = 2 (launches at m0 = 0, 2, 4, 6 of one call); FDC_HOST_SUB = 2 (sub-batches whose first
    block is 0, 2, 4, 6 behind the call's) — the same bytes; then the same stream as calls of 3 + 4 blocks"""
    if FORCED:
        pytest.skip(NO_F4)
    N, nb, D = 4096, 7, 3
    chans = PLANS["narrow channels: 128 and 64 bins beside the example"]
    H = N - N // R
    x = noise_stream(nb * H, route_seed(N, R, nb))
    levels = noise_levels(N)

    def run(cuts, **kw):
        p = G.Pipeline(N, R, chans, max_blocks=nb, **kw)
        assert p.path() == 5, p.describe()
        w = G.Waterfall(N, 1e6, R, D, 0, *levels, 1, 0, max_items=nb)
        outs, parts = [], []
        for a, b in cuts:
            o, r = p.work_waterfall(x[a * H:b * H], w)
            outs.append(o)
            parts.append(r)
        assert "k_f4096 epilogue" in p.describe(), p.describe()
        return [np.concatenate([o[c] for o in outs]) for c in range(len(chans))], cat(parts)

    for cuts in ([(0, 7)], [(0, 3), (3, 7)]):
        one = run(cuts)
        grouped = run(cuts, chunk_blocks=2)
        G.defaults["FDC_HOST_SUB"] = "2"
        sub = run(cuts)
        del G.defaults["FDC_HOST_SUB"]
        for what, other in (("chunk_blocks = 2", grouped), ("FDC_HOST_SUB = 2", sub)):
            same_channels(other[0], one[0], (what, cuts))
            same_bytes(other[1], one[1], (what, cuts))
        if len(cuts) == 1:
            whole = one
            s = G.Pipeline(N, R, chans, max_blocks=nb, keep_spectrum=True, flags=G.FDC_PIPE_NO_FUSED)
            m = decimate(spectrum_rows(s.work(x, want_spectrum=True)[1], N), D)
            assert one[1].power.shape[0] == 2
            check(one[1], m, 4, levels=levels, scheme=1, what="R=%d one launch" % R)
        else:
            same_channels(one[0], whole[0], "calls of 3 + 4")
            same_bytes(one[1], whole[1], "calls of 3 + 4")


# ---- 3. the group-sum route at every r ----------------------------------------------------------------------------------------------------
EPILOGUE, PASS, BOTH = "group powers: block kernel epilogue", "group powers: k_group_power behind the two-pass transform", \
    "group powers: block kernel epilogue and k_group_power"


def mixed_plan(N):
    return [(100, 256, 0.8, 1.0), (N // 4 + 1, 512, 0.7, 0.95), (N // 2, 1024, 0.8, 1.0), (N - 300, 128, 0.8, 1.0)]


GROUP_CASES = [(N, R, nb, {}, 0, EPILOGUE) for N in (16384, 32768) for nb in (3, 9) for R in (2, 4)] + [
    (65536, 2, 3, {}, 0, EPILOGUE),
    (65536, 2, 9, {}, 0, EPILOGUE),
    (65536, 2, 3, {"FDC_BLOCK_MIN_BLOCKS": None}, 0, PASS),               # the default threshold (96): a short call takes the two-pass transform
    (16384, 2, 3, {"FDC_NO_BLOCK": "1"}, 0, PASS),
    (32768, 4, 9, {"FDC_BLOCK_MIN_BLOCKS": None}, 0, PASS),
    (16384, 2, 9, {"FDC_BLOCK_MIN_BLOCKS": "4"}, 4, BOTH),               # launch groups of 4 + 4 + 1: the last one is short; group powers at m0 > 0
    (262144, 2, 2, {}, 0, PASS),                                          # no block forward kernel at this length
]


GROUP_IDS = ["N%d-R%d-nb%d-%s%s" % (c[0], c[1], c[2], {EPILOGUE: "epilogue", PASS: "group_power", BOTH: "both"}[c[5]], "".join("-" + k for k in c[3]))
             for c in GROUP_CASES]


@pytest.mark.parametrize("N,R,nb,defaults,chunk,source", GROUP_CASES, ids=GROUP_IDS)
def test_group_sum_route_at_every_r(oracle, N, R, nb, defaults, chunk, source):
    """r = N / 16384 group powers per pixel, D = 2 (nb = 3 and 9 leave a carry; a second call of the same handle takes it up); rows against the
    model on the same plan's debug-spectrum call (n = 16: a group power is a float32 sum of 16 bins, everything behind it FP64), the channels
    byte for byte those of that call, rows against the oracle's spectrum.  describe() names who summed the group powers."""
    for k, v in defaults.items():
        if v is None:
            G.defaults.pop(k, None)
        else:
            G.defaults[k] = v
    D, chans = 2, mixed_plan(N)
    H = N - N // R
    x = noise_stream(nb * H, route_seed(N, R, nb))
    levels = noise_levels(N)
    p = G.Pipeline(N, R, chans, max_blocks=nb, chunk_blocks=chunk)
    w = G.Waterfall(N, 1e6, R, D, 0, *levels, 2, 0, max_items=nb)
    outs, got = p.work_waterfall(x, w)
    d = p.describe()
    assert "k_wf_from_groups" in d, d
    assert G.defaults.get("FDC_FORCE_GENERIC") or d.endswith(source), d
    t = G.Pipeline(N, R, chans, max_blocks=nb, chunk_blocks=chunk, keep_spectrum=True)
    dbg, spec = t.work(x, want_spectrum=True)
    same_channels(outs, dbg, "N=%d R=%d nb=%d" % (N, R, nb))
    blocks = spectrum_rows(spec, N)
    assert got.power.shape[0] == nb // D
    check(got, decimate(blocks, D), 16, levels=levels, scheme=2, what="N=%d R=%d nb=%d %s" % (N, R, nb, source))
    _r, ospec = oracle.channelizer(N, R, 1, chans, x, want_spectrum=True, nthreads=8)
    m = decimate(spectrum_rows(ospec, N), D)
    assert np.abs(got.power - m).max() <= 1e-5 * m.max()
    if nb % D:
        # the carry: the same samples again, as the stream's next nb blocks, finish the open group first
        outs2, more = p.work_waterfall(x, w)
        dbg2, spec2 = t.work(x, want_spectrum=True)
        same_channels(outs2, dbg2, "N=%d R=%d nb=%d second call" % (N, R, nb))
        both = decimate(np.concatenate([blocks, spectrum_rows(spec2, N)]), D)
        assert more.power.shape[0] == nb - nb // D
        check(more, both[nb // D:], 16, levels=levels, scheme=2, what="N=%d R=%d nb=%d second call" % (N, R, nb))


def test_both_sources_of_the_group_powers_are_among_the_cases():
    for sizes in ((65536,), (16384, 32768)):
        seen = {c[5] for c in GROUP_CASES if c[0] in sizes}
        assert {EPILOGUE, PASS} <= seen, (sizes, seen)
    assert {c[0] // 16384 for c in GROUP_CASES} == {1, 2, 4, 16}


# ---- 4. the spectrum route at every N below 16384 -----------------------------------------------------------------------------------------
SPECTRUM_CASES = [
    (64, [(3, 16, 0.8, 1.0), (40, 16, 0.7, 0.9)], None),                                     # one bin per 16 pixels
    (256, [(10, 64, 0.8, 1.0), (100, 32, 0.7, 0.9), (200, 16, 0.8, 1.0)], None),              # ... per 4
    (512, [(10, 128, 0.8, 1.0), (300, 64, 0.7, 0.9)], None),                                  # ... per 2
    (1024, [(10, 256, 0.8, 1.0), (600, 128, 0.7, 0.9), (900, 64, 0.8, 1.0)], None),           # r = 1
    (2048, [(100, 256, 0.8, 1.0), (1000, 512, 0.7, 0.95)], None),
    (4096, [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0)], "FDC_PIPE_NO_FUSED"),
    (4096, [(100, 2048, 0.8, 1.0), (3000, 256, 0.8, 1.0)], None),                             # a 2048-bin channel: the plan cannot fuse
]


@pytest.mark.parametrize("N,chans,flag", SPECTRUM_CASES, ids=["N%d%s" % (c[0], "-NO_FUSED" if c[2] else "-2048-bin" if c[1][0][1] == 2048 else "") for c in SPECTRUM_CASES])
def test_spectrum_route_at_every_block_length(N, chans, flag):
    """two calls of 5 blocks, D = 2 (the first leaves one block): rows against the model on the handle's own spectrum, n = max(1, N / 1024)
    bins per pixel; N < 1024: pixel p is bin p / (1024 / N)"""
    R, nb, D = 2, 5, 2
    H = N - N // R
    flags = getattr(G, flag) if flag else None
    x = noise_stream(2 * nb * H, route_seed(N, R, 2 * nb))
    levels = noise_levels(N)
    p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    s = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags, keep_spectrum=True)
    w = G.Waterfall(N, 1e6, R, D, 0, *levels, 3, 0, max_items=nb)
    parts, specs = [], []
    for k in range(2):
        outs, rows = p.work_waterfall(x[k * nb * H:(k + 1) * nb * H], w)
        dbg, spec = s.work(x[k * nb * H:(k + 1) * nb * H], want_spectrum=True)
        same_channels(outs, dbg, "N=%d call %d" % (N, k))
        parts.append(rows)
        specs.append(spec)
    assert "k_wf_from_spectrum" in p.describe(), p.describe()
    assert [r.power.shape[0] for r in parts] == [2, 3]
    m = decimate(spectrum_rows(np.concatenate(specs), N), D)
    n = max(1, N // 1024)
    got = cat(parts)
    check(got, m, n, levels=levels, scheme=3, what="N=%d %s" % (N, flag))
    if N < 1024:
        k = 1024 // N                                                       # every bin is k equal pixels, in the order of the bins
        assert np.array_equal(got.power, np.repeat(got.power[:, ::k], k, axis=1))
    if flag:
        # the one-launch form of the same plan sums the same bins in float32: both within row_bound(4) of the exact sums
        f = G.Pipeline(N, R, chans, max_blocks=nb)
        assert FORCED or f.path() == 5
        wf = G.Waterfall(N, 1e6, R, D, 0, *levels, 3, 0, max_items=nb)
        fused = cat([f.work_waterfall(x[k * nb * H:(k + 1) * nb * H], wf)[1] for k in range(2)])
        assert FORCED or "k_f4096 epilogue" in f.describe(), f.describe()
        assert np.all(np.abs(fused.power.astype(np.float64) - got.power) <= 2 * row_bound(n) * m)


# ---- 5. the finish kernel on every branch of the digitize (standalone face) -----------------------------------------------------------------
def digitized(got, values, e, scheme, what):
    """rows = the input values (one term, div = 1: -0 may come back as +0, NaN as NaN), index = numpy.digitize of them, rgb = table[index]"""
    v = np.asarray(values, np.float32).reshape(-1, 1024)
    assert got.power.shape == v.shape, what
    assert np.array_equal(got.power, v, equal_nan=True), what
    assert np.array_equal(got.index, np.digitize(v.astype(np.float64), e)), what
    assert got.index.max() <= 1023, what                                   # 1023 edges: numpy.digitize gives 0 ... 1023, the table has 1024 colours
    assert np.array_equal(got.rgb, WF.color_table(scheme)[0][got.index]), what


def tie_rows():
    """every integer -513 ... 513 and the half-integers between them, filled up to three rows and shuffled"""
    v = np.arange(-513.0, 513.25, 0.5)
    assert v.size == 2053
    v = np.concatenate([v, v[:3 * 1024 - v.size]])
    return np.random.default_rng(3).permutation(v).astype(np.float32).reshape(3, 1024)


def test_values_exactly_on_an_edge_increasing_and_decreasing():
    """loginput = 1, levels (-511, 511): the edges are the integers.  x on edge i counts edge i (<=) where the edges increase and does not (>)
    where they decrease; construction, and a live handle that goes increasing -> decreasing -> increasing"""
    up, down = model_edges(1, -511, 511), model_edges(1, 511, -511)
    assert np.array_equal(up, np.arange(-511.0, 512.0)) and np.array_equal(down, up[::-1])
    v = tie_rows()
    w = G.Waterfall(1024, 1e6, 4, 1, 1, -511, 511, 1, 0, max_items=3)
    first = w.work(v)
    assert first.power.tobytes() == v.tobytes()
    digitized(first, v, up, 1, "increasing")
    digitized(G.Waterfall(1024, 1e6, 4, 1, 1, 511, -511, 2, 0, max_items=3).work(v), v, down, 2, "decreasing at construction")
    w.set_minvaldb(511)                                                     # (511, 511) on the way: equal edges
    digitized(w.work(v), v, model_edges(1, 511, 511), 1, "equal on the way")
    w.set_maxvaldb(-511)
    got = w.work(v)
    assert got.power.tobytes() == v.tobytes()
    digitized(got, v, down, 1, "decreasing on a live handle")
    assert not np.array_equal(got.index, first.index)
    w.set_minvaldb(-511)
    w.set_maxvaldb(511)
    same_bytes(w.work(v), first, "increasing again")


@pytest.mark.parametrize("loginput", [0, 1])
def test_equal_levels(loginput):
    """(-30, -30): numpy takes constant bins as increasing — 0 below the level, 1023 on it and above (and for NaN)"""
    e = model_edges(loginput, -30.0, -30.0)
    assert np.all(e == e[0])
    c = np.float32(e[0])
    around = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf)), c * 2, c / 2, c - 1, c + 1, -30.0, -31.0, -29.0, 0.0, np.nan]
    v = np.resize(np.array(around, np.float32), 1024)
    got = G.Waterfall(1024, 1e6, 4, 1, loginput, -30.0, -30.0, 0, 0).work(v)
    digitized(got, v, e, 0, "equal levels, loginput %d" % loginput)
    assert set(np.unique(got.index)) == {0, 1023}


SPECIAL = [0.0, -0.0, 1e-45, 3.4028234663852886e38, np.inf, -np.inf, np.nan, -1.0, 1e-3, -33.0]


@pytest.mark.parametrize("scheme", [0, 1, 2, 3])
@pytest.mark.parametrize("levels", [(-45.0, -20.0), (-20.0, -45.0)])
@pytest.mark.parametrize("loginput", [0, 1])
def test_special_pixel_values(loginput, levels, scheme):
    """+0, -0, the smallest denormal, FLT_MAX, +-inf, NaN, a negative power: the index stays inside the table, as numpy.digitize counts it"""
    v = np.resize(np.array(SPECIAL, np.float32), 2 * 1024)
    assert v[2] > 0 and v[2] == np.float32(2.0 ** -149)
    got = G.Waterfall(1024, 1e6, 4, 1, loginput, *levels, scheme, 0).work(v)
    digitized(got, v, model_edges(loginput, *levels), scheme, "loginput %d levels %s scheme %d" % (loginput, levels, scheme))


def test_a_nan_stays_in_its_pixel_and_its_row():
    """D = 3, calls of 2 + 2 + 2 blocks, one NaN pixel in block 1: it sits in the carried group of call 1.  Row 0 is NaN there and nowhere else,
    row 1 is finite; after reset() the stream without the NaN gives the model's bytes"""
    N, D, pix = 1024, 3, 777
    clean = power_stream(6, N, seed=21)
    pw = clean.copy()
    pw[1, pix] = np.nan
    m = decimate(block_rows(clean), D)
    w = G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 0, 0)
    parts = [w.work(pw[a:a + 2]) for a in (0, 2, 4)]
    assert [r.power.shape[0] for r in parts] == [0, 1, 1]
    got = cat(parts)
    bad = np.zeros((2, 1024), bool)
    bad[0, pix] = True
    assert np.array_equal(np.isnan(got.power), bad)
    e = model_edges(0, *LEVELS)
    assert got.index[0, pix] == 1023 and np.array_equal(got.index, np.digitize(got.power.astype(np.float64), e))
    assert np.array_equal(got.rgb, WF.color_table(0)[0][got.index])
    ok = ~bad
    assert got.power[ok].tobytes() == m.astype(np.float32)[ok].tobytes()
    w.reset()
    again = cat([w.work(clean[a:a + 2]) for a in (0, 2, 4)])
    assert again.power.tobytes() == m.astype(np.float32).tobytes()
    check(again, m, 1, what="after reset", bound=ONE_ROUNDING)


@pytest.mark.parametrize("N,nitems", [(1, 9), (2, 9), (256, 9), (3072, 9), (1 << 20, 3)])
@pytest.mark.parametrize("D", [1, 4])
def test_block_lengths_the_face_admits(N, nitems, D):
    """kron (N = 1, 2, 256), r = 3 (a multiple of 1024 that is no power of two) and r = 1024; one internal pass per item and one for the call;
    the stream is the items twice, in two calls (D = 4: the second call finishes the group the first one left)"""
    pw = power_stream(nitems, N, seed=N % 1000 + D)
    m = decimate(block_rows(np.concatenate([pw, pw])), D)
    assert m.shape[0] == 2 * nitems // D
    res = []
    for max_items in (1, nitems):
        w = G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 1, 0, max_items=max_items)
        got = cat([w.work(pw), w.work(pw)])
        assert w.rows_done() == m.shape[0]
        check(got, m, 1, scheme=1, what="N=%d D=%d max_items=%d" % (N, D, max_items), bound=face_bound(N))
        res.append(got)
    same_bytes(res[0], res[1], "max_items 1 against %d" % nitems)


def test_rows_that_finish_inside_a_pass():
    """D = 25, passes of 4 items over 60: row 0 ends inside pass 7 (items 24 ... 27), row 1 inside pass 13 (48 ... 51)"""
    N, D, n = 1024, 25, 60
    pw = power_stream(n, N, seed=25)
    w = G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 2, 0, max_items=4)
    got = w.work(pw)
    assert got.power.shape[0] == 2 and w.rows_done() == 2
    check(got, decimate(block_rows(pw), D), 1, scheme=2, what="D=25", bound=ONE_ROUNDING)
    same_bytes(G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 2, 0, max_items=n).work(pw), got, "one pass")


def test_calls_without_some_of_the_buffers():
    """index and rgb but no rows buffer, and rows alone, through the C-ABI: the parts of the full call (the carry moves on either way)"""
    N, D, n = 2048, 3, 8
    pw = power_stream(n, N, seed=8)
    full = G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 3, 0).work(pw)
    assert full.power.shape[0] == 2
    for want in (("index", "rgb"), ("power",)):
        w = G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 3, 0)
        bufs = {"power": np.full((3, 1024), -1.0, np.float32), "index": np.full((3, 1024), 0xFFFF, np.uint16), "rgb": np.full((3, 1024, 3), 7, np.uint8)}
        ptr = {k: (bufs[k].ctypes.data if k in want else None) for k in bufs}
        for off, (a, b) in enumerate(((0, 5), (5, 8))):                       # rows 0 and 1: the second one through the carry
            x = np.ascontiguousarray(pw[a:b])
            got = C.c_int32(-1)
            rc = _lib.lib().fdc_waterfall_work(w._h, x.ctypes.data, b - a,
                                               None if ptr["power"] is None else ptr["power"] + 4 * 1024 * off,
                                               None if ptr["index"] is None else ptr["index"] + 2 * 1024 * off,
                                               None if ptr["rgb"] is None else ptr["rgb"] + 3 * 1024 * off, 3 - off, C.byref(got))
            assert _lib.check(rc) == b - a and got.value == 1
        for k in bufs:
            if k in want:
                assert bufs[k][:2].tobytes() == getattr(full, k).tobytes(), (want, k)
                assert bufs[k][2:].tobytes() == (np.full_like(bufs[k][2:], -1.0 if k == "power" else 0xFFFF if k == "index" else 7)).tobytes()
            else:
                assert np.all(bufs[k] == (-1.0 if k == "power" else 0xFFFF if k == "index" else 7)), (want, k)
