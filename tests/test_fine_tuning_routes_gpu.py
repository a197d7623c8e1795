"""GPU tests (-m gpu) of fine tuning on every route, channel width, overlap and call form (tests/test_fine_tuning_gpu.py covers the setting itself).

Two pieces of device code turn the samples: the FINE forms of the one-launch kernel on path 5 (k_f4096_fine, csrc/fdc_fused4096_body.inc: every row class has
its own fine_row call and store indices), and k_fine_rotate behind the channel kernels of every other plan (csrc/fdc_postpass.hip, launched per launch group by
process_device_impl).  Each case here is an index, an offset or a dispatch decision of one of them.

The model and its bound are test_fine_tuning_gpu.py's (holds(), phasors(); DESIGN.md "Fine tuning"): the float64 phasor of the 64-bit wrapping phase applied
to THE SAME handle's output on the same input with fine tuning off, |y' - y w| <= 20 * 2^-24 |y| + 2^-40 max|y| per sample.  Integer outputs are compared byte
for byte with narrowed(the same handle's float y').  Every case takes its frequencies from one set of edge values (EDGES), the rest seeded draws;
test_every_edge_frequency_is_used_on_both_routes checks that each value is launched on both routes."""
import ctypes as C
import functools

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
from test_fine_tuning_gpu import BANK, FORCED, MIXED, holds, narrowed, signal, work_span
from test_fused4096_gpu import EXAMPLE, plans as fused_plans
from test_iq_input_gpu import iq, plans as iq_plans, same_bytes
from test_iq_output_gpu import EXTRA

pytestmark = pytest.mark.gpu

NEAR_HALF = 0.5 - 2.0 ** -40
# +-(0.5 - 2^-40); +-2^-64: inc = 1 and 2^64 - 1; +-0.25; +-0.125: exactly on fine_phasor's quarter-turn boundary; 2^-30; 0
EDGES = [NEAR_HALF, -NEAR_HALF, 2.0 ** -64, -2.0 ** -64, 0.25, -0.25, 0.125, -0.125, 2.0 ** -30, 0.0]
FORMATS = (("sc16", np.int16), ("sc8", np.int8))


def edge_nus(nchan, k):
    """one frequency per channel: EDGES from its k-th value on (cyclically), as many as there are channels, the rest uniform draws seeded by k"""
    nu = np.random.default_rng(1000 + k).uniform(-0.5, 0.5, nchan)
    n = min(nchan, len(EDGES))
    nu[:n] = [EDGES[(k + i) % len(EDGES)] for i in range(n)]
    if not nu.any():                                       # (a one-channel plan on the value 0: all zeros would switch fine tuning off)
        nu[0] = EDGES[(k + 1) % len(EDGES)]
    return nu


@functools.lru_cache(maxsize=4)
def stream(n, seed):
    """the input of the cases that share one (read only)"""
    x = signal(n, seed)
    x.setflags(write=False)
    return x


def on_and_off(p, nu, call):
    """call() from block 0 of handle p with fine tuning on, describe() behind it, and call() again with it off"""
    p.reset()
    p.set_fine_tuning(nu)
    got = call()
    d = p.describe()
    p.set_fine_tuning(None)
    p.reset()
    plain = call()
    assert "fine tuning: " in d and "fine tuning" not in p.describe(), (d, p.describe())
    return got, d, plain


def all_hold(got, plain, nu, lout, first_block, what):
    assert len(got) == len(plain) == len(nu) == len(lout), what
    for c, (u, v) in enumerate(zip(got, plain)):
        holds(u, v, nu[c], lout[c], first_block, "%s ch%d (nu %r)" % (what, c, nu[c]))


def int_scale(ys, dtype):
    """an output scale that puts the largest component of the float outputs ys at about 60 % of dtype's range (a float32 value)"""
    top = max(float(np.abs(np.ascontiguousarray(y).view(np.float32)).max()) for y in ys)
    assert top > 0
    return float(np.float32(0.6 * np.iinfo(dtype).max / top))


def by_channel(p, flat, nb):
    """the channel-major device layout of one call of nb blocks, cut into its channels"""
    return [flat[p.channel_offset(c, nb):p.channel_offset(c, nb) + nb * lo] for c, lo in enumerate(p.lout)]


# ---- 1. every FINE row class of path 5 ------------------------------------------------------------------------------------------------------------------

F4 = list(fused_plans().items())
F4_R = (2, 4, 8, 16)
TWICE = "the same slice twice and overlapping slices"
NARROW = "narrow channels: 128 and 64 bins beside the example"


def fused_nus(k, R):
    return edge_nus(len(F4[k][1]), 3 * k + F4_R.index(R))


@pytest.mark.parametrize("R", F4_R)
@pytest.mark.parametrize("k", range(len(F4)), ids=[name for name, _ in F4])
def test_every_row_class_of_the_fused_route(k, R):
    """All 17 plans of test_fused4096_gpu.py (row classes 1 to 8, two waves on a row, both workgroup forms) at every overlap: lout = l - l / R moves where a
    row's step factors start.  nb = 1: one valid block in a two-block workgroup; nb = 5: an odd count."""
    name, chans = F4[k]
    N = 4096
    H = N - N // R
    x = stream(5 * H, 100 + R)
    nu = fused_nus(k, R)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=5)
    for nb in (1, 5):
        got, d, plain = on_and_off(p, nu, lambda: p.work(x[:nb * H]))
        all_hold(got, plain, nu, p.lout, 0, "%s R=%d nb=%d" % (name, R, nb))
        if not FORCED:
            assert "fine tuning: fused" in d and p.path() == 5, (name, p.path(), d)
        if name == TWICE:
            # channels 0 and 1 are one slice: the same samples without fine tuning, each turned by its own frequency with it
            assert nu[0] != nu[1]
            same_bytes(plain[0], plain[1], "the same slice twice, fine tuning off")
            assert got[0].tobytes() != got[1].tobytes()


@pytest.mark.parametrize("R", [2, 4])
def test_launch_groups_of_the_fused_route(R):
    """chunk_blocks = 2: five blocks are three launches at mbase 0, 2, 4 (block0 = first_block + mbase), byte-equal to one launch"""
    N, nb = 4096, 5
    H = N - N // R
    chans = fused_plans()[NARROW]
    x = stream(5 * H, 100 + R)
    nu = edge_nus(len(chans), 4)
    outs = []
    for chunk in (0, 2):
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, chunk_blocks=chunk)
        assert chunk == 0 or p.chunk_blocks() == 2
        got, d, plain = on_and_off(p, nu, lambda: p.work(x))
        all_hold(got, plain, nu, p.lout, 0, "chunk_blocks %d R=%d" % (chunk, R))
        assert FORCED or ("fine tuning: fused" in d and p.path() == 5), d
        outs.append(got)
    for c, (u, v) in enumerate(zip(*outs)):
        same_bytes(v, u, "chunk_blocks 2 against 0, ch%d" % c)


def test_a_spectrum_call_between_fused_calls():
    """keep_spectrum: work, work(want_spectrum=True), work.  The middle call runs the spectrum path and k_fine_rotate, the outer ones the one-launch kernel;
    every call holds the model at its own global block index, and the spectrum is what the handle returns with fine tuning off."""
    N, R, nb = 4096, 4, 3
    H = N - N // R
    x = signal(3 * nb * H, 21)
    nu = edge_nus(len(EXAMPLE), 6)
    p = G.Pipeline(N, R, EXAMPLE, windowtype=1, max_blocks=nb, keep_spectrum=True)
    routes = []

    def three_calls():
        res = []
        for k in range(3):
            r = p.work(x[k * nb * H:(k + 1) * nb * H], want_spectrum=(k == 1))
            res.append(r)
            routes.append(p.describe())
        return res

    got, _d, plain = on_and_off(p, nu, three_calls)
    for k in range(3):
        a, b = (got[k][0], plain[k][0]) if k == 1 else (got[k], plain[k])
        all_hold(a, b, nu, p.lout, k * nb, "call %d of three" % k)
    same_bytes(got[1][1], plain[1][1], "the spectrum of the middle call")
    assert np.abs(plain[1][1]).max() > 0
    if not FORCED:
        assert p.path() == 5
        assert ["fine tuning: fused" in d for d in routes[:3]] == [True, False, True], routes[:3]
        assert "fine tuning: rotated" in routes[1], routes[1]


# ---- 2. k_fine_rotate behind every other route -----------------------------------------------------------------------------------------------------------

ROTATED = [c for c in iq_plans() if "k_f4096" not in c[0]] + EXTRA
# fdc_pipeline_path() of those plans where it is not 3 (a bank on its block kernel): what the setting must not change
PATHS = {"example plan under FDC_PIPE_NO_FUSED": 0, "mixed plan (path 1)": 1, "mixed plan, generic kernels (path 0)": 0, "256-bin channels at N = 262144 (path 2)": 2,
         "split plan (path 4)": 4, "keep_spectrum, example plan": 5}


def rotated_nus(k):
    return edge_nus(len(ROTATED[k][3]), 2 * k + 1)


@pytest.mark.parametrize("k", range(len(ROTATED)), ids=[c[0] for c in ROTATED])
def test_rotation_behind_every_other_route(k):
    name, N, R, chans, flags, _r_in, keep = ROTATED[k]
    H, nb = N - N // R, (3 if N >= 65536 else 5)
    x = stream(nb * H, 200 + N // 4096 + R)
    nu = rotated_nus(k)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb, flags=flags, keep_spectrum=keep)
    path = p.path()
    got, d, plain = on_and_off(p, nu, lambda: p.work(x, want_spectrum=keep))
    if keep:
        (got, sa), (plain, sb) = got, plain
        same_bytes(sa, sb, "%s: the spectrum does not turn" % name)
        assert np.abs(sb).max() > 0
    all_hold(got, plain, nu, p.lout, 0, name)
    assert p.path() == path, name
    if not FORCED:
        assert "fine tuning: rotated" in d, (name, d)
        assert path == PATHS.get(name, 3), (name, path, d)


def alias_plan(N):
    """test_parity_gpu's "slots twice": most slots of the 256-bin grid, and the first three quarters of them a second time (copies: bank_alias)"""
    n1 = N // 256
    s0 = [int(v) for v in np.random.default_rng(5).permutation(n1 - 1)[:(4 * n1) // 5]]
    return [(256 * c, 256, 0.88, 1.0) for c in s0] + [(256 * c, 256, 0.88, 1.0) for c in s0[:(3 * len(s0)) // 4]]


ALIAS_N = 16384


def test_copies_of_channels_with_the_same_slice():
    """bank_alias: a channel with an earlier channel's slice is a device-to-device copy of that channel's rows, made BEFORE the rotation; the two carry
    different frequencies.  N = 16384 is the smallest block length of the one-kernel path."""
    N, R, nb = ALIAS_N, 2, 5
    H = N - N // R
    plan = alias_plan(N)
    first = len(set(plan))
    x = stream(nb * H, 200 + N // 4096 + R)
    nu = edge_nus(len(plan), 5)                            # (a copy never has its source's frequency: asserted below)
    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
    got, d, plain = on_and_off(p, nu, lambda: p.work(x))
    all_hold(got, plain, nu, p.lout, 0, "slots twice")
    for c in range(first, len(plan)):
        same_bytes(plain[c], plain[c - first], "ch%d is a copy of ch%d" % (c, c - first))
        assert nu[c] != nu[c - first] and got[c].tobytes() != got[c - first].tobytes(), c
    if not FORCED:
        assert p.path() == 3 and "copies of channels with the same slice" in d and "fine tuning: rotated" in d, d


def test_short_groups_under_the_default_dispatch():
    """Without FDC_BLOCK_MIN_BLOCKS (conftest.py sets 1) a launch group of fewer than 96 blocks takes the two-launch form: 100 blocks in groups of 96 run
    96 on the block kernel and 4 on stage 1 + stage 2, rotated with mbase = 96.  The same with sc16 output (float, rotate, narrow: one layout per call)."""
    N, R, nb = 16384, 2, 100
    H = N - N // R
    x = signal(nb * H, 22)
    nu = edge_nus(len(BANK), 7)
    saved = G.defaults.pop("FDC_BLOCK_MIN_BLOCKS", None)
    try:
        p = G.Pipeline(N, R, BANK, windowtype=1, max_blocks=nb, chunk_blocks=96)
    finally:
        if saved is not None:
            G.defaults["FDC_BLOCK_MIN_BLOCKS"] = saved
    assert p.chunk_blocks() == 96
    got, d, plain = on_and_off(p, nu, lambda: p.work(x))
    all_hold(got, plain, nu, p.lout, 0, "96 + 4 blocks")
    if not FORCED:
        assert p.path() == 3 and "fine tuning: rotated" in d, d
    scale = int_scale(got, np.int16)
    p.set_fine_tuning(nu)
    p.set_output_format("sc16", scale)
    p.reset()
    gi = p.work(x)
    d = p.describe()
    for c, (u, v) in enumerate(zip(gi, got)):
        same_bytes(u, narrowed(v, scale, np.int16), "96 + 4 blocks, sc16 out, ch%d" % c)
    if not FORCED:
        assert "fine tuning: rotated" in d and "output sc16: narrowed" in d, d


TINY = [(0, 1, .5, 1.), (3, 16, .8, 1.), (100, 8, .7, .9), (200, 256, .8, 1.), (500, 2, 1., 1.), (4000, 1024, .8, 1.)]
TINY_R = (4, 8, 16)


@pytest.mark.parametrize("R", TINY_R)
def test_the_8_byte_branch_and_tiny_rows(R):
    """k_fine_rotate reads and writes 16 bytes per lane only where lout is even and the channel's run is 16-byte aligned: odd lout, lout = 1 (64 rows per
    wave) and even lout behind an odd offset take 8 bytes per lane"""
    N, nb = 8192, 5
    H = N - N // R
    x = stream(nb * H, 200 + N // 4096 + R)
    nu = edge_nus(len(TINY), TINY_R.index(R) * 3)
    p = G.Pipeline(N, R, TINY, windowtype=1, max_blocks=nb)
    off = [p.channel_offset(c, nb) for c in range(len(TINY))]
    # (what keeps the case on the 8-byte branch if the plan is ever edited)
    assert 1 in p.lout and any(lo % 2 for lo in p.lout), p.lout
    # (R = 16: lout = 1, 15, 8, 240, 2, 960, and 1 + 15 is even: every even row of that plan starts at an even offset, whatever the block count)
    assert R == 16 or any(lo % 2 == 0 and o % 2 for lo, o in zip(p.lout, off)), (p.lout, off)
    got, d, plain = on_and_off(p, nu, lambda: p.work(x))
    all_hold(got, plain, nu, p.lout, 0, "tiny rows R=%d" % R)
    if not FORCED:
        assert p.path() == 0 and "fine tuning: rotated" in d, (p.path(), d)


LONG = [(100, 8192, .8, 1.), (16001, 16384, .8, 1.), (0, 32768, .8, 1.)]


def test_rows_longer_than_a_wave():
    """lout = 6144, 12288 and 24576: every lane of a wave makes 48 to 192 accesses of 16 bytes per row (channels above 4096 bins)"""
    N, R, nb = 32768, 4, 3
    H = N - N // R
    x = stream(nb * H, 200 + N // 4096 + R)
    nu = edge_nus(len(LONG), 8)
    p = G.Pipeline(N, R, LONG, windowtype=1, max_blocks=nb)
    assert min(p.lout) // 2 > 64
    got, d, plain = on_and_off(p, nu, lambda: p.work(x))
    all_hold(got, plain, nu, p.lout, 0, "long rows")
    assert FORCED or "fine tuning: rotated" in d, d


def test_a_second_trip_of_the_grid_stride_loop():
    """launch_fine_rotate gives gx = max(1, min(ceil(nb / 4), ceil(2048 / channels))) workgroups of four waves to every channel; a wave takes 64 >> lg rows a
    trip, lg = min(6, ceil(log2(accesses per row))): 256 channels of lout = 128 and 40 blocks are 32 rows a trip"""
    N, R, nb = 65536, 2, 40
    H = N - N // R
    chans = [(256 * c, 256, 0.88, 1.0) for c in range(256)]
    nu = edge_nus(len(chans), 9)
    p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=nb)
    nc = len(chans)
    gx = max(1, min((nb + 3) // 4, (2048 + nc - 1) // nc))
    nwaves = 4 * gx
    for lo in set(p.lout):
        for per in (lo, lo // 2):                          # 8 and 16 bytes per lane
            lg = min(6, 0 if per <= 1 else (per - 1).bit_length())
            rows = 64 >> lg
            assert nb > nwaves * rows, (gx, rows, nwaves)
    x = signal(nb * H, 23)
    got, d, plain = on_and_off(p, nu, lambda: p.work(x))
    all_hold(got, plain, nu, p.lout, 0, "40 blocks of the full bank")
    if not FORCED:
        assert p.path() == 3 and "fine tuning: rotated" in d, d


# ---- 3. call forms on the rotated route ----------------------------------------------------------------------------------------------------------------

FORMS = [("mixed, N = 8192", 8192, MIXED), ("bank, N = 16384", 16384, BANK)]
form_ids = [f[0] for f in FORMS]


def form_nus(k):
    return edge_nus(len(FORMS[k][2]), 5 * k + 2)


@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["float", "sc16"])
@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("sub", [0, 2], ids=["one sub-batch", "sub-batches of 2"])
@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_sub_batches_registered_outputs_and_ragged_calls(k, sub, registered, fmt):
    """test_iq_output_gpu.py's test_host_fed_branches_and_ragged_calls with fine tuning on: calls of 1, 7, 3 and 5 blocks (host sub-batches; pageable outputs
    or registered ones through k_scatter_out / k_scatter_oq) are byte-equal to one call of 16 blocks on a second handle, which holds the model"""
    _name, N, chans = FORMS[k]
    R, mb, sizes = 2, 7, (1, 7, 3, 5)
    H = N - N // R
    x = stream(sum(sizes) * H, 300 + k)
    nu = form_nus(k)
    one = G.Pipeline(N, R, chans, max_blocks=sum(sizes))
    yf, d, plain = on_and_off(one, nu, lambda: one.work(x))
    all_hold(yf, plain, nu, one.lout, 0, "one call of 16 blocks")
    assert FORCED or "fine tuning: rotated" in d, d
    dt = np.int16 if fmt else np.complex64
    scale = int_scale(yf, np.int16) if fmt else 1.0
    p = G.Pipeline(N, R, chans, max_blocks=mb, host_sub_blocks=sub or None)
    p.set_fine_tuning(nu)
    if fmt:
        p.set_output_format(fmt, scale)
    bufs = [np.zeros((mb * lo, 2) if fmt else mb * lo, dt) for lo in p.lout]
    if registered:
        for b in bufs:
            G.register_host(b)
    try:
        pieces, b0 = [[] for _ in chans], 0
        for n in sizes:
            outs = [b[:n * lo] for b, lo in zip(bufs, p.lout)]
            p.work(x[b0 * H:(b0 + n) * H], outs=outs)
            for c, o in enumerate(outs):
                pieces[c].append(o.copy())
            b0 += n
    finally:
        if registered:
            for b in bufs:
                G.unregister_host(b)
    for c in range(len(chans)):
        want = narrowed(yf[c], scale, np.int16) if fmt else yf[c]
        same_bytes(np.concatenate(pieces[c]), want, "ragged stream ch%d" % c)
    assert FORCED or "fine tuning: rotated" in p.describe(), p.describe()


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_real_input(k):
    _name, N, chans = FORMS[k]
    R, nb = 2, 5
    H = N - N // R
    xr = stream(nb * H, 300 + k).real[:nb * H].copy()
    nu = form_nus(k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    got, d, plain = on_and_off(p, nu, lambda: p.work_real(xr))
    all_hold(got, plain, nu, p.lout, 0, "work_real")
    assert FORCED or "fine tuning: rotated" in d, d


class DeviceBuffers:
    """hipMalloc'd buffers of one test, freed on exit"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.all = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.all:
            self.hip.hipFree(d)

    def put(self, a):
        d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d), C.c_size_t(max(1, a.nbytes))) == 0
        self.all.append(d)
        assert self.hip.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return d

    def get(self, d, n, dtype):
        a = np.empty(n, dtype)
        assert self.hip.hipMemcpy(C.c_void_p(a.ctypes.data), d, C.c_size_t(a.nbytes), 2) == 0
        return a


@pytest.mark.parametrize("k", range(len(FORMS)), ids=form_ids)
def test_device_entries_at_a_first_block(k):
    """process_device (and process_device_iq on the bank) at first_block = 13: the phase of block 13 of the stream, whatever the handle's own counter"""
    _name, N, chans = FORMS[k]
    R, nb, first = 2, 4, 13
    H, ovl = N - N // R, N // R
    nu = form_nus(k)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    n_out = p.output_samples(nb)
    ring_f = np.ascontiguousarray(stream(sum((1, 7, 3, 5)) * H, 300 + k)[:ovl + nb * H])
    ring_i = iq(ovl + nb * H, np.int16, 31)
    with DeviceBuffers() as dev:
        d_f, d_i, d_o = dev.put(ring_f), dev.put(ring_i), dev.put(np.zeros(n_out, np.complex64))

        def run(call):
            call()
            p.synchronize()
            return by_channel(p, dev.get(d_o, n_out, np.complex64), nb)

        entries = [("process_device", lambda: p.process_device(d_f, first, nb, d_o))]
        if chans is BANK:
            entries.append(("process_device_iq", lambda: p.process_device_iq("sc16", 2.0 ** -12, d_i, first, nb, d_o)))
        for what, call in entries:
            got, d, plain = on_and_off(p, nu, lambda: run(call))
            all_hold(got, plain, nu, p.lout, first, "%s at block %d" % (what, first))
            assert FORCED or "fine tuning: rotated" in d, d


def test_group_of_two_virtual_members_on_the_rotated_route():
    N, R, nb = 16384, 2, 8
    H = N - N // R
    x = stream(sum((1, 7, 3, 5)) * H, 301)
    nu = form_nus(1)
    g = G.PipelineGroup(N, R, BANK, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    p = G.Pipeline(N, R, BANK, max_blocks=nb)
    g.set_fine_tuning(nu)
    p.set_fine_tuning(nu)
    for k in range(2):
        a, b = g.work(x[k * nb * H:(k + 1) * nb * H]), p.work(x[k * nb * H:(k + 1) * nb * H])
        for c, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, "call %d ch%d" % (k, c))
        assert sum(n > 0 for _f, n in g.last_spans()) == 2
    buf = C.create_string_buffer(512)
    _lib.lib().fdc_pipeline_describe(_lib.lib().fdc_pipeline_group_member(g._h, 1), buf, 512)
    if not FORCED:
        assert "fine tuning: rotated" in buf.value.decode() and "fine tuning: rotated" in p.describe(), (buf.value.decode(), p.describe())
    # (the one handle's own samples against the model: the second call starts at block nb)
    p.set_fine_tuning(None)
    p.reset()
    plain = [p.work(x[k * nb * H:(k + 1) * nb * H]) for k in range(2)]
    all_hold(b, plain[1], nu, p.lout, nb, "the second call")


# ---- 4. integer formats on a bank ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [2, 4])
def test_integer_input_and_output_on_a_bank(R):
    """A bank of 256-bin channels reads sc16 / sc8 in its own loads and, without fine tuning, narrows in its own stores.  With it the kernel stores float,
    k_fine_rotate turns, k_complex_to_iq narrows (the fine_on line of oq_fused): bytes equal to narrowed(the handle's float y')."""
    N, nb = 16384, 5
    H = N - N // R
    nu = edge_nus(len(BANK), 10 + R)
    p = G.Pipeline(N, R, BANK, windowtype=1, max_blocks=nb)
    for ifmt, idt in FORMATS:
        xi = iq(nb * H, idt, 40)
        sc_in = 2.0 ** -15 if idt is np.int16 else 2.0 ** -7
        p.set_output_format(None)
        yf, d, plain = on_and_off(p, nu, lambda: p.work_iq(xi, scale=sc_in))
        all_hold(yf, plain, nu, p.lout, 0, "%s in, float out, R=%d" % (ifmt, R))
        if not FORCED:
            assert ("input %s: fused" % ifmt) in d and "fine tuning: rotated" in d, d
        for ofmt, odt in FORMATS:
            scale = int_scale(yf, odt)
            p.set_output_format(ofmt, scale)
            p.set_fine_tuning(nu)
            p.reset()
            got = p.work_iq(xi, scale=sc_in)
            d = p.describe()
            for c, (u, v) in enumerate(zip(got, yf)):
                same_bytes(u, narrowed(v, scale, odt), "%s in, %s out, R=%d: the turn comes before the narrowing, ch%d" % (ifmt, ofmt, R, c))
            p.set_fine_tuning(None)
            p.reset()
            off = p.work_iq(xi, scale=sc_in)
            d_off = p.describe()
            for c, (u, v) in enumerate(zip(off, plain)):
                same_bytes(u, narrowed(v, scale, odt), "%s in, %s out, R=%d, switched off again, ch%d" % (ifmt, ofmt, R, c))
            if not FORCED:
                for words in ("input %s: fused" % ifmt, "output %s: narrowed" % ofmt, "fine tuning: rotated"):
                    assert words in d, (words, d)
                assert ("output %s: fused" % ofmt) in d_off and "fine tuning" not in d_off, d_off


# ---- 5. edge frequencies -----------------------------------------------------------------------------------------------------------------------------

FAR = [0.125, -0.125, NEAR_HALF, -NEAR_HALF]
FOUR8192 = MIXED + [(3000, 512, 0.75, 0.95), (7001, 128, 0.7, 0.9)]


@pytest.mark.parametrize("N,chans,want", [(4096, EXAMPLE, "fused"), (8192, FOUR8192, "rotated")], ids=["fused", "rotated"])
@pytest.mark.parametrize("first", [0, 2 ** 40 + 3], ids=["block 0", "block 2^40 + 3"])
def test_quarter_turn_boundary_and_half_turn_far_into_the_stream(N, chans, want, first):
    R, nb = 2, 4
    H = N - N // R
    x = stream(nb * H, 500 + N // 4096)
    halo = signal(N // R, 24) if first else None
    nu = np.array(FAR)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    p.set_fine_tuning(nu)
    got = work_span(p, halo, x, first, nb)
    d = p.describe()
    p.set_fine_tuning(None)
    plain = work_span(p, halo, x, first, nb)
    all_hold(got, plain, nu, p.lout, first, "first_block %d" % first)
    assert FORCED or ("fine tuning: " + want) in d, d


def test_every_edge_frequency_is_used_on_both_routes():
    """the frequencies of the cases above, as their parameters give them: every value of EDGES is launched on the fused and on the rotated route"""
    fused = {float(v) for k in range(len(F4)) for R in F4_R for v in fused_nus(k, R)} | set(FAR)
    rotated = {float(v) for k in range(len(ROTATED)) for v in rotated_nus(k)} | {float(v) for k in range(len(FORMS)) for v in form_nus(k)} | set(FAR)
    assert set(EDGES) <= fused, sorted(set(EDGES) - fused)
    assert set(EDGES) <= rotated, sorted(set(EDGES) - rotated)
    assert G.fine_tuning_increment(2.0 ** -64) == 1 and G.fine_tuning_increment(-2.0 ** -64) == 2 ** 64 - 1
