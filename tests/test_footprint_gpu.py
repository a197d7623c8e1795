"""GPU tests (-m gpu): every entry writes exactly its output bytes and nothing else (tests/footprint.py; the checker itself is proved on the CPU by
tests/test_footprint_cpu.py).

The other files compare WHAT the kernels wrote; this one looks at WHERE.  Every output buffer of a call (d_out, d_spectrum, d_group_power, the caller's
outs[c], spectrum and waterfall rows on the host) is the payload of a banded allocation, filled with a poison byte before the call; afterwards the payload
must hold the expected bytes and every guard byte the poison byte, under 0xA5 and under 0x5A.  Every device ring is surrounded by NaN (float) or the
type's minimum (sc16 / sc8) and must come back unchanged.

Expected bytes: a second, fresh handle of the same plan, flags and settings run through the host entry (work / work_iq / work_real) on the same input
from block 0; the device calls use first_block = 0 and a zero halo, so both are the same stream.  (The host entries refuse nblocks > max_blocks, so the
second handle's max_blocks is the call's block count where that is above the first one's: max_blocks sizes buffers and bounds a launch group, it does not
enter any sample.)  The existing files hold the host entries against the oracle and the numpy models; this file adds the footprint only, and compares byte
for byte throughout: there is no tolerance in it.  The one output no host entry hands out, the 16-bin group powers, is compared with the same device entry
of a fresh handle on exact-size buffers.

Known limit of the method: a read outside the ring that never reaches an output byte, and stores into the handle's internal scratch, are invisible here.

245 cases; the file takes 11 s on one MI355X, its slowest case 0.3 s (nothing had to be cut: the N = 262144 plan and the 261-block cases take 0.1 to 0.2 s)."""
import ctypes as C

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
import footprint as F
from test_fine_tuning_routes_gpu import DeviceBuffers, edge_nus, int_scale
from test_fused4096_gpu import plans as fused_plans
from test_gains_cpu import draw_gains
from test_gains_gpu import FORMS
from test_iq_input_gpu import EXAMPLE, FORCED, iq, plans as iq_plans, same_bytes
from test_iq_output_gpu import EXTRA, route, signal
from waterfall_model import power_stream

pytestmark = pytest.mark.gpu

ODT = {"sc16": np.int16, "sc8": np.int8}
SAMPLE_BYTES = {None: 8, "sc16": 4, "sc8": 2}
IN_SCALE = {"sc16": 2.0 ** -15, "sc8": 2.0 ** -7}
# k_blknar's other width: plans() has the 64-bin bank only
BANK128 = ("uniform 128-bin bank", 16384, 2, [(128 * c, 128, 0.88, 1.0) for c in range(128)], 0, "widened", False)
PLANS = iq_plans() + EXTRA + [BANK128]
assert len(PLANS) == 26
plan_ids = [c[0] for c in PLANS]


def settings(h, fmt=None, scale=1.0, nu=None, gains=None, levels=False):
    h.set_output_format(fmt, scale if fmt else 1.0)
    h.set_fine_tuning(nu)
    h.set_gains(gains)
    h.set_levels(levels)


def host_run(q, x, nb, in_fmt):
    """nb blocks from block 0 of the stream x through the host entry of handle q"""
    q.reset()
    if in_fmt:
        return q.work_iq(x[:2 * nb * q.H], scale=IN_SCALE[in_fmt])
    return q.work(x[:nb * q.H])


def device_layout(p, outs, nb, fmt):
    """the bytes of d_out after a call of nb blocks: channel c's stream at channel_offset(c, nb), the streams tiling the buffer exactly"""
    ssz = SAMPLE_BYTES[fmt]
    n = p.output_samples(nb)
    flat, seen = np.zeros(n * ssz, np.uint8), np.zeros(n, bool)
    for c, o in enumerate(outs):
        a, cnt = p.channel_offset(c, nb), nb * p.lout[c]
        assert not seen[a:a + cnt].any() and a + cnt <= n
        seen[a:a + cnt] = True
        flat[a * ssz:(a + cnt) * ssz] = F.as_bytes(o)
    assert seen.all()
    return flat


def stream_of(in_fmt, n, seed):
    return iq(n, ODT[in_fmt], seed) if in_fmt else signal(n, seed)


def ring_of(x, nb, p, in_fmt):
    """(the device ring of a call of nb blocks from block 0: a zero halo and the samples; the elements of one block)"""
    per = 2 if in_fmt else 1
    return np.concatenate([np.zeros(per * p.ovl, x.dtype), x[:per * nb * p.H]]), per * p.H


def run_device(case, nbs, mb, fmt=None, in_fmt=None, chunk=0, nu=None, gains=None, levels=False, seed=0):
    """The device entry of `case` on a handle of max_blocks = mb, at every block count of nbs, against the host entry of a second handle; d_out banded, the
    ring surrounded.  Returns (the handle, its describe() after every block count)."""
    name, N, R, chans, flags, _r_in, keep = case
    kw = dict(windowtype=1, flags=flags, keep_spectrum=keep)
    p = G.Pipeline(N, R, chans, max_blocks=mb, chunk_blocks=chunk, **kw)
    q = G.Pipeline(N, R, chans, max_blocks=max(max(nbs), mb), **kw)
    assert chunk == 0 or p.chunk_blocks() == chunk
    x = stream_of(in_fmt, max(nbs) * p.H, 700 + seed)
    scale = 1.0
    if fmt:
        settings(q, None, 1.0, nu, gains)
        scale = int_scale(host_run(q, x, nbs[0], in_fmt), ODT[fmt])
    for h in (p, q):
        settings(h, fmt, scale, nu, gains, levels)
    described = []
    for nb in nbs:
        what = "%s, %s in, %s out, %d blocks" % (name, in_fmt or "fc32", fmt or "fc32", nb)
        want = host_run(q, x, nb, in_fmt)
        want_lev = q.levels() if levels else None
        flat = device_layout(p, want, nb, fmt)
        ring, block = ring_of(x, nb, p, in_fmt)
        with DeviceBuffers() as dev:
            d_ring = F.DeviceRing(dev, ring, block)
            band = F.DeviceBanded(dev, [flat.size], p.output_samples(1) * SAMPLE_BYTES[fmt])
            for _byte in F.twice(band):
                if in_fmt:
                    p.process_device_iq(in_fmt, IN_SCALE[in_fmt], d_ring.ptr, 0, nb, band.ptr())
                else:
                    p.process_device(d_ring.ptr, 0, nb, band.ptr())
                p.synchronize()
                band.check(flat, what)
                d_ring.unchanged(what)
                if levels:
                    same_bytes(p.levels(nb), want_lev, what + ": the levels")
        described.append(p.describe())
    return p, described


# ---- a. the device entries on every route ----------------------------------------------------------------------------------------------------------------

def float_counts(N):
    """1, 3, 4, 5, 9 around max_blocks = 4: 5 and 9 are several launch groups (mbase != 0, nb_call != nb_chunk); from N = 65536 on 1, 3, 5 (time)"""
    return (1, 3, 5) if N >= 65536 else (1, 3, 4, 5, 9)


def input_route(case):
    """the route the tables of test_iq_input_gpu.py / test_iq_output_gpu.py name, which for the two keep_spectrum plans is that of a call WITH a spectrum;
    the calls here ask for none, and those two plans (k_f4096, k_blk256) then take their integers in their own loads and stores"""
    return "fused" if case[6] else case[5]


def kernel_names_hold(case, p, d):
    name = case[0]
    if "k_f4096" in name:
        assert p.path() == 5 and "k_f4096" in d, (name, d)
        assert ("one block" if "one block" in name else "two blocks") in d, (name, d)


@pytest.mark.parametrize("fmt", [None, "sc16", "sc8"], ids=["fc32 out", "sc16 out", "sc8 out"])
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_device_entry_on_every_route(k, fmt):
    """process_device on all 26 plans, max_blocks = 4.  Float output at 1, 3, 4, 5 and 9 blocks; sc16 / sc8 output at 1, 3 and 4 (a narrowed device call
    needs nblocks <= max_blocks, include/fdc_amd.h)."""
    case = PLANS[k]
    name, N, R = case[:3]
    r_in = input_route(case)
    p, ds = run_device(case, (1, 3, 4) if fmt else float_counts(N), 4, fmt=fmt, seed=k)
    if not FORCED:
        kernel_names_hold(case, p, ds[-1])
        if fmt:
            # (N = 65536 at R = 4 on float input narrows behind the float kernel: test_iq_output_gpu.py)
            want = "fused" if r_in == "fused" and not (N == 65536 and R == 4) else "narrowed"
            assert all(("output %s: %s" % (fmt, want)) in d for d in ds), (name, ds)


INT_CASES = [(k, "sc16") for k in range(len(PLANS))] + [(k, "sc8") for k in range(len(PLANS)) if PLANS[k][5] == "fused"]


@pytest.mark.parametrize("k,in_fmt", INT_CASES, ids=["%s, %s in" % (PLANS[k][0], f) for k, f in INT_CASES])
def test_device_entry_with_integer_input(k, in_fmt):
    """process_device_iq: sc16 input on every plan, sc8 input where the kernels read the integers in their own loads; float output and output of the
    input's format (the integer loads of the forms with integer stores), 1, 3 and 4 blocks"""
    case = PLANS[k]
    name, r_in = case[0], input_route(case)
    for fmt in (None, in_fmt):
        p, ds = run_device(case, (1, 3, 4), 4, fmt=fmt, in_fmt=in_fmt, seed=100 + k)
        if not FORCED:
            kernel_names_hold(case, p, ds[-1])
            assert all(("input %s: %s" % (in_fmt, r_in)) in d for d in ds), (name, ds)
            if fmt:
                assert route(p) == ("fused" if r_in == "fused" else "narrowed"), (name, ds)


CHUNKED = [PLANS[0], [c for c in PLANS if c[0].startswith("configs[0] example plan")][0], [c for c in PLANS if "path 0" in c[0]][0]]


@pytest.mark.parametrize("case", CHUNKED, ids=[c[0] for c in CHUNKED])
def test_a_handle_with_launch_groups_of_two(case):
    """chunk_blocks = 2: five blocks are launch groups at mbase 0, 2 and 4 (the last of one block)"""
    p, ds = run_device(case, (5,), 5, chunk=2, seed=50)
    if not FORCED:
        kernel_names_hold(case, p, ds[-1])


# ---- b. the row classes of the one-launch kernel ---------------------------------------------------------------------------------------------------------

F4 = list(fused_plans().items())
assert len(F4) == 17


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("k", range(len(F4)), ids=[name for name, _ in F4])
def test_every_row_class_of_the_fused_route(k, R):
    """nb = 1: one valid block in a two-block workgroup; 2; 5: an odd count, and two launch groups on a handle of max_blocks = 4"""
    name, chans = F4[k]
    p, ds = run_device((name, 4096, R, chans, None, "fused", False), (1, 2, 5), 4, seed=200 + k + R)
    assert FORCED or (p.path() == 5 and all("k_f4096" in d for d in ds)), ds


# ---- c. the passes behind the kernels -----------------------------------------------------------------------------------------------------------------------

SETTINGS = [("fine tuning", True, False, False), ("gains", False, True, False), ("levels", False, False, True), ("fine tuning, gains and levels", True, True, True)]


@pytest.mark.parametrize("fmt", [None, "sc16", "sc8"], ids=["fc32 out", "sc16 out", "sc8 out"])
@pytest.mark.parametrize("s", range(len(SETTINGS)), ids=[s[0] for s in SETTINGS])
@pytest.mark.parametrize("k", range(len(FORMS)), ids=[f[0] for f in FORMS])
def test_the_passes_behind_the_kernels(k, s, fmt):
    """k_fine_rotate in its forms (plain, with the levels, with the gains), k_chan_gain in place and with the narrowing, k_chan_levels, and k_f4096_fine,
    into a banded d_out at 1 and 4 blocks; the levels afterwards from the handle, byte for byte those of the host entry"""
    name, N, chans = FORMS[k]
    what, fine, gain, lev = SETTINGS[s]
    nu = edge_nus(len(chans), 3 * k + s) if fine else None
    g = draw_gains(len(chans), 60 + k) if gain else None
    p, ds = run_device((name + ", " + what, N, 2, chans, None, "", False), (1, 4), 4, fmt=fmt, nu=nu, gains=g, levels=lev, seed=300 + k)
    for d in ds:
        assert ("fine tuning: " in d) == fine and ("gains: " in d) == gain and ("levels: " in d) == lev, d
    if not FORCED and fine:
        # (path 5 turns the samples in its own stores whatever runs behind it; every other plan takes k_fine_rotate)
        assert all(("fine tuning: fused" if N == 4096 else "fine tuning: rotated") in d for d in ds), ds


# ---- d. more blocks than workgroups -----------------------------------------------------------------------------------------------------------------------

PERSISTENT = [("k_blk256", 16384, [(256 * c, 256, 0.88, 1.0) for c in range(64)]), ("k_blk512", 32768, [(512 * c, 512, 0.8, 0.95) for c in (0, 3, 17, 40, 63)]),
              ("k_blknar", 16384, [(128 * c, 128, 0.88, 1.0) for c in range(0, 128, 3)])]


@pytest.mark.parametrize("kernel,N,chans", PERSISTENT, ids=[c[0] for c in PERSISTENT])
def test_more_blocks_than_workgroups(kernel, N, chans):
    """261 blocks in ONE launch group (max_blocks = 261): the persistent kernels loop over the blocks of a workgroup, and the last round is partial"""
    p, ds = run_device((kernel + " bank", N, 2, chans, None, "", False), (261,), 261, seed=400)
    assert FORCED or (p.path() == 3 and kernel in ds[0]), ds


# ---- e. spectrum and group powers ---------------------------------------------------------------------------------------------------------------------------

KEEP = [c for c in PLANS if c[6]] + [("keep_spectrum, 256-bin bank at N = 16384", 16384, 2, [(256 * c, 256, 0.88, 1.0) for c in range(64)], 0, "widened", True)]
assert len(KEEP) == 3
# (plan, min_block_launch): under the suite's min_block_launch = 1 the forward block kernel of N = 16384 / 65536 sums the groups in its epilogue; at the
# default of 96 a launch group of 1 to 5 blocks takes the tiled transform and the pass over the spectrum, which N = 4096 always takes
SPECTRA = [(KEEP[0], None), (KEEP[1], None), (KEEP[2], None), (KEEP[2], 96)]


@pytest.mark.parametrize("power", [True, False], ids=["process_device_power", "process_device with a spectrum"])
@pytest.mark.parametrize("case,mbl", SPECTRA, ids=["%s%s" % (c[0], ", short groups" if m else "") for c, m in SPECTRA])
def test_spectrum_and_group_powers(case, mbl, power):
    """d_out, d_spectrum (nb * N complex64) and d_group_power (nb * N / 16 float32), each banded on its own, at 1, 3 and 5 blocks of a handle with
    max_blocks = 4.  Channels and spectrum against work(want_spectrum = True); the group powers, which no host entry hands out, against the same entry
    of a fresh handle on exact-size buffers."""
    name, N, R, chans, flags, _r_in, _keep = case
    kw = dict(windowtype=1, flags=flags, keep_spectrum=True, min_block_launch=mbl)
    p, q, r = (G.Pipeline(N, R, chans, max_blocks=mb, **kw) for mb in (4, 5, 4))
    x = signal(5 * p.H, 500)
    for nb in (1, 3, 5):
        what = "%s, %d blocks" % (name, nb)
        q.reset()
        want, want_spec = q.work(x[:nb * p.H], want_spectrum=True)
        flat = device_layout(p, want, nb, None)
        assert np.abs(want_spec).max() > 0
        ring, block = ring_of(x, nb, p, None)
        with DeviceBuffers() as dev:
            d_ring = F.DeviceRing(dev, ring, block)
            bands = [F.DeviceBanded(dev, [flat.size], 8 * p.output_samples(1)), F.DeviceBanded(dev, [8 * nb * N], 8 * N)]
            expected = [flat, want_spec]
            if power:
                exact = [dev.put(np.zeros(n, np.uint8)) for n in (flat.size, 8 * nb * N, 4 * nb * N // 16)]
                r.process_device(dev.put(ring), 0, nb, exact[0], exact[1], d_group_power=exact[2])
                r.synchronize()
                gp = dev.get(exact[2], nb * N // 16, np.float32)
                assert gp.min() > 0
                same_bytes(dev.get(exact[1], nb * N, np.complex64), want_spec, what + ": the spectrum of the exact-size call")
                bands.append(F.DeviceBanded(dev, [gp.nbytes], 4 * N // 16))
                expected.append(gp)
            for _byte in F.twice(*bands):
                p.process_device(d_ring.ptr, 0, nb, bands[0].ptr(), bands[1].ptr(), d_group_power=bands[2].ptr() if power else None)
                p.synchronize()
                for b, e, buf in zip(bands, expected, ("d_out", "d_spectrum", "d_group_power")):
                    b.check(e, "%s: %s" % (what, buf))
                d_ring.unchanged(what)


# ---- f. the host entries ----------------------------------------------------------------------------------------------------------------------------------

HOST_PLANS = [("example, N = 4096", 4096, EXAMPLE), FORMS[0]]
assert FORMS[0][1] == 8192


def host_band(p, nb, fmt):
    """outs[c] as views of ONE banded host array, a guard between every pair of channels"""
    ssz = SAMPLE_BYTES[fmt]
    band = F.HostBanded([nb * lo * ssz for lo in p.lout], max(p.lout) * ssz)
    outs = [band.view(c, ODT[fmt], (-1, 2)) if fmt else band.view(c, np.complex64) for c in range(len(p.lout))]
    return band, outs


@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["fc32 out", "sc16 out"])
@pytest.mark.parametrize("sub", [0, 2], ids=["one sub-batch", "sub-batches of 2"])
@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("in_fmt", [None, "sc16"], ids=["work", "work_iq"])
@pytest.mark.parametrize("k", range(len(HOST_PLANS)), ids=[c[0] for c in HOST_PLANS])
def test_host_entries(k, in_fmt, registered, sub, fmt):
    """work(x, outs = ...) and work_iq(..., outs = ...): staged through the handle's pinned memory, or stored straight into the caller's array after
    register_host (k_scatter_out / k_scatter_oq); five blocks, in one sub-batch or in sub-batches of 2, 2 and 1"""
    name, N, chans = HOST_PLANS[k]
    R, nb = 2, 5
    p = G.Pipeline(N, R, chans, max_blocks=nb, host_sub_blocks=sub or None)
    q = G.Pipeline(N, R, chans, max_blocks=nb)
    x = stream_of(in_fmt, nb * p.H, 600 + k)
    scale = int_scale(host_run(q, x, nb, in_fmt), ODT[fmt]) if fmt else 1.0
    for h in (p, q):
        settings(h, fmt, scale)
    want = host_run(q, x, nb, in_fmt)
    band, outs = host_band(p, nb, fmt)
    xin = F.HostRing(x, (2 if in_fmt else 1) * p.H)
    what = "%s, %s, %s out" % (name, "work_iq" if in_fmt else "work", fmt or "fc32")
    if registered:
        G.register_host(band.mem)
    try:
        for _byte in F.twice(band):
            p.reset()
            got = p.work_iq(xin.ring, scale=IN_SCALE[in_fmt], outs=outs) if in_fmt else p.work(xin.ring, outs=outs)
            assert got is outs
            band.check(want, what)
            xin.unchanged(what)
    finally:
        if registered:
            G.unregister_host(band.mem)


def pointers(outs):
    return (C.c_void_p * max(1, len(outs)))(*[o.ctypes.data for o in outs])


@pytest.mark.parametrize("k", range(len(HOST_PLANS)), ids=[c[0] for c in HOST_PLANS])
def test_the_spectrum_pointer_of_work(k):
    """fdc_pipeline_work with a spectrum (the Python face allocates it): nb * N complex64 in a banded host array, the channels in another"""
    name, N, chans = HOST_PLANS[k]
    R, nb = 2, 5
    p, q = (G.Pipeline(N, R, chans, max_blocks=nb, keep_spectrum=True) for _ in range(2))
    x = signal(nb * p.H, 610 + k)
    want, want_spec = q.work(x, want_spectrum=True)
    band, outs = host_band(p, nb, None)
    spec = F.HostBanded([8 * nb * N], 8 * N)
    xin = F.HostRing(x, p.H)
    for _byte in F.twice(band, spec):
        p.reset()
        _lib.check(_lib.lib().fdc_pipeline_work(p._h, xin.ring.ctypes.data, nb, pointers(outs), spec.view(0, np.uint8).ctypes.data))
        band.check(want, name + ": the channels")
        spec.check(want_spec, name + ": the spectrum")
        xin.unchanged(name)


@pytest.mark.parametrize("fmt", [None, "sc16"], ids=["fc32 out", "sc16 out"])
@pytest.mark.parametrize("k", range(len(HOST_PLANS)), ids=[c[0] for c in HOST_PLANS])
def test_work_real(k, fmt):
    """fdc_pipeline_work_real (the Python face allocates its outputs): float32 input inside NaN, banded outputs"""
    name, N, chans = HOST_PLANS[k]
    R, nb = 2, 5
    p, q = (G.Pipeline(N, R, chans, max_blocks=nb) for _ in range(2))
    xr = signal(nb * p.H, 620 + k).real.copy()
    scale = int_scale(q.work_real(xr), ODT[fmt]) if fmt else 1.0
    for h in (p, q):
        settings(h, fmt, scale)
    q.reset()
    want = q.work_real(xr)
    band, outs = host_band(p, nb, fmt)
    xin = F.HostRing(xr, p.H)
    for _byte in F.twice(band):
        p.reset()
        _lib.check(_lib.lib().fdc_pipeline_work_real(p._h, xin.ring.ctypes.data, nb, pointers(outs), None))
        band.check(want, name + ": work_real")
        xin.unchanged(name)


# ---- g. waterfall rows --------------------------------------------------------------------------------------------------------------------------------------

WIDTH = 1024
ROW_BYTES = (4 * WIDTH, 2 * WIDTH, 3 * WIDTH)           # rows float32, index uint16, rgb 3 bytes
WF_D, WF_CALLS = 4, (5, 5)                              # blocks 0-3 finish row 0 in the first call, block 4 waits; the second call finishes row 1 with 5-7
LEVELS = (-45.0, -20.0)


def rows_expected(rows, cap, byte):
    """what the three buffers of cap rows must hold: the n finished rows, and the poison byte behind them (the library's stated behaviour)"""
    out = []
    for a, rb in zip(rows, ROW_BYTES):
        e = np.full(cap * rb, byte, np.uint8)
        e[:a.shape[0] * rb] = F.as_bytes(a)
        out.append(e)
    return out


WF_PLANS = [("rows in k_f4096", 4096, 4, EXAMPLE, "k_f4096 epilogue"), ("rows from the spectrum", 8192, 2, [(100, 256, 0.8, 1.0), (3000, 512, 0.7, 0.95)], "k_wf_from_spectrum")]


@pytest.mark.parametrize("name,N,R,chans,words", WF_PLANS, ids=[c[0] for c in WF_PLANS])
def test_pipeline_waterfall_rows(name, N, R, chans, words):
    """fdc_pipeline_work_waterfall with cap_rows = rows_for(nb) exactly: rows, index and rgb as three payloads of one banded host array, the channels in
    another.  A block decimation of 4 on calls of 5 and 5 blocks: the first call leaves an unfinished group, the second finishes it; each finishes one
    row of the two it has room for.  The stream has a state, so every poison byte gets fresh handles."""
    nb = WF_CALLS[0]
    assert all(n == nb for n in WF_CALLS)
    x = signal(sum(WF_CALLS) * (N - N // R), 630)
    band, outs = host_band(G.Pipeline(N, R, chans, max_blocks=nb), nb, None)
    cap = (nb + WF_D - 1) // WF_D
    rows = F.HostBanded([cap * rb for rb in ROW_BYTES], ROW_BYTES[0])
    for byte in F.twice(band, rows):
        p, q = (G.Pipeline(N, R, chans, max_blocks=nb) for _ in range(2))
        w, wq = (G.Waterfall(N, 1e6, R, WF_D, 0, *LEVELS, 0, 0, max_items=nb) for _ in range(2))
        assert w.rows_for(nb) == cap == 2
        for k in range(len(WF_CALLS)):
            xs = np.ascontiguousarray(x[k * nb * p.H:(k + 1) * nb * p.H])
            want, want_rows = q.work_waterfall(xs, wq)
            assert want_rows.power.shape[0] == 1
            band.fill(byte)
            rows.fill(byte)
            n = C.c_int32(-1)
            _lib.check(_lib.lib().fdc_pipeline_work_waterfall(p._h, w._h, xs.ctypes.data, nb, pointers(outs), rows.view(0, np.uint8).ctypes.data,
                                                              rows.view(1, np.uint8).ctypes.data, rows.view(2, np.uint8).ctypes.data, cap, C.byref(n)))
            assert n.value == 1
            band.check(want, "%s, call %d: the channels" % (name, k))
            rows.check(rows_expected(want_rows, cap, byte), "%s, call %d: rows, index, rgb" % (name, k))
        assert FORCED or words in p.describe(), p.describe()


@pytest.mark.parametrize("N", [512, 4096])
def test_standalone_waterfall_rows(N):
    """fdc_waterfall_work on float32 power vectors inside NaN, max_items = 3: several internal passes a call"""
    nb = WF_CALLS[0]
    pw = power_stream(sum(WF_CALLS), N, seed=N)
    cap = (nb + WF_D - 1) // WF_D
    rows = F.HostBanded([cap * rb for rb in ROW_BYTES], ROW_BYTES[0])
    for byte in F.twice(rows):
        w, wq = (G.Waterfall(N, 1e6, 4, WF_D, 0, *LEVELS, 1, 0, max_items=3) for _ in range(2))
        assert w.rows_for(nb) == cap == 2
        for k in range(len(WF_CALLS)):
            xin = F.HostRing(pw[k * nb:(k + 1) * nb].reshape(-1), N)
            want_rows = wq.work(xin.ring)
            assert want_rows.power.shape[0] == 1
            rows.fill(byte)
            n = C.c_int32(-1)
            _lib.check(_lib.lib().fdc_waterfall_work(w._h, xin.ring.ctypes.data, nb, rows.view(0, np.uint8).ctypes.data, rows.view(1, np.uint8).ctypes.data,
                                                     rows.view(2, np.uint8).ctypes.data, cap, C.byref(n)))
            assert n.value == 1
            rows.check(rows_expected(want_rows, cap, byte), "N = %d, call %d: rows, index, rgb" % (N, k))
            xin.unchanged("N = %d" % N)
