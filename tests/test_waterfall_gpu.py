"""GPU tests (-m gpu) of the waterfall rows (include/fdc_amd.h fdc_waterfall_*, fdc_pipeline_work_waterfall; csrc/fdc_waterfall.hip and the
ROWS epilogue of csrc/fdc_fused4096.hip) against the numpy model of FDC.WaterfallMsgTagging's arithmetic (tests/waterfall_model.py).

Rows: relative error <= 1e-6 per pixel where the input is the same float32 power (the standalone face, the pipeline's own spectrum); colour
indices equal wherever the model's pixel lies further than 1e-5 (relative) from an edge, the others counted and reported; RGB = table[index]."""
import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import waterfall as WF
from test_parity_gpu import noise
from waterfall_model import block_rows, decimate, model_edges, colour_index, near_edge, power_stream

pytestmark = pytest.mark.gpu
FORCED = any(G.defaults.get(k) for k in ("FDC_FORCE_GENERIC", "FDC_NO_POLY", "FDC_NO_FUSED"))
EXAMPLE = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]      # test_fused4096_gpu.py
NARROW = [(300 + 900 * c + c, 256, 0.8, 1.0) for c in range(4)]            # configs[0]: no wide rows, one block per workgroup (T = 1)
LEVELS = (-45.0, -20.0)                                                    # examples/FDC_example.grc


def check_rows(got, model_rows, loginput=0, levels=LEVELS, scheme=0, rel=1e-6, what=""):
    """got: Rows; model_rows: float64 [n, 1024].  Returns the number of pixels near an edge (index not compared)."""
    assert got.power.shape == model_rows.shape, (what, got.power.shape, model_rows.shape)
    err = np.abs(got.power.astype(np.float64) - model_rows) / np.maximum(np.abs(model_rows), 1e-300)
    assert err.max() <= rel, "%s: rows rel err %.3g" % (what, err.max())
    e = model_edges(loginput, *levels)
    want = colour_index(got.power, e)                                      # the library's float32 value, digitized as numpy would
    assert np.array_equal(got.index, want), what
    far = ~near_edge(model_rows, e)
    assert np.array_equal(got.index[far], colour_index(model_rows, e)[far]), what
    table, _ = WF.color_table(scheme)
    assert np.array_equal(got.rgb, table[got.index]), what
    return int((~far).sum())


@pytest.mark.parametrize("N", [512, 1024, 4096, 65536])
@pytest.mark.parametrize("D", [1, 3, 8])
def test_standalone_face_vs_model(N, D):
    nitems = 24 if N < 65536 else 17
    pw = power_stream(nitems, N, seed=N + D)
    w = G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 1, 0, max_items=10)      # max_items < nitems: several internal passes
    got = w.work(pw)
    near = check_rows(got, decimate(block_rows(pw), D), scheme=1, what="N=%d D=%d" % (N, D))
    assert near <= got.power.size // 1000, near
    assert w.rows_done() == nitems // D
    # the same input again after reset: the same bytes
    w.reset()
    again = w.work(pw)
    assert again.power.tobytes() == got.power.tobytes() and again.index.tobytes() == got.index.tobytes()


def test_more_rows_than_one_finish_grid_holds():
    """k_wf_finish walks rows in steps of its grid's height (4096): 5000 rows of one call"""
    N, n = 512, 5000
    pw = power_stream(n, N, seed=12)
    w = G.Waterfall(N, 1e6, 4, 1, 0, *LEVELS, 0, 0, max_items=n)
    check_rows(w.work(pw), block_rows(pw), what="5000 rows")


def test_log_input_levels_and_scheme_callbacks():
    N, D = 2048, 2
    pw = (10 * np.log10(power_stream(8, N, seed=5))).astype(np.float32)      # already in dB (loginput = 1)
    w = G.Waterfall(N, 1e6, 4, D, 1, -50.0, -10.0, 3, 0)
    check_rows(w.work(pw), decimate(block_rows(pw), D), loginput=1, levels=(-50.0, -10.0), scheme=3, rel=1e-6, what="loginput")
    w.set_minvaldb(-40.3)                                                   # not a float32: the edges come from the double levels
    w.set_maxvaldb(-30.1)
    w.set_colorscheme(2)
    check_rows(w.work(pw), decimate(block_rows(pw), D), loginput=1, levels=(-40.3, -30.1), scheme=2, rel=1e-6, what="callbacks")


def test_carry_across_calls_is_byte_identical_to_one_call():
    N, D = 4096, 5
    pw = power_stream(23, N, seed=9)
    one = G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 0, 0).work(pw)
    w = G.Waterfall(N, 1e6, 4, D, 0, *LEVELS, 0, 0)
    parts, counts, b = [], [], 0
    for n in (7, 1, 13, 2):
        r = w.work(pw[b:b + n])
        b += n
        parts.append(r)
        counts.append(r.power.shape[0])
    assert counts == [1, 0, 3, 0]                                      # the unfinished group of a call is finished by a later one
    for k in ("power", "index", "rgb"):
        cat = np.concatenate([getattr(r, k) for r in parts])
        assert cat.tobytes() == getattr(one, k).tobytes(), k
    check_rows(one, decimate(block_rows(pw), D), what="carry")


def spectrum_rows(spec, N):
    return block_rows(np.abs(spec.reshape(-1, N).astype(np.complex128)) ** 2)


@pytest.mark.parametrize("name,chans", [("example", EXAMPLE), ("no wide rows", NARROW)])
@pytest.mark.parametrize("D", [1, 3])
def test_fused_4096_rows_channels_bit_identical(oracle, name, chans, D):
    N, R, nb = 4096, 4, 37
    H = N - N // R
    x = noise(2 * nb * H, 77 + D)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    q = G.Pipeline(N, R, chans, max_blocks=nb)
    w = G.Waterfall(N, 1e6, R, D, 0, *LEVELS, 0, 0, max_items=nb)
    assert FORCED or p.path() == 5, p.describe()
    outs, rows = [], []
    for k in range(2):
        o, r = p.work_waterfall(x[k * nb * H:(k + 1) * nb * H], w)
        outs.append(o)
        rows.append(r)
    assert FORCED or p.path() == 5
    assert FORCED or "k_f4096 epilogue" in p.describe(), p.describe()
    for k in range(2):
        ref = q.work(x[k * nb * H:(k + 1) * nb * H])
        for c, (a, b) in enumerate(zip(outs[k], ref)):
            assert a.tobytes() == b.tobytes(), (name, k, c)
    got = WF.Rows(*[np.concatenate([getattr(r, f) for r in rows]) for f in WF.Rows._fields])
    # the pipeline's own spectrum (two-launch path, keep_spectrum): the same float32 bins the epilogue sums
    s = G.Pipeline(N, R, chans, max_blocks=2 * nb, keep_spectrum=True, flags=G.FDC_PIPE_NO_FUSED)
    _o, spec = s.work(x, want_spectrum=True)
    check_rows(got, decimate(spectrum_rows(spec, N), D), rel=1e-6, what="%s D=%d vs own spectrum" % (name, D))
    # and the oracle's spectrum: bins agree to the parity tolerance (1e-5 of the largest), so pixels far below the peak agree less closely
    _r, ospec = oracle.channelizer(N, R, 1, chans, x, want_spectrum=True)
    m = decimate(spectrum_rows(ospec, N), D)
    assert np.abs(got.power - m).max() <= 1e-5 * m.max()
    e = model_edges(0, *LEVELS)
    far = ~near_edge(m, e, rel=1e-3)
    assert np.array_equal(got.index[far], colour_index(m, e)[far])
    print("%s D=%d: %d of %d pixels within 1e-3 of an edge" % (name, D, int((~far).sum()), m.size))


def test_waterfall_entry_refuses_mismatches_and_small_caps():
    N, R = 4096, 4
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=8)
    x = noise(8 * (N - N // R), 1)
    with pytest.raises(G.FdcError):
        p.work_waterfall(x, G.Waterfall(8192, 1e6, R, 1, 0, *LEVELS, 0, 0, max_items=8))
    with pytest.raises(G.FdcError):
        p.work_waterfall(x, G.Waterfall(N, 1e6, R, 1, 0, *LEVELS, 0, 0, max_items=4))


@pytest.mark.parametrize("name,chans,flags,path", [
    ("configs[1]-shaped plan (path 3 without rows)", [(256 * c, 256, 0.88, 1.0) for c in (0, 1, 17, 64, 127, 128, 200, 255)], None, 3),
    ("mixed plan (path 1)", [(100, 256, 0.8, 1.0), (5001, 512, 0.7, 0.95), (30001, 1024, 0.8, 1.0), (60000, 128, 0.8, 1.0)],
     G.FDC_PIPE_NO_POLY, 1),
])
@pytest.mark.parametrize("nb", [8, 100])
def test_group_sum_route_at_65536(oracle, name, chans, flags, path, nb):
    """Plans off path 5 take the spectrum path for a waterfall call, whatever their path without rows (fdc_pipeline_path() names the plan's
    path; a call with rows runs the spectrum path, as a call with a debug spectrum does).  Both block counts take the block forward kernel, whose
    epilogue sums the 16-bin groups: the suite runs with the block kernels' minimum at one block (conftest.py, FDC_BLOCK_MIN_BLOCKS), so nb = 8
    is not below it.  The two-pass transform with a pass over the spectrum (k_group_power) behind it is run by
    test_waterfall_routes_gpu.py::test_group_sum_route_at_every_r, which takes the minimum back to its default or forbids the block kernels."""
    N, R, D = 65536, 2, 3
    H = N - N // R
    x = noise(nb * H, 5 + nb)
    p = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags)
    assert FORCED or p.path() == path, p.describe()
    w = G.Waterfall(N, 1e6, R, D, 0, *LEVELS, 0, 0, max_items=nb)
    outs, got = p.work_waterfall(x, w)
    assert "k_wf_from_groups" in p.describe(), p.describe()
    # the channels are those of the same plan's call with a debug spectrum: the same kernels, the same bits
    dbg, _spec = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags, keep_spectrum=True).work(x, want_spectrum=True)
    for a, b in zip(outs, dbg):
        assert a.tobytes() == b.tobytes()
    ref, ospec = oracle.channelizer(N, R, 1, chans, x, want_spectrum=True, nthreads=8)
    m = decimate(spectrum_rows(ospec, N), D)
    assert got.power.shape == m.shape
    err = np.abs(got.power - m) / m
    assert err.max() <= 1e-5, (name, err.max())                       # 64 bins per pixel: the bins' own errors average out
    e = model_edges(0, *LEVELS)
    far = ~near_edge(m, e, rel=1e-4)
    assert np.array_equal(got.index[far], colour_index(m, e)[far])
    q = G.Pipeline(N, R, chans, max_blocks=nb, flags=flags).work(x)
    for a, b in zip(outs, q):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max()


def test_spectrum_route_below_16384(oracle):
    N, R, D, nb = 8192, 2, 2, 12
    chans = [(100, 256, 0.8, 1.0), (3000, 512, 0.7, 0.95)]
    x = noise(nb * (N - N // R), 3)
    p = G.Pipeline(N, R, chans, max_blocks=nb)
    w = G.Waterfall(N, 1e6, R, D, 0, *LEVELS, 0, 0, max_items=nb)
    _o, got = p.work_waterfall(x, w)
    assert "k_wf_from_spectrum" in p.describe(), p.describe()
    _r, ospec = oracle.channelizer(N, R, 1, chans, x, want_spectrum=True)
    m = decimate(spectrum_rows(ospec, N), D)
    assert (np.abs(got.power - m) / m).max() <= 1e-5


def test_hier_block_with_waterfall():
    """FrequencyDomainChannelizer(..., waterfall=...) with the example flowgraph's parameters: the same channel streams as without it, plus rows"""
    user = [[0.12, 0.05], [0.22, 0.1], [-0.14, 0.12], [0, 0.081]]
    args = (8, 1, 2 ** 12, 4, user, None, 6.0, 1.0, 0.0, 'normalized', 1, False, False, "", False, None, 10.0, 0.005, 1, 0.2, 0, 0, 128, 128, False)
    wf = G.Waterfall(4096, 1e6, 4, 1, 0, *LEVELS, 0, 0, max_items=16)
    a = G.FrequencyDomainChannelizer(*args, max_blocks=16, waterfall=wf)
    b = G.FrequencyDomainChannelizer(*args, max_blocks=16)
    s = G.FrequencyDomainChannelizer(*args[:-1], True, max_blocks=16)      # debug port: the spectrum the rows come from
    x = noise(12 * a.inpblocklen, 42)
    ports, rows = a.work(x)
    assert FORCED or a.pipeline.path() == 5
    for p, q in zip(ports, b.work(x)):
        assert p.tobytes() == q.tobytes()
    spec = s.work(x)[0]
    check_rows(rows, spectrum_rows(spec, 4096), rel=1e-6, what="hier")
    assert rows.power.shape == (12, 1024)
