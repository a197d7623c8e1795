"""CPU tests (no GPU) of the host side of the waterfall rows (include/fdc_amd.h, fdc_waterfall_*; gr_fdc_amd.waterfall): the colour tables
against the numpy-built fixture (tests/golden/waterfall_colors.npz, tools/make_waterfall_colors.py), the FP64 edges, the constructor's
argument checks, and the PDU geometry of WaterfallImage (python/WaterfallMsgTagging.py:85-110, :172-241) on hand-computed positions."""
import math
import os

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import waterfall as WF
from waterfall_model import (NEAR_CAP, block_rows, colour_index, decimate, model_edges, near_edge, near_share, noise_levels, noise_stream,
                             route_streams, row_bound, stream_rows)


@pytest.mark.parametrize("scheme", [0, 1, 2, 3])
def test_color_table_matches_the_fixture_byte_for_byte(golden_dir, scheme):
    z = np.load(os.path.join(golden_dir, "waterfall_colors.npz"))
    cols, frame = WF.color_table(scheme)
    assert cols.dtype == np.uint8 and cols.shape == (1024, 3)
    assert np.array_equal(cols, z["cols%d" % scheme])
    assert np.array_equal(frame, z["frame%d" % scheme])


@pytest.mark.parametrize("scheme", [-1, 4, 99])
def test_unknown_scheme_is_scheme_0(golden_dir, scheme):
    z = np.load(os.path.join(golden_dir, "waterfall_colors.npz"))
    cols, frame = WF.color_table(scheme)
    assert np.array_equal(cols, z["cols0"]) and np.array_equal(frame, z["frame0"])


@pytest.mark.parametrize("loginput", [0, 1])
@pytest.mark.parametrize("levels", [(-45.0, -20.0), (-45.3, -20.1), (-120.0, 10.0), (-20.0, -45.0), (-30.0, -30.0), (0.1, 7.3)])
def test_edges_are_linspace_and_ten_to_the_tenth(loginput, levels):
    """linspace bit for bit; 10**(x/10) bit for bit as C's pow (math.pow) gives it, and within one ulp of numpy's array power, which
    takes a vectorised path of its own on some CPUs (so numpy's last bit is a property of the machine, not of the reference)"""
    e = WF.edges(loginput, *levels)
    ref = model_edges(loginput, *levels)
    assert e.shape == (1023,)
    if loginput:
        assert np.array_equal(e.view(np.uint64), ref.view(np.uint64))
    else:
        lin = model_edges(1, *levels)
        assert np.array_equal(e.view(np.uint64), np.array([math.pow(10.0, x / 10.0) for x in lin]).view(np.uint64))
        assert np.all(np.abs(e - ref) <= np.spacing(ref))


def test_check_config_normalises_the_decimation_and_refuses_bad_block_lengths():
    for d in (0, -3):
        assert WF.check_config(4096, d)["blockdecimation"] == 1
    assert WF.check_config(4096, 5)["blockdecimation"] == 5
    for n in (1, 2, 512, 1024, 2048, 4096, 65536, 3072):           # divisors and multiples of 1024
        assert WF.check_config(n)["blocklen"] == n
    for n in (0, -1024, 1536, 3, 1000, 4097):
        with pytest.raises(ValueError):
            WF.check_config(n)


def test_constructor_refuses_a_bad_block_length_before_device_use():
    with pytest.raises(ValueError):
        G.Waterfall(1536, 1e6, 4, 1, 0, -45, -20, 0, 0)


# ---- the model the GPU tests compare with (tests/waterfall_model.py) ---------------------------------------------------------------------
@pytest.mark.parametrize("levels", [(-45.0, -20.0), (-20.0, -45.0), (-30.0, -30.0), (511.0, -511.0)])
@pytest.mark.parametrize("loginput", [0, 1])
def test_near_edge_is_the_brute_force_distance_for_edges_in_either_order(loginput, levels):
    e = model_edges(loginput, *levels)
    rng = np.random.default_rng(4)
    lo, hi = min(e[0], e[-1]), max(e[0], e[-1])
    v = np.concatenate([rng.uniform(lo - 0.1 * abs(lo) - 1e-9, hi + 0.1 * abs(hi) + 1e-9, 4000), e[::7], e[::5] * (1 + 5e-6), e[::3] * (1 - 2e-5),
                        [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1.0]])
    with np.errstate(invalid="ignore"):
        d = np.abs(v[:, None] - e[None, :]).min(1)
        brute = d <= 1e-5 * np.maximum(np.abs(v), 1e-300)
    got = near_edge(v, e)
    assert np.array_equal(got, brute)
    assert got[4000:4000 + len(e[::7])].all() and not got[-3] and 0 < got.sum() < len(v)


def test_integer_levels_give_integer_edges():
    """loginput = 1, levels (-511, 511): linspace's step is exactly 1, the 1023 edges are the integers; the library's are the model's"""
    up = model_edges(1, -511, 511)
    assert np.array_equal(up, np.arange(-511.0, 512.0))
    assert np.array_equal(model_edges(1, 511, -511), up[::-1])
    assert np.array_equal(WF.edges(1, -511, 511), up) and np.array_equal(WF.edges(1, 511, -511), up[::-1])


def test_what_numpy_digitize_makes_of_ties_decreasing_and_constant_bins():
    """the rules the finish kernel follows: increasing bins count the edges <= x (NaN: all of them); decreasing bins the edges > x (NaN: none);
    constant bins are increasing; 1023 edges give indices 0 ... 1023"""
    up = model_edges(1, -511, 511)
    x = np.array([-512.0, -511.0, -510.5, 0.0, 510.5, 511.0, 600.0, np.inf, -np.inf, np.nan])
    assert colour_index(x, up).tolist() == [0, 1, 1, 512, 1022, 1023, 1023, 1023, 0, 1023]
    assert colour_index(x, up[::-1]).tolist() == [1023, 1022, 1022, 511, 1, 0, 0, 0, 1023, 0]
    flat = model_edges(1, -30, -30)
    assert np.all(flat == -30.0)
    assert colour_index([-31.0, np.nextafter(-30.0, -np.inf), -30.0, -29.0, np.nan, np.inf, -np.inf], flat).tolist() == [0, 0, 1023, 1023, 1023, 1023, 0]
    assert np.all(model_edges(0, -30, -30) == 10.0 ** -3.0)


def test_row_bound_is_the_suites_tolerance_at_13_bins():
    assert row_bound(13) <= 1e-6 < row_bound(14)
    assert row_bound(4) == 7 * 2.0 ** -24 and row_bound(16) == 19 * 2.0 ** -24
    # a float32 sum of n non-negative products pairs stays inside it: 200 draws at n = 4 and n = 16
    rng = np.random.default_rng(6)
    for n in (4, 16):
        z = (rng.standard_normal((200, n)) + 1j * rng.standard_normal((200, n))).astype(np.complex64)
        acc = np.zeros(200, np.float32)
        for j in range(n):
            acc = acc + (z.real[:, j] * z.real[:, j] + z.imag[:, j] * z.imag[:, j])
        exact = (z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2).sum(1)
        assert np.all(np.abs(acc - exact) <= row_bound(n) * exact)


def test_stream_rows_of_a_tone():
    """a tone on bin k of a block lands on shifted bin k + N / 2: pixel (k + N / 2) / (N / 1024), with the mean power 1 / (N / 1024)"""
    N, R, k = 4096, 4, 1000
    H = N - N // R
    x = np.exp(2j * np.pi * k * np.arange(3 * H) / N)
    rows = stream_rows(x, N, R)
    assert rows.shape == (3, 1024)
    pix = ((k + N // 2) % N) // 4
    assert np.all(rows[1:].argmax(1) == pix) and np.allclose(rows[1:, pix], 0.25) and np.allclose(rows[1:].sum(1), 0.25)


@pytest.mark.parametrize("N,R,nb,D,seed,reps", route_streams())
def test_route_streams_stay_under_the_cap_of_pixels_near_an_edge(N, R, nb, D, seed, reps):
    """the streams of tests/test_waterfall_routes_gpu.py, by the model alone: at most 1 % of the pixels lie within 1e-5 of an edge, and the
    pixels spread over many colours (the levels follow the noise power 2 / N)"""
    x = np.tile(noise_stream(nb * (N - N // R), seed), reps)
    rows = decimate(stream_rows(x, N, R), D)
    e = model_edges(0, *noise_levels(N))
    assert near_share(rows, e) <= NEAR_CAP
    idx = colour_index(rows, e)
    assert len(np.unique(idx)) >= 50 and np.mean((idx > 0) & (idx < 1023)) > 0.9


# ---- WaterfallImage: the reference's geometry, hand-computed ----------------------------------------------------------------------------
WHITE = (255, 255, 255)


def framed(img):
    """(row, pixel) of every pixel in the frame colour"""
    return set(map(tuple, np.argwhere(np.all(img.image == np.array(WHITE, np.uint8), axis=2))))


def test_rectangle_fully_inside_the_window():
    img = G.WaterfallImage(20)
    # rel_cfreq 0.25, rel_bw 0.0625: columns int(1024 * 0.21875) = 224 .. ceil(1024 * 0.28125) = 288
    img.msg({"blockstart": 5, "blockend": 9, "rel_cfreq": 0.25, "rel_bw": 0.0625})
    img.append(np.zeros((12, 1024, 3), np.uint8))          # max_block 12, min_block = -20 + 12 = -8
    # begin = 20 - ceil(12 - 5) = 13, end = 20 - int(12 - 9) = 17: verticals rows 13..16 at 224 and 288, horizontals rows 13 and 17 over 224..287
    want = {(r, c) for r in range(13, 17) for c in (224, 288)} | {(r, c) for r in (13, 17) for c in range(224, 288)}
    assert framed(img) == want
    assert img.pending == []


def test_rectangle_whose_begin_is_out_of_range():
    img = G.WaterfallImage(10)
    img.msg({"blockstart": 0, "blockend": 14, "rel_cfreq": 0.5, "rel_bw": 0.01})      # columns 506 .. 518
    img.append(np.zeros((16, 1024, 3), np.uint8))          # max_block 16, min_block = -10 + 16 = 6 >= blockstart
    # h line at 10 - max(int(16 - 14), 1) = 8 over 506..517; v line up from 10 - int(2) = 8: rows 4..7 at 506 and 518
    want = {(8, c) for c in range(506, 518)} | {(r, c) for r in range(4, 8) for c in (506, 518)}
    assert framed(img) == want
    assert img.pending == []


def test_rectangle_whose_end_is_not_yet_seen_is_kept():
    img = G.WaterfallImage(10)
    img.msg({"blockstart": 7, "blockend": 30, "rel_cfreq": 0.125, "rel_bw": 0.03125})  # columns 112 .. 144
    img.append(np.zeros((9, 1024, 3), np.uint8))           # max_block 9, min_block -1
    # h line at 10 - max(int(9 - 7), 1) = 8 over 112..143; v line down from 10 - int(9 - 30) = 31: nothing (31 is below the picture)
    want = {(8, c) for c in range(112, 144)}
    assert framed(img) == want
    assert len(img.pending) == 1                        # kept: its end may come


def test_pdus_without_geometry_are_ignored_and_rows_scroll_in():
    img = G.WaterfallImage(4)
    img.msg({"blockstart": 1})
    img.msg({"blockstart": 1, "blockend": 2, "rel_cfreq": -0.5, "rel_bw": 0.1})
    img.msg("not a dict")
    assert img.pending == []
    rows = np.arange(3 * 1024 * 3, dtype=np.uint32).astype(np.uint8).reshape(3, 1024, 3)
    img.append(rows[:2])
    img.append(rows[2:])
    assert np.array_equal(img.image[1:], rows) and not img.image[0].any()
    assert img.image.shape == (4, 1024, 3)
