"""CPU tests of the packed audio's definition (no GPU): tests/audio_pack_model.py against a double loop written out here, its two consequences (all
open: the matrix's bytes; the packed buffers of the calls of a stream, concatenated, are the stream's), and gr_fdc_amd.audio_pack_offsets /
unpack_audio against the model.  (The device against the model, in bytes: tests/test_audio_pack_gpu.py.)"""
import numpy as np
import pytest

import gr_fdc_amd as G
import audio_pack_model as M

NPBS = ([4, 8, 16, 8], [1], [3, 1, 7, 2, 5], [16] * 12)
DENSITIES = (0.5, 0.02, 1.0, 0.0)


def cases():
    for k, npb in enumerate(NPBS):
        for d in DENSITIES:
            for nb in (1, 2, 9):
                rng = np.random.default_rng(1000 * k + 10 * nb + int(100 * d))
                yield npb, (rng.random((nb, len(npb))) < d).astype(np.uint8)


def matrix(nb, npb, dtype, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(-30000, 30000, size=(nb, sum(npb)))
    return (a.astype(np.float32) / np.float32(7.0)).astype(dtype) if dtype == np.float32 else a.astype(dtype)


def test_offsets_equal_a_double_loop():
    for npb, mask in cases():
        off, count = M.offsets(mask, npb)
        run = 0
        for m in range(mask.shape[0]):
            for c in range(mask.shape[1]):
                assert off[m, c] == run
                run += int(mask[m, c]) * npb[c]
        assert count == run == int((mask.astype(np.int64) * np.array(npb)[None, :]).sum())
        off7, count7 = M.offsets(mask, npb, base=7)
        assert (off7 == off + 7).all() and count7 == count + 7


@pytest.mark.parametrize("dtype", (np.float32, np.int16))
def test_unpack_of_pack_round_trips(dtype):
    for npb, mask in cases():
        a = matrix(mask.shape[0], npb, dtype, seed=3)
        packed, count = M.pack(a, mask, npb)
        assert packed.dtype == dtype and packed.shape == (count,)
        per = M.unpack(packed, mask, npb)
        at = 0
        for c, n in enumerate(npb):
            want = a[mask[:, c] != 0, at:at + n].reshape(-1)
            assert per[c].tobytes() == want.tobytes() and per[c].size == int(mask[:, c].sum()) * n
            at += n


@pytest.mark.parametrize("dtype", (np.float32, np.int16))
def test_all_open_is_the_matrix(dtype):
    for npb in NPBS:
        a = matrix(5, npb, dtype, seed=4)
        packed, count = M.pack(a, np.ones((5, len(npb)), np.uint8), npb)
        assert count == a.size and packed.tobytes() == a.tobytes()
        packed, count = M.pack(a, np.zeros((5, len(npb)), np.uint8), npb)
        assert count == 0 and packed.size == 0


def test_every_cut_of_nine_rows_concatenates():
    npb = [4, 8, 16, 8]
    rng = np.random.default_rng(9)
    mask = (rng.random((9, 4)) < 0.5).astype(np.uint8)
    a = matrix(9, npb, np.float32, seed=5)
    whole, count = M.pack(a, mask, npb)
    assert 0 < count < a.size
    for bits in range(1 << 8):                                        # a cut behind row j where bit j is set: all 256 compositions of 9
        edges = [0] + [j + 1 for j in range(8) if (bits >> j) & 1] + [9]
        parts = [M.pack(a[lo:hi], mask[lo:hi], npb)[0] for lo, hi in zip(edges[:-1], edges[1:])]
        assert np.concatenate(parts).tobytes() == whole.tobytes(), edges


def test_the_package_helpers_agree_with_the_model():
    for npb, mask in cases():
        off, count = G.audio_pack_offsets(mask, npb)
        moff, mcount = M.offsets(mask, npb)
        assert off.dtype == np.int64 and off.shape == mask.shape and (off == moff).all() and count == mcount and isinstance(count, int)
        a = matrix(mask.shape[0], npb, np.int16, seed=6)
        packed, _n = M.pack(a, mask, npb)
        got, want = G.unpack_audio(packed, mask, npb), M.unpack(packed, mask, npb)
        assert len(got) == len(npb)
        for g, w in zip(got, want):
            assert g.dtype == np.int16 and g.ndim == 1 and g.tobytes() == w.tobytes()
    off, count = G.audio_pack_offsets(np.zeros((0, 3), np.uint8), [1, 2, 3])
    assert off.shape == (0, 3) and count == 0
    with pytest.raises(ValueError):
        G.audio_pack_offsets(np.ones((2, 3), np.uint8), [1, 2])
    with pytest.raises(ValueError):
        G.audio_pack_offsets(np.ones(3, np.uint8), [1, 2, 3])
    with pytest.raises(ValueError):
        G.unpack_audio(np.zeros(5, np.float32), np.ones((2, 2), np.uint8), [1, 2])        # six samples are open
