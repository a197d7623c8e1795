"""GPU tests (-m gpu) of the packed channel audio (fdc_pipeline_set_audio_packing and its kin; include/fdc_amd.h).

THE REFERENCE FOR BITS is tests/audio_pack_model.py fed with the GATED matrix and the mask of a SECOND handle with the same settings and the packing
off: the packed bytes, the count and the mask must equal the model's BYTE FOR BYTE, so no tolerance appears anywhere.  The streams, plans and
thresholds are those of tests/test_squelch_gpu.py (imported, not copied), 9 blocks, R = 2."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib
import audio_pack_model as M
import squelch_model as S
from footprint import DeviceBanded, twice
from test_demod_gpu import CYCLES, KW
from test_fine_tuning_gpu import BANK
from test_fine_tuning_routes_gpu import DeviceBuffers
from test_iq_input_gpu import EXAMPLE, same_bytes
from test_squelch_gpu import FORMATS, NB, PLANS, keyed, plan_ids, shows_everything, squelched, stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def taps_of(D, K):
    return G.lowpass_taps(D, K) if K > 1 else np.array([0.75], np.float32)


def audio_handle(k, hang, D, K, fmt="f32", scale=1.0, packed=False, thr=None, nb=NB, **kw):
    """a handle of plan k with the squelch (thr: (open, close), default the stream's), FM and the audio on, and the packing where asked"""
    _name, N, chans, flags = PLANS[k]
    _x, _power, thr_o, thr_c = stream(k)
    if thr is not None:
        thr_o, thr_c = thr
    p = squelched(N, chans, thr_o, thr_c, hang, nb=nb, flags=flags, **kw)
    p.set_demod("fm", CYCLES)
    p.set_audio(D, taps_of(D, K), fmt, scale)
    if packed:
        p.set_audio_packing(True)
    return p


def raw_packed(p, nb, capacity_elems, dtype, poison=0x5A):
    """fdc_pipeline_audio_packed into a poisoned buffer of the given capacity: (rc, count, the buffer as bytes)"""
    buf = np.full(capacity_elems * np.dtype(dtype).itemsize + 16, poison, np.uint8)
    count = C.c_int64(-1)
    rc = _lib.lib().fdc_pipeline_audio_packed(p._h, buf.ctypes.data, capacity_elems * np.dtype(dtype).itemsize, nb, C.byref(count))
    return rc, count.value, buf


# ---- 1. packed against the gated matrix -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hang", (0, 1, 3))
@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_packed_against_the_gated_matrix(k, hang):
    _name, N, chans, flags = PLANS[k]
    x, power, thr_o, thr_c = stream(k)
    whole, _s = S.squelch(power, None, thr_o, thr_c, hang)
    shows_everything(whole, power, thr_o, thr_c, "hang %d" % hang)
    for D, K in ((8, 64), (64, 1)) + (((1, 256),) if k == 0 else ()):
        for fmt, scale, dt in FORMATS:
            un, on = audio_handle(k, hang, D, K, fmt, scale), audio_handle(k, hang, D, K, fmt, scale, packed=True)
            assert not un.audio_packing() and on.audio_packing()
            un.work(x)
            outs = on.work(x)
            mask, mat = un.squelch(), un.audio()
            same_bytes(mask, whole, "the unpacked handle's mask")
            same_bytes(on.squelch(), mask, "the mask")
            npb = M.npb_of(on.lout, D)
            want, count = M.pack(mat, mask, npb)
            # no case passes by packing nothing or everything
            assert ((mask == 1).any(axis=0) & (mask == 0).any(axis=0)).all() and 0 < count < NB * sum(npb)
            got = on.audio_packed()
            assert got.dtype == dt and got.ndim == 1
            what = "%s D %d K %d hang %d" % (fmt, D, K, hang)
            print(what, "count", got.size, "of", NB * sum(npb))
            assert got.size == count, what
            same_bytes(got, want, what)
            for c, (a, b) in enumerate(zip(outs, M.unpack(want, mask, npb))):
                same_bytes(a, b, "what work() returns, ch%d, %s" % (c, what))
            assert "audio: pass, gated, packed" in on.describe() and "packed" not in un.describe() and "squelch: pass" in on.describe()


# ---- 2. all open and all closed --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_all_open_and_all_closed(k):
    _name, N, chans, flags = PLANS[k]
    x, _power, _o, _c = stream(k)
    D, K = 8, 64
    zero, huge = np.zeros(len(chans), np.float32), np.full(len(chans), 3e38, np.float32)
    for fmt, scale, dt in FORMATS:
        plain = G.Pipeline(N, 2, chans, max_blocks=NB, flags=flags)            # no squelch at all
        plain.set_demod("fm", CYCLES)
        plain.set_audio(D, taps_of(D, K), fmt, scale)
        plain.work(x)
        mat = plain.audio()
        assert np.count_nonzero(mat) > mat.size // 2
        on = audio_handle(k, 1, D, K, fmt, scale, packed=True, thr=(zero, zero))
        on.work(x)
        assert on.squelch().all()
        got = on.audio_packed()
        assert got.dtype == dt
        same_bytes(got, mat.reshape(-1), "all open, %s: the matrix's bytes" % fmt)
        off = audio_handle(k, 1, D, K, fmt, scale, packed=True, thr=(huge, huge))
        off.work(x)
        assert not off.squelch().any()
        assert off.audio_packed().shape == (0,)
        rc, count, buf = raw_packed(off, NB, 64, dt)
        assert rc == 0 and count == 0 and (buf == 0x5A).all(), "all closed: the getter leaves dst untouched"
        assert all(o.size == 0 for o in off.work(x))


# ---- 3. cuts of the stream ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(PLANS)), ids=plan_ids)
def test_cuts_of_the_stream_concatenate(k):
    _name, N, chans, flags = PLANS[k]
    H = N - N // 2
    x, power, thr_o, thr_c = stream(k)
    D, K, hang = 8, 64, 1
    un = audio_handle(k, hang, D, K)
    un.work(x)
    mask = un.squelch()
    shows_everything(mask, power, thr_o, thr_c, "hang 1")
    npb = M.npb_of(un.lout, D)
    whole, count = M.pack(un.audio(), mask, npb)
    assert 0 < count < NB * sum(npb)
    for cut in ((9,), (4, 5), (1, 1, 7), (3, 3, 3)):
        p = audio_handle(k, hang, D, K, packed=True)
        parts, b0 = [], 0
        for n in cut:
            p.work(x[b0 * H:(b0 + n) * H])
            same_bytes(p.squelch(), mask[b0:b0 + n], "cut %r: the mask at %d" % (cut, b0))
            parts.append(p.audio_packed())
            assert parts[-1].size == M.offsets(mask[b0:b0 + n], npb)[1], "cut %r: the offsets start at 0 in every call" % (cut,)
            b0 += n
        same_bytes(np.concatenate(parts), whole, "cut %r" % (cut,))
    for kw in (dict(host_sub_blocks=2), dict(chunk_blocks=2), dict(chunk_blocks=2, host_sub_blocks=3)):
        p = audio_handle(k, hang, D, K, packed=True, **kw)
        p.work(x)
        same_bytes(p.squelch(), mask, repr(kw))
        same_bytes(p.audio_packed(), whole, repr(kw))
        p.work(x[:4 * H])                                                   # a stream that starts elsewhere: still from 0, still what the mask says
        m2 = p.squelch()
        assert p.audio_packed().size == M.offsets(m2, npb)[1]


# ---- 4. the offsets alone ---------------------------------------------------------------------------------------------------------------------------------

# The sizes at which the offsets kernels take another path (csrc/fdc_postpass.hip): k_pack_scan gives a lane kPackPer = 4 consecutive rows (3, 4, 5), a
# wave 256 (255 .. 257), a trip of the workgroup 1024 (1023 .. 1025; two trips: 2047 .. 2049; four: 4095 .. 4097); k_pack_rows takes 256 rows per
# workgroup where a lane walks a row (up to kPackSerial = 8 channels) and 4 rows (a wave each) above that, 64 channels per trip of the wave: the bank has
# exactly 64, and the two tables of 63 and 65 channels (not the issue's: added for the partial and the second trip) stand on either side.  The cap of
# the grid, 65536 workgroups, is not reached below 262144 blocks and is not tested.
OFFSET_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
RAGGED = lambda n: [(200 * c, 256 if c % 3 else 128, 0.8, 1.0) for c in range(n)]
TABLES = [("example", 4096, EXAMPLE, OFFSET_COUNTS), ("bank", 16384, BANK, OFFSET_COUNTS), ("63 ragged", 16384, RAGGED(63), (1, 5, 257, 1025)),
          ("65 ragged", 16384, RAGGED(65), (1, 5, 257, 1025)), ("8 ragged", 4096, RAGGED(8), (1, 257, 1025)), ("9 ragged", 4096, RAGGED(9), (1, 257, 1025))]


def hand_masks(nb, Cn, seed):
    rng = np.random.default_rng(seed)
    first, last = np.zeros((nb, Cn), np.uint8), np.zeros((nb, Cn), np.uint8)
    first[0, 0] = 1
    last[-1, -1] = 1
    return [("density 0.5", (rng.random((nb, Cn)) < 0.5).astype(np.uint8)), ("density 0.02", (rng.random((nb, Cn)) < 0.02).astype(np.uint8)),
            ("all ones", np.ones((nb, Cn), np.uint8)), ("all zeros", np.zeros((nb, Cn), np.uint8)), ("the first cell", first), ("the last cell", last)]


@pytest.mark.parametrize("t", range(len(TABLES)), ids=[t[0] for t in TABLES])
def test_offsets_alone(t):
    """fdc_pipeline_audio_pack_offsets_device on hand-made masks against numpy cumsums, d_off and the total between poisoned guards: exactly nblocks C
    words and 8 bytes change.  A mask byte that is not 0 or 1 counts as open"""
    _name, N, chans, counts = TABLES[t]
    D = 8
    p = G.Pipeline(N, 2, chans, max_blocks=4)
    p.set_demod("fm", CYCLES)
    p.set_audio(D, taps_of(D, 8))
    Cn, npb = len(chans), np.array(M.npb_of(p.lout, D), np.int64)
    assert len(set(npb.tolist())) > 1 or t == 1                       # ragged widths (the bank's are uniform)
    seen = set()
    with DeviceBuffers() as dev:
        d_base = dev.put(np.array([123456789], np.int64))
        for nb in counts:
            band = DeviceBanded(dev, [4 * nb * Cn, 8], 4 * Cn)
            for name, mask in hand_masks(nb, Cn, 100 * t + nb):
                w = (mask != 0).astype(np.int64).reshape(-1) * np.tile(npb, nb)
                end = np.cumsum(w)
                d_mask = dev.put(mask if name != "density 0.5" else (mask * 0x81).astype(np.uint8))
                for base, d_b in ((0, None), (123456789, d_base)):
                    want_off, want_total = (end - w + base).astype(np.uint32).reshape(nb, Cn), np.array([end[-1] + base], np.int64)
                    for poison in twice(band):
                        p.audio_pack_offsets_device(d_mask, band.ptr(0), band.ptr(1), nb, d_b)
                        p.synchronize()
                        band.check([want_off, want_total], "%s, %d blocks, %s, base %d" % (_name, nb, name, base))
                    seen.add((name, base != 0))
                same_bytes(dev.get(d_mask, nb * Cn, np.uint8), (mask if name != "density 0.5" else (mask * 0x81).astype(np.uint8)).reshape(-1), "the mask is read only")
            same_bytes(dev.get(d_base, 1, np.int64), np.array([123456789], np.int64), "the base is read only")
        # the total may be the base's own word (the running total of a host call's sub-batches)
        mask = hand_masks(257, Cn, 5)[0][1]
        d_mask, d_run = dev.put(mask), dev.put(np.array([1000], np.int64))
        d_off = dev.put(np.zeros(257 * Cn, np.uint32))
        p.audio_pack_offsets_device(d_mask, d_off, d_run, 257, d_run)
        p.synchronize()
        off, count = M.offsets(mask, npb, base=1000)
        same_bytes(dev.get(d_off, 257 * Cn, np.uint32).reshape(257, Cn), off.astype(np.uint32), "base and total in one word: the offsets")
        assert int(dev.get(d_run, 1, np.int64)[0]) == count
    assert len(seen) == 12
    lib = _lib.lib()
    assert lib.fdc_pipeline_audio_pack_offsets_device(p._h, None, None, 1, 1, 1, None) == -1 and lib.fdc_pipeline_audio_pack_offsets_device(p._h, 1, None, None, 1, 1, None) == -1
    assert lib.fdc_pipeline_audio_pack_offsets_device(p._h, 1, None, 1, None, 1, None) == -1 and lib.fdc_pipeline_audio_pack_offsets_device(p._h, 1, None, 1, 1, -1, None) == -1
    assert lib.fdc_pipeline_audio_pack_offsets_device(p._h, None, None, None, None, 0, None) == 0
    p.set_audio(None)
    assert lib.fdc_pipeline_audio_pack_offsets_device(p._h, 1, None, 1, 1, 1, None) == -1         # no decimation to size the cells by


# ---- 5. footprint of the PACK pass -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (0, 2), ids=[plan_ids[0], plan_ids[2]])
def test_footprint_of_the_packed_pass(k):
    """fdc_pipeline_audio_pass_device with the packing on, into poisoned buffers: exactly the first `count` elements change, the history buffer is written
    as it is ungated, the history that is read and every guard byte stay"""
    _name, N, chans, flags = PLANS[k]
    x, power, thr_o, thr_c = stream(k)
    Cn, D, K = len(chans), 8, 64
    un = squelched(N, chans, thr_o, thr_c, 1, flags=flags)
    un.set_demod("fm", CYCLES)
    ports = un.work(x)                                               # the demodulated ports, per channel
    un.set_audio(D, taps_of(D, K))
    un.reset()
    un.work(x)
    on = audio_handle(k, 1, D, K, packed=True)
    on.work(x)
    mask = on.squelch()
    same_bytes(mask, un.squelch(), "the mask")
    npb = M.npb_of(on.lout, D)
    hist_in = (np.arange(Cn * (K - 1), dtype=np.float32) % 17 - 8) / np.float32(64)
    flat = np.zeros(on.output_samples(NB), np.float32)
    for c, w in enumerate(ports):
        flat[on.channel_offset(c, NB):on.channel_offset(c, NB) + NB * on.lout[c]] = w
    hist = np.concatenate([w[-(K - 1):] for w in ports]).astype(np.float32)
    row = sum(npb)
    with DeviceBuffers() as dev:
        d_in = dev.put(flat)
        # what the gated pass gives with this history in front: the reference matrix for the packed pass over the same inputs
        d_ref, d_h2 = dev.put(np.zeros(NB * row, np.float32)), dev.put(np.zeros(Cn * (K - 1), np.float32))
        d_hin = dev.put(hist_in)
        un.audio_pass_device(d_in, d_ref, NB, d_hin, d_h2)
        un.synchronize()
        want, count = M.pack(dev.get(d_ref, NB * row, np.float32).reshape(NB, row), mask, npb)
        assert 0 < count < NB * row
        # (the output payload is count elements long: an element more would land in the guard behind it)
        band = DeviceBanded(dev, [4 * count, 4 * Cn * (K - 1), 4 * Cn * (K - 1)], 4 * row)
        for poison in twice(band):
            assert dev.hip.hipMemcpy(band.ptr(2), C.c_void_p(hist_in.ctypes.data), C.c_size_t(hist_in.nbytes), 1) == 0
            on.audio_pass_device(d_in, band.ptr(0), NB, band.ptr(2), band.ptr(1))
            on.synchronize()
            band.check([want, hist, hist_in], "the packed audio pass")
        lib = _lib.lib()
        assert lib.fdc_pipeline_audio_pass_device(on._h, d_in, band.ptr(0), None, band.ptr(1), NB - 1, None) == -1     # not that call's block count


def test_footprint_of_the_packed_pass_on_the_spectrum_path():
    """the third plan of the squelch footprint tests' set: the example plan on the spectrum path, the packed pass into one poisoned buffer"""
    k = 1
    _name, N, chans, flags = PLANS[k]
    x, _power, _o, _c = stream(k)
    Cn, D, K = len(chans), 8, 64
    un, on = audio_handle(k, 1, D, K), audio_handle(k, 1, D, K, packed=True)
    un.work(x)
    on.work(x)
    mask = on.squelch()
    npb, row = M.npb_of(on.lout, D), sum(M.npb_of(on.lout, D))
    want, count = M.pack(un.audio(), mask, npb)
    dm = G.Pipeline(N, 2, chans, max_blocks=NB, flags=flags)
    dm.set_demod("fm", CYCLES)
    ports = dm.work(x)
    flat = np.zeros(on.output_samples(NB), np.float32)
    for c, w in enumerate(ports):
        flat[on.channel_offset(c, NB):on.channel_offset(c, NB) + NB * on.lout[c]] = w
    hist = np.concatenate([w[-(K - 1):] for w in ports]).astype(np.float32)
    with DeviceBuffers() as dev:
        d_in = dev.put(flat)
        band = DeviceBanded(dev, [4 * NB * row, 4 * Cn * (K - 1)], 4 * row)
        for poison in twice(band):
            on.audio_pass_device(d_in, band.ptr(0), NB, None, band.ptr(1))
            on.synchronize()
            band.check([np.concatenate([want.view(np.uint8), np.full(4 * (NB * row - count), poison, np.uint8)]), hist], "the packed pass, zeros in front")


# ---- 6. the setting ---------------------------------------------------------------------------------------------------------------------------------------

def test_setting_semantics():
    _name, N, chans, flags = PLANS[0]
    H = N - N // 2
    x, power, thr_o, thr_c = stream(0)
    lib = _lib.lib()
    D, K = 8, 64
    taps = taps_of(D, K)
    p = G.Pipeline(N, 2, chans, max_blocks=NB)
    # off by default; refused unless both the audio and the squelch are on
    assert p.audio_packing() is False and lib.fdc_pipeline_audio_packing(p._h) == 0
    for step in (lambda: None, lambda: p.set_levels(True), lambda: p.set_squelch(thr_o, thr_c, 1), lambda: p.set_demod("fm", CYCLES)):
        step()
        with pytest.raises(G.FdcError) as e:
            p.set_audio_packing(True)
        assert e.value.status == -1 and "switch both on first" in str(e.value) and not p.audio_packing()
    p.set_audio(D, taps)
    p.set_squelch(None)
    with pytest.raises(G.FdcError):
        p.set_audio_packing(True)                                     # the audio alone
    p.set_squelch(thr_o, thr_c, 1)
    p.set_audio_packing(False)                                        # off while off: accepted
    # the unpacked reference, and the describe string with the packing off
    p.work(x)
    mat, mask, desc = p.audio(), p.squelch(), p.describe()
    npb = M.npb_of(p.lout, D)
    want, count = M.pack(mat, mask, npb)
    assert "audio: pass, gated" in desc and "packed" not in desc
    p.set_audio_packing(True)
    assert p.audio_packing() and lib.fdc_pipeline_audio_packing(p._h) == 1
    # a switch leaves nothing to fetch until the next call
    c64 = C.c_int64(-5)
    assert lib.fdc_pipeline_audio_packed(p._h, None, 0, NB, C.byref(c64)) == -1 and c64.value == -5
    p.reset()
    assert p.audio_packing()                                          # the setting survives reset()
    p.work(x)
    same_bytes(p.audio_packed(), want, "switched on")
    assert p.describe() == desc.replace("audio: pass, gated", "audio: pass, gated, packed")
    # the matrix getter is refused, by Python and by the library
    with pytest.raises(ValueError):
        p.audio()
    buf = np.full(mat.nbytes, 0xA5, np.uint8)
    assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, buf.nbytes, NB) == -1 and (buf == 0xA5).all() and "packing" in lib.fdc_last_error().decode()
    # while it is on the audio and the squelch cannot be switched off
    with pytest.raises(G.FdcError) as e:
        p.set_audio(None)
    assert "packing" in str(e.value) and p.audio_setting() is not None
    with pytest.raises(G.FdcError) as e:
        p.set_squelch(None)
    assert "packing" in str(e.value) and p.squelch_setting() is not None
    # the getter's capacity rule, the count query, a wrong block count
    rc, n, buf = raw_packed(p, NB, count - 1, np.float32)
    assert rc == -1 and n == count and (buf == 0x5A).all(), "capacity below count: refused, nothing written, the count set"
    rc, n, buf = raw_packed(p, NB, 0, np.float32)
    assert rc == -1 and n == count and (buf == 0x5A).all()
    c64 = C.c_int64(-5)
    assert lib.fdc_pipeline_audio_packed(p._h, None, 0, NB, C.byref(c64)) == 0 and c64.value == count       # dst NULL: a query
    assert lib.fdc_pipeline_audio_packed(p._h, None, 0, NB, None) == -1
    for nb in (NB - 1, NB + 1, 0):
        c64 = C.c_int64(-5)
        rc = lib.fdc_pipeline_audio_packed(p._h, buf.ctypes.data, 4 * count, nb, C.byref(c64))
        assert rc == -1 and c64.value == -5 and (buf == 0x5A).all(), nb
    rc, n, buf = raw_packed(p, NB, count, np.float32)
    assert rc == 0 and n == count and (buf[4 * count:] == 0x5A).all()
    same_bytes(buf[:4 * count].view(np.float32), want, "the raw getter")
    # a new format, decimation or taps is allowed and leaves nothing to fetch until the next call
    p.set_audio(D, taps, "s16", 9000.0)
    assert p.audio_packing()
    c64 = C.c_int64(-5)
    assert lib.fdc_pipeline_audio_packed(p._h, None, 0, NB, C.byref(c64)) == -1 and c64.value == -5
    with pytest.raises(G.FdcError):
        p.audio_pass_device(1, 1, NB, None, 1)                        # ... nor offsets for the pass alone
    p.set_audio(4, taps_of(4, 32), "s16", 9000.0)
    p.reset()
    p.work(x)
    ref = audio_handle(0, 1, 4, 32, "s16", 9000.0)
    ref.work(x)
    same_bytes(p.audio_packed(), M.pack(ref.audio(), mask, M.npb_of(p.lout, 4))[0], "a new decimation, taps and format")
    # off again: the matrix bytes and the describe string are back
    p.set_audio(D, taps)
    p.set_audio_packing(False)
    assert not p.audio_packing()
    with pytest.raises(ValueError):
        p.audio_packed()
    assert lib.fdc_pipeline_audio(p._h, buf.ctypes.data, mat.nbytes, NB) == -1       # the last call's audio was packed: nothing to fetch as a matrix
    p.reset()
    p.work(x)
    same_bytes(p.audio(), mat, "switched off again: the matrix")
    assert p.describe() == desc
    p.set_squelch(None)                                               # ... and the squelch may go
    p.set_squelch(thr_o, thr_c, 1)
    # a call above max_blocks is refused as ever, and leaves the last result in place
    p.set_audio_packing(True)
    p.reset()
    p.work(x[:4 * H])
    first = p.audio_packed()
    with pytest.raises(G.FdcError):
        p.work(np.zeros((NB + 1) * H, np.complex64))
    same_bytes(p.audio_packed(4), first, "behind a refused call")
    # a plan without channels accepts it
    z = G.Pipeline(N, 2, [], max_blocks=3, keep_spectrum=True)
    z.set_levels(True)
    z.set_squelch(1.0, 0.5, 2)
    z.set_demod("fm", CYCLES)
    z.set_audio(D, taps)
    z.set_audio_packing(True)
    z.work(x[:3 * H])
    assert z.audio_packing() and z.audio_packed().shape == (0,) and "packed" not in z.describe()
    z.set_audio_packing(False)


# (The refusal of max_blocks A >= 2^32 is not reached here: the audio's own buffers, which the setter needs first, would take 16 GiB on the device and
# as much pinned memory.)


def test_refused_while_a_pipelined_sinks_batch_is_inside():
    from test_demod_gpu import SINKS_KW
    N, R, nb = 4096, 2, 3
    H = N - N // R
    x, _power, _o, _c = stream(0)
    p = G.Pipeline(N, R, EXAMPLE, max_blocks=nb, keep_spectrum=True)
    bank = G.Sinks(N, R, lookahead=True, max_blocks=nb, **SINKS_KW)
    p.work(x[:nb * H], sinks=bank)
    for on in (True, False):
        with pytest.raises(G.FdcError) as e:
            p.set_audio_packing(on)
        assert e.value.status == -1 and "sinks" in str(e.value)
    while p.flush_sinks(bank) > 0:
        pass
    p.set_audio_packing(False)


# ---- 7. the device entry -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (0, 2), ids=[plan_ids[0], plan_ids[2]])
def test_device_entry(k):
    _name, N, chans, flags = PLANS[k]
    H = N - N // 2
    x, power, thr_o, thr_c = stream(k)
    D, K = 8, 64
    un, on = audio_handle(k, 1, D, K), audio_handle(k, 1, D, K, packed=True)
    npb = M.npb_of(on.lout, D)
    ring = np.concatenate([np.zeros(N // 2, np.complex64), x])
    with DeviceBuffers() as dev:
        d_in = dev.put(ring)
        for first, n in ((0, NB), (0, 4), (4, 5), (2, 3)):
            res = []
            for h in (un, on):
                d_o = dev.put(np.zeros(h.output_samples(n), np.float32))
                h.process_device(C.c_void_p(d_in.value + 8 * first * H), first, n, d_o)
                h.synchronize()
                res.append(dev.get(d_o, h.output_samples(n), np.float32))
            same_bytes(res[1], res[0], "d_out of the device entry at %d" % first)
            mask = un.squelch(n)
            same_bytes(on.squelch(n), mask, "the mask at %d" % first)
            want, count = M.pack(un.audio(n), mask, npb)
            got = on.audio_packed(n)
            same_bytes(got, want, "audio_packed after the device entry at %d" % first)
            same_bytes(dev.get(C.c_void_p(on.audio_device()), count, np.float32), want, "audio_device(): its first count elements")
            assert 0 < count < n * sum(npb) or n < NB
        assert "packed" in on.describe()
        d_o = dev.put(np.zeros(on.output_samples(NB + 1), np.float32))
        with pytest.raises(G.FdcError):
            on.process_device(d_in, 0, NB + 1, d_o)                   # above max_blocks: refused as now
        same_bytes(on.audio_packed(3), got, "behind the refused call")


# ---- 8. no allocation in the steady state -----------------------------------------------------------------------------------------------------------------

NO_ALLOC_CHILD = r'''
import ctypes as C, sys
import numpy as np
shim = C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL)
sys.path.insert(0, sys.argv[2])
import gr_fdc_amd as G

def counts():
    v = (C.c_long * 4)()
    shim.fdc_test_alloc_counts(v)
    return list(v)

hip = C.CDLL("libamdhip64.so")
N, R, nb = 4096, 2, 8
H = N - N // R
rng = np.random.default_rng(3)
x = (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H)).astype(np.complex64)
x[3 * H:5 * H] *= 1e-3
EXAMPLE = [(100, 256, 0.8, 1.0), (700, 512, 0.75, 0.95), (1500, 1024, 0.8, 1.0), (3001, 512, 0.6, 0.9)]
taps = G.lowpass_taps(8, 64)
hs = [G.Pipeline(N, R, EXAMPLE, max_blocks=nb), G.Pipeline(N, R, EXAMPLE, max_blocks=nb, host_sub_blocks=3), G.Pipeline(N, R, EXAMPLE, max_blocks=nb)]
for h in hs:
    h.set_levels(True)
    h.set_squelch(300.0, 100.0, 0)
    h.set_demod("fm", 0.5)
    h.set_audio(8, taps)
    h.set_audio_packing(True)
p, ps, pd = hs
p.work(x)
thr = (p.levels()[:, :, 0].max(axis=0) * 1e-3).astype(np.float32)      # between the loud blocks and the quiet ones
for h in hs:
    h.set_squelch(thr, thr, 0)
d_ring, d_out, d_mask, d_off, d_tot = (C.c_void_p() for _ in range(5))
assert hip.hipMalloc(C.byref(d_ring), C.c_size_t(8 * (N // R + nb * H))) == 0
assert hip.hipMemcpy(C.c_void_p(d_ring.value + 8 * (N // R)), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0
assert hip.hipMalloc(C.byref(d_out), C.c_size_t(8 * pd.output_samples(nb))) == 0
assert hip.hipMalloc(C.byref(d_mask), C.c_size_t(4 * nb)) == 0 and hip.hipMemset(d_mask, 1, C.c_size_t(4 * nb)) == 0
assert hip.hipMalloc(C.byref(d_off), C.c_size_t(16 * nb)) == 0 and hip.hipMalloc(C.byref(d_tot), C.c_size_t(8)) == 0
blk = [0]

def device():
    pd.process_device(d_ring, blk[0], nb, d_out)
    blk[0] += nb
    pd.synchronize()
    return pd.audio_packed(nb).size

def offsets():
    pd.audio_pack_offsets_device(d_mask, d_off, d_tot, nb)
    pd.synchronize()

entries = {"fdc_pipeline_work (packed)": lambda: (p.work(x), p.audio_packed()),
           "fdc_pipeline_work (packed, sub-batches)": lambda: (ps.work(x), ps.audio_packed()),
           "fdc_pipeline_process_device and fdc_pipeline_audio_packed": device,
           "fdc_pipeline_audio_pack_offsets_device": offsets,
           "fdc_pipeline_set_audio_packing off and on again": lambda: (p.set_audio_packing(False), p.work(x), p.set_audio_packing(True), p.work(x))}
bad = []
for name, call in entries.items():
    for _ in range(3):
        call()
    before = counts()
    for _ in range(30):
        call()
    after = counts()
    print(name, [a - b for a, b in zip(after, before)])
    if after != before:
        bad.append((name, [a - b for a, b in zip(after, before)]))
m = p.squelch()
assert m.any() and not m.all(), m.tolist()
assert 0 < p.audio_packed().size < nb * 144 and p.audio_packed().tobytes() == ps.audio_packed().tobytes()
assert "packed" in p.describe() and "packed" in ps.describe() and "packed" in pd.describe(), (p.describe(), ps.describe(), pd.describe())
assert not bad, bad
print("OK")
'''


def test_no_allocation_in_the_steady_state(tmp_path):
    shim = str(tmp_path / "libhipcount.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hip_alloc_counter.c"), "-o", shim,
                           "-ldl", "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([sys.executable, "-c", NO_ALLOC_CHILD, shim, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


# ---- 9. the hier block -------------------------------------------------------------------------------------------------------------------------------------

def test_hier_block():
    N, R, nb, D = 4096, 2, 6, 4
    H = N - N // R
    ref = G.FrequencyDomainChannelizer(inptype=8, levels=True, **KW)
    chans = [(f, l, p, s) for (f, l, _lo, p, s) in ref.channel_params]
    x = keyed(N, R, chans, nb=2 * nb, seed=21)
    ref.work(x[:nb * H])
    la = ref.levels
    ref.work(x[nb * H:])
    lev = np.concatenate([la, ref.levels])[:, :, 0]
    top_db = 10.0 * np.log10(lev.max(axis=0) / np.array(ref.pipeline.lout, np.float64))
    kw = dict(KW, levels=True, demod="fm", demod_gain=CYCLES, audio_decim=D, audio_taps=G.lowpass_taps(D, 33), squelch_db=top_db - 5.0,
              squelch_close_db=top_db - 15.0, squelch_hang=1)
    gated = G.FrequencyDomainChannelizer(inptype=8, **kw)
    packed = G.FrequencyDomainChannelizer(inptype=8, audio_packed=True, **kw)
    assert packed.audio_packed is True and gated.audio_packed is False and packed.pipeline.audio_packing() and not gated.pipeline.audio_packing()
    npb = M.npb_of(packed.pipeline.lout, D)
    for j in range(2):
        a, b = gated.work(x[j * nb * H:(j + 1) * nb * H]), packed.work(x[j * nb * H:(j + 1) * nb * H])
        same_bytes(packed.squelch, gated.squelch, "hier block, call %d: the mask" % j)
        m = packed.squelch
        assert m.any() and not m.all()
        for c in range(len(npb)):
            keep = np.repeat(m[:, c] != 0, npb[c])
            same_bytes(b[c], a[c][keep], "hier block, call %d, ch%d: the open blocks of the gated audio" % (j, c))
    res = packed.work(x[:0])
    assert [r.size for r in res] == [0, 0, 0] and packed.squelch.shape == (0, 3)
