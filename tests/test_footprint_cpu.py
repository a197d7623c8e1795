"""The footprint checker (tests/footprint.py) on the CPU: "kernels" are numpy writes into a host Banded region.  It must accept an exact write and fail,
with the right offsets in its message, on every kind of miss the GPU tests (tests/test_footprint_gpu.py) are there to catch; nothing on the GPU is ever
broken to see those fail."""
import re

import numpy as np
import pytest

import footprint as F

BLOCK = 3 * 1000            # the bytes of one block of the simulated buffer (1500 sc8 samples)
NB = 4


def expected_bytes(seed=1):
    e = np.random.default_rng(seed).integers(0, 256, NB * BLOCK, dtype=np.int64).astype(np.uint8)
    e[e == F.POISONS[0]] = 7        # (the cases below place the poison values themselves)
    e[e == F.POISONS[1]] = 7
    return e


def run(kernel, expected, sizes=None):
    """one case as the GPU tests run it: under both poison bytes; returns the messages of the checks that failed, by poison byte"""
    band = F.HostBanded(sizes or [expected.size], BLOCK)
    failed = {}
    for byte in F.POISONS:
        band.fill(byte)
        kernel(band)
        try:
            band.check(expected, "case")
        except AssertionError as err:
            failed[byte] = str(err)
    return failed


def exact(band):
    band.view(0, np.uint8)[:] = expected_bytes()


def test_the_layout_holds_the_conditions_of_the_method():
    for sizes, block in (([1], 1), ([12000], 3000), ([100, 0, 70000, 255, 256, 257], 70001), ([8 * 5 * 131072], 8 * 131072)):
        b = F.HostBanded(sizes, block)
        assert b.guard >= max(block, 64 * 1024) and b.guard % 256 == 0
        ends = [s + n for s, n in zip(b.starts, b.sizes)]
        assert b.starts[0] == b.guard and b.total - ends[-1] >= b.guard
        assert all(s % 256 == 0 for s in b.starts) and all(nxt - e >= b.guard for e, nxt in zip(ends, b.starts[1:]))
        assert b.view(0, np.uint8).ctypes.data % 256 == 0
    assert F.guard_bytes(1) == 65536 and F.guard_bytes(65537) == 65792 and F.guard_bytes(8 * 131072) == 8 * 131072
    assert F.POISONS == (0xA5, 0x5A)


def test_an_exact_write_passes_under_both_poison_bytes():
    assert run(exact, expected_bytes()) == {}
    band = F.HostBanded([NB * BLOCK], BLOCK)
    n = 0
    for byte in F.twice(band):
        assert band.mem.min() == band.mem.max() == byte
        exact(band)
        band.check(expected_bytes())
        n += 1
    assert n == 2 and band.checked == set(F.POISONS)


def test_twice_refuses_a_body_that_does_not_check():
    band = F.HostBanded([NB * BLOCK], BLOCK)
    with pytest.raises(AssertionError, match="not checked under poison 0xA5"):
        for _byte in F.twice(band):
            exact(band)


def test_an_unwritten_byte_that_equals_the_expected_one_under_one_poison():
    """byte 4321 is never written and its expected value is 0xA5: the run under 0xA5 cannot see it, the run under 0x5A does"""
    e = expected_bytes()
    e[4321] = 0xA5

    def kernel(band):
        v = band.view(0, np.uint8)
        v[:4321] = e[:4321]
        v[4322:] = e[4322:]
    failed = run(kernel, e)
    assert list(failed) == [0x5A], failed
    assert "payload 0: 1 of 12000 bytes differ" in failed[0x5A] and "first at offset 4321, last at offset 4321 (1 of them still hold the poison" in failed[0x5A]
    assert "poison 0x5A" in failed[0x5A] and "guard" not in failed[0x5A]


def test_an_unwritten_sample_at_the_end():
    """the last sc8 sample (two bytes) of the payload is skipped: both runs fail at offsets 11998 and 11999"""
    e = expected_bytes()

    def kernel(band):
        band.view(0, np.uint8)[:-2] = e[:-2]
    failed = run(kernel, e)
    assert sorted(failed) == sorted(F.POISONS)
    for msg in failed.values():
        assert "2 of 12000 bytes differ" in msg and "first at offset 11998, last at offset 11999 (2 of them still hold the poison byte: unwritten)" in msg


def test_a_byte_in_the_front_guard():
    e = expected_bytes()

    def kernel(band):
        exact(band)
        band.mem[band.starts[0] - 16] = 0
    failed = run(kernel, e)
    assert sorted(failed) == sorted(F.POISONS)
    for msg in failed.values():
        assert "payload 0: 1 guard bytes written, first at offset -16, last at offset -16" in msg and "differ" not in msg


def test_a_byte_in_the_back_guard():
    e = expected_bytes()

    def kernel(band):
        exact(band)
        band.mem[band.starts[0] + e.size + 8] = 0x33
    failed = run(kernel, e)
    assert sorted(failed) == sorted(F.POISONS)
    for msg in failed.values():
        assert "payload 0: 1 guard bytes written, first at offset 12008, last at offset 12008 (the payload is bytes 0 to 11999)" in msg


def test_a_whole_extra_block_behind_the_payload():
    """a call that stores NB + 1 blocks: the fifth lands in the back guard, which is at least one block long, so all of it is seen.  The block holds the
    poison values too (as real samples may): those bytes are the ones the other run sees."""
    e = expected_bytes()
    extra = expected_bytes(2)[:BLOCK].copy()
    extra[10], extra[11] = F.POISONS

    def kernel(band):
        exact(band)
        s = band.starts[0] + e.size
        band.mem[s:s + BLOCK] = extra
    failed = run(kernel, e)
    assert sorted(failed) == sorted(F.POISONS)
    for byte, msg in failed.items():
        m = re.search(r"payload 0: (\d+) guard bytes written, first at offset (\d+), last at offset (\d+)", msg)
        assert m, msg
        assert [int(v) for v in m.groups()] == [BLOCK - 1, e.size, e.size + BLOCK - 1], msg


def test_guards_between_the_channels_of_a_host_call():
    """three payloads (the outs[c] of a host entry): a store one sample past channel 1 is reported against channel 1, one in front of channel 2 too
    (the guard belongs to the payload in front of it), and a short channel 0 as unwritten"""
    sizes = [4000, 300, 8000]
    e = [expected_bytes(3)[:n] for n in sizes]

    def kernel(band):
        band.view(0, np.uint8)[:3992] = e[0][:3992]
        band.view(1, np.uint8)[:] = e[1]
        band.view(2, np.uint8)[:] = e[2]
        band.mem[band.starts[1] + 300:band.starts[1] + 308] = 1
        band.mem[band.starts[2] - 8:band.starts[2]] = 1
    failed = run(kernel, e, sizes)
    assert sorted(failed) == sorted(F.POISONS)
    for msg in failed.values():
        assert "payload 0: 8 of 4000 bytes differ from the expected ones, first at offset 3992, last at offset 3999 (8 of them" in msg
        back = F.HostBanded(sizes, BLOCK)
        assert "payload 1: 16 guard bytes written, first at offset 300, last at offset %d" % (back.starts[2] - back.starts[1] - 1) in msg
        assert "payload 2" not in msg


def test_ring_surrounds():
    for ring, block in ((np.arange(1000, dtype=np.float32).view(np.complex64), 100), (np.arange(-500, 500, dtype=np.int16), 200),
                        (np.arange(-128, 128, dtype=np.int8), 64), (np.arange(300, dtype=np.float32), 100)):
        whole, start = F.ring_surround(ring, block)
        item = ring.dtype.itemsize
        assert (start * item) % 256 == 0 and start * item >= max(65536, block * item) and (whole.size - start - ring.size) * item >= max(65536, block * item)
        assert np.array_equal(whole[start:start + ring.size], ring)
        around = np.concatenate([whole[:start], whole[start + ring.size:]])
        if ring.dtype.kind == "i":
            assert (around == np.iinfo(ring.dtype).min).all()
        else:
            assert np.isnan(around.view(np.float32)).all()
        h = F.HostRing(ring, block)
        assert np.array_equal(h.ring, ring) and h.ring.ctypes.data % 256 == 0
        h.unchanged()
        h.whole[start - 1] = 0
        with pytest.raises(AssertionError, match="wrote into its input"):
            h.unchanged("case")
