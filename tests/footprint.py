"""Footprint checks: did a call write exactly its output bytes, and nothing else?  (tests/test_footprint_cpu.py proves the checker on numpy writes,
tests/test_footprint_gpu.py holds every entry of the library to it.)

A Banded region is ONE allocation laid out as  [guard | payload 0 | guard | payload 1 | ... | guard].  Before every call the whole allocation is filled
with one poison byte; check(expected) then asserts that every payload holds the expected bytes and that every guard byte still is the poison byte.  Every
case runs under both poison bytes (twice()): a byte a kernel never wrote cannot equal the expected byte under 0xA5 AND under 0x5A, whatever the expected
byte is, so no "this value never occurs in an output" assumption is made (an sc8 sample is two arbitrary bytes).

What the method rests on is asserted in the constructor, not left to the cases: every guard is at least one further block of the buffer long (block_bytes,
the bytes one more block of the call would take) and at least 64 KiB, a multiple of 256 bytes, and every payload starts at a multiple of 256 bytes, the
alignment hipMalloc gives a buffer of its own.  Lesser alignments are not tested.

An input ring gets the same banding with another filling (ring_surround): NaN around a float ring, the type's minimum around an integer ring, so that a
kernel whose output depends on a sample outside the ring cannot reproduce the expected bytes.  A read outside the ring that never reaches an output byte
stays invisible: that is the known limit of the method.

Nothing here needs a GPU: the device form takes a test's DeviceBuffers (tests/test_fine_tuning_routes_gpu.py) and goes through its hip handle."""
import ctypes as C

import numpy as np

POISONS = (0xA5, 0x5A)
MIN_GUARD = 64 * 1024
ALIGN = 256


def round_up(n, m):
    return (int(n) + m - 1) // m * m


def guard_bytes(block_bytes):
    """the length of every guard: one further block, 64 KiB at the least, rounded up to 256 bytes"""
    return round_up(max(int(block_bytes), MIN_GUARD), ALIGN)


def as_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Banded:
    """The layout and the checker; HostBanded / DeviceBanded own the memory.  sizes: the payloads' byte counts; block_bytes: what one more block of the
    largest payload would take."""

    def __init__(self, sizes, block_bytes):
        assert POISONS[0] ^ POISONS[1] == 0xFF and len(set(POISONS)) == 2, "two poison bytes that differ in every bit"
        self.sizes = [int(n) for n in sizes]
        assert self.sizes and all(n >= 0 for n in self.sizes) and block_bytes > 0
        self.guard = guard_bytes(block_bytes)
        self.starts, at = [], self.guard
        for n in self.sizes:
            self.starts.append(at)
            at = round_up(at + n, ALIGN) + self.guard
        self.total = at
        # the conditions of the method
        assert self.guard >= block_bytes and self.guard >= MIN_GUARD and self.guard % ALIGN == 0, (self.guard, block_bytes)
        assert all(s % ALIGN == 0 for s in self.starts), self.starts
        ends = [s + n for s, n in zip(self.starts, self.sizes)]
        assert self.starts[0] >= self.guard and self.total - ends[-1] >= self.guard
        assert all(b - a >= self.guard for a, b in zip(ends, self.starts[1:])), "a guard between every pair of payloads"
        self.poison = None          # the byte of the last fill()
        self.checked = set()        # the poison bytes under which check() has passed

    # -- what the owners give
    def _fill(self, byte):
        raise NotImplementedError

    def _read(self):
        """the whole allocation as uint8[total]"""
        raise NotImplementedError

    def fill(self, byte):
        assert byte in POISONS, byte
        self._fill(byte)
        self.poison = byte

    def check(self, expected, what=""):
        """expected: one array per payload (any dtype; its bytes).  Raises AssertionError naming the first and last offending offset, relative to the
        payload, and the count: of payload bytes that differ from the expected ones (and how many of those still hold the poison byte: unwritten), and
        of guard bytes that no longer hold the poison byte (negative offsets: in front of the payload; offsets >= its size: behind it)."""
        assert self.poison in POISONS, "check() without fill()"
        if isinstance(expected, np.ndarray):
            expected = [expected]
        assert len(expected) == len(self.sizes), (len(expected), len(self.sizes))
        mem = self._read()
        assert mem.dtype == np.uint8 and mem.size == self.total
        bad = []
        is_guard = np.ones(self.total, bool)
        for k, (s, n, e) in enumerate(zip(self.starts, self.sizes, expected)):
            e = as_bytes(e)
            assert e.size == n, "%s: payload %d holds %d bytes, %d expected ones were given" % (what, k, n, e.size)
            is_guard[s:s + n] = False
            got = mem[s:s + n]
            off = np.flatnonzero(got != e)
            if off.size:
                unwritten = int(np.count_nonzero(got[off] == self.poison))
                bad.append("payload %d: %d of %d bytes differ from the expected ones, first at offset %d, last at offset %d (%d of them still hold the poison "
                           "byte: unwritten)" % (k, off.size, n, off[0], off[-1], unwritten))
        hit = np.flatnonzero(is_guard & (mem != self.poison))
        if hit.size:
            # every guard byte belongs to the payload in front of it; the first guard to payload 0
            owner = np.clip(np.searchsorted(np.asarray(self.starts), hit, side="right") - 1, 0, None)
            for k in np.unique(owner):
                rel = hit[owner == k] - self.starts[k]
                bad.append("payload %d: %d guard bytes written, first at offset %d, last at offset %d (the payload is bytes 0 to %d)"
                           % (k, rel.size, rel[0], rel[-1], self.sizes[k] - 1))
        assert not bad, "%s, poison 0x%02X: %s" % (what or "footprint", self.poison, "; ".join(bad))
        self.checked.add(self.poison)


class HostBanded(Banded):
    """the numpy form: outs[c] of the host entries are views of its payloads"""

    def __init__(self, sizes, block_bytes):
        super().__init__(sizes, block_bytes)
        self._raw = np.zeros(self.total + ALIGN, np.uint8)
        skip = (-self._raw.ctypes.data) % ALIGN
        self.mem = self._raw[skip:skip + self.total]
        assert self.mem.ctypes.data % ALIGN == 0

    def _fill(self, byte):
        self.mem[:] = byte

    def _read(self):
        return self.mem

    def view(self, k, dtype, shape=None):
        """payload k as a writable array of dtype (a view: what the library is handed)"""
        a = self.mem[self.starts[k]:self.starts[k] + self.sizes[k]].view(dtype)
        return a if shape is None else a.reshape(shape)


class DeviceBanded(Banded):
    """the device form: one hipMalloc of a test's DeviceBuffers (freed with it)"""

    def __init__(self, dev, sizes, block_bytes):
        super().__init__(sizes, block_bytes)
        self.dev = dev
        self.base = dev.put(np.zeros(self.total, np.uint8))
        assert self.base.value % ALIGN == 0, "hipMalloc gives 256-byte alignment"

    def _fill(self, byte):
        assert self.dev.hip.hipMemset(self.base, C.c_int(byte), C.c_size_t(self.total)) == 0
        # hipMemset on device memory may return before the fill has run, and a handle's own stream does not wait for the null stream: without this
        # the fill can land on top of what the call under test stores
        assert self.dev.hip.hipDeviceSynchronize() == 0

    def _read(self):
        return self.dev.get(self.base, self.total, np.uint8)

    def ptr(self, k=0):
        return C.c_void_p(self.base.value + self.starts[k])


def twice(*bands):
    """for poison in twice(band, ...): every band is filled with the poison byte; the body makes the call and checks every band.  Both poison bytes, and
    a body that left a band unchecked is an error."""
    for byte in POISONS:
        for b in bands:
            b.fill(byte)
        yield byte
        for b in bands:
            assert byte in b.checked, "a band was not checked under poison 0x%02X" % byte


# ---- input rings ------------------------------------------------------------------------------------------------------------------------------------------

def ring_surround(ring, block_samples):
    """(whole, start): `ring` (complex64 / float32 samples, or interleaved int16 / int8 I/Q) inside one array of its dtype, NaN (float) or the type's minimum
    (integer) in front of it and behind it, each at least one further block (block_samples, counted in elements of `ring`: twice the samples of an
    interleaved integer ring) and 64 KiB long; the ring starts at element `start`, a multiple of 256 bytes."""
    ring = np.ascontiguousarray(ring).reshape(-1)
    item = ring.dtype.itemsize
    g = guard_bytes(block_samples * item)
    assert g % item == 0
    back = round_up(g + ring.nbytes, ALIGN) + g - (g + ring.nbytes)
    n0, n1 = g // item, back // item
    if ring.dtype.kind in "fc":
        fill = np.array(np.nan, ring.dtype) if ring.dtype.kind == "f" else np.array(complex(np.nan, np.nan), ring.dtype)
    else:
        fill = np.array(np.iinfo(ring.dtype).min, ring.dtype)
    whole = np.empty(n0 + ring.size + n1, ring.dtype)
    whole[:n0] = fill
    whole[n0:n0 + ring.size] = ring
    whole[n0 + ring.size:] = fill
    assert (n0 * item) % ALIGN == 0 and n0 * item >= g and n1 * item >= g
    return whole, n0


class DeviceRing:
    """an input ring on the device inside its surround; unchanged() asserts that the call wrote nothing into the ring or around it"""

    def __init__(self, dev, ring, block_samples):
        self.dev = dev
        self.whole, self.start = ring_surround(ring, block_samples)
        self.base = dev.put(self.whole)
        assert self.base.value % ALIGN == 0
        self.ptr = C.c_void_p(self.base.value + self.start * self.whole.dtype.itemsize)

    def unchanged(self, what=""):
        now = self.dev.get(self.base, self.whole.size, self.whole.dtype)
        assert now.tobytes() == self.whole.tobytes(), "%s: the call wrote into its input ring or around it" % what


class HostRing:
    """the same on the host: .ring is the view the host entries are handed"""

    def __init__(self, ring, block_samples):
        whole, start = ring_surround(ring, block_samples)
        raw = np.empty(whole.nbytes + ALIGN, np.uint8)
        skip = (-raw.ctypes.data) % ALIGN
        self._raw = raw
        self.whole = raw[skip:skip + whole.nbytes].view(whole.dtype)
        self.whole[:] = whole
        self.before = whole
        n = np.ascontiguousarray(ring).size
        self.ring = self.whole[start:start + n]
        assert self.ring.ctypes.data % ALIGN == 0

    def unchanged(self, what=""):
        assert self.whole.tobytes() == self.before.tobytes(), "%s: the call wrote into its input or around it" % what
