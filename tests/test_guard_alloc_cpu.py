"""The guard-band shim (tests/cpp/hip_guard_alloc.c) proved where no GPU is, as tests/test_footprint_cpu.py proves tests/footprint.py: the shim is linked
against tests/cpp/fake_hip_runtime.c, whose "device" memory is host memory, and driven through ctypes; the stray bytes are written with ctypes.memmove.
Every build is loaded into a scope of its own (not RTLD_GLOBAL): nothing else in this process ever binds to the shim or to the fake.

Every property is asserted under both poison bytes (0xFF and 0x00); test_a_stray_byte_equal_to_the_poison is why there are two."""
import ctypes as C
import itertools
import threading

import pytest

import guard_alloc as GA
from footprint import ALIGN, MIN_GUARD, guard_bytes

POISONS = GA.POISONS
SIZES = (0, 1, 16, 1000, 4096, 65537)              # nothing, one byte, one float4, no multiple of 256, a multiple, and one byte more than 64 KiB
_serial = itertools.count()


@pytest.fixture
def fresh(tmp_path):
    """fresh(): a newly built shim on a fake runtime of its own: (Shim, the fake's CDLL).  Its counters and its sticky count start at zero."""
    def make():
        shim, fake = GA.build_on_fake(str(tmp_path), "t%d" % next(_serial))
        return GA.Shim(shim), C.CDLL(fake)
    return make


def poke(address, byte):
    C.memmove(address, bytes([byte]), 1)


def fake_counts(fake):
    v = (C.c_long * 5)()
    fake.fake_hip_counts(v)
    return list(v)


def test_the_two_poisons():
    assert set(POISONS) == {0xFF, 0x00} and len(POISONS) == 2


@pytest.mark.parametrize("host", [False, True], ids=["hipMalloc", "hipHostMalloc"])
@pytest.mark.parametrize("poison", POISONS, ids=["0xFF", "0x00"])
def test_alignment_clean_writes_and_every_guard_edge(fresh, poison, host):
    """every size: a 256-byte aligned pointer, the payload poisoned, a write of every payload byte leaves the check at 0, and one stray byte at -1, -g, n
    and n + g - 1 is reported with its offset, a count of 1, the payload size and the ordinal"""
    s, fake = fresh()
    g = guard_bytes(1)
    assert g == MIN_GUARD
    s.set(g, poison)
    other = poison ^ 0xFF
    ptrs = [s.malloc(n, host) for n in SIZES]
    assert s.counts() == (len(SIZES), 0)
    assert fake_counts(fake)[2 if host else 0] == len(SIZES)                    # the shim forwarded to the runtime it was linked against
    for p, n in zip(ptrs, SIZES):
        assert p % ALIGN == 0, (n, p)
        assert C.string_at(p, n) == bytes([poison]) * n                          # the payload is poisoned too
        C.memset(p, other, n)
    total, first, text = s.check()
    assert total == 0 and text == "", (total, first, text)
    for k, (p, n) in enumerate(zip(ptrs, SIZES)):
        for off in (-1, -g, n, n + g - 1):
            poke(p + off, other)
            total, first, text = s.check()
            assert total == 1 and first == (k, n, off, off, 1), (n, off, total, first, text)
            assert ("number %d of %d payload bytes" % (k, n)) in text and ("first at offset %d," % off) in text, text
            poke(p + off, poison)
            assert s.check()[0] == 0
    # several bytes, in front and behind: first, last and the count
    p, n = ptrs[3], SIZES[3]
    for off in (-7, n, n + 5):
        poke(p + off, other)
    total, first, _ = s.check()
    assert total == 3 and first == (3, n, -7, n + 5, 3), (total, first)
    for off in (-7, n, n + 5):
        poke(p + off, poison)
    # two offenders: the total counts both, the report names the one with the lower ordinal
    poke(ptrs[4] + SIZES[4], other)
    poke(ptrs[1] - 1, other)
    total, first, _ = s.check()
    assert total == 2 and first == (1, 1, -1, -1, 1), (total, first)
    poke(ptrs[4] + SIZES[4], poison)
    poke(ptrs[1] - 1, poison)
    for p in ptrs:
        s.free(p, host)
    assert s.counts() == (len(SIZES), len(SIZES)) and s.check()[0] == 0
    assert fake_counts(fake)[3 if host else 1] == len(SIZES)


@pytest.mark.parametrize("poison", POISONS, ids=["0xFF", "0x00"])
def test_a_stray_byte_equal_to_the_poison(fresh, poison):
    """a stray byte that equals the poison is missed under that poison and found under the other one: why every scenario runs twice"""
    s, _fake = fresh()
    stray = poison
    seen = {}
    for byte in POISONS:
        s.set(MIN_GUARD, byte)
        p = s.malloc(1000)
        poke(p + 1000, stray)
        seen[byte] = s.check()[0]
        poke(p + 1000, byte)
        s.free(p)
    assert seen == {poison: 0, poison ^ 0xFF: 1}, seen
    assert s.check()[0] == 0


@pytest.mark.parametrize("host", [False, True], ids=["hipFree", "hipHostFree"])
@pytest.mark.parametrize("poison", POISONS, ids=["0xFF", "0x00"])
def test_a_guard_broken_before_the_free_still_counts(fresh, poison, host):
    s, fake = fresh()
    s.set(MIN_GUARD, poison)
    a, b = s.malloc(1000, host), s.malloc(24, host)
    poke(b + 24, poison ^ 0xFF)
    poke(b + 30, poison ^ 0xFF)
    s.free(b, host)
    assert fake_counts(fake)[3 if host else 1] == 1                              # the real free followed
    total, first, text = s.check()
    assert total == 2 and first == (1, 24, 24, 30, 2) and "freed" in text, (total, first, text)
    poke(a - 1, poison ^ 0xFF)                                                  # a live offender beside it: the sticky count is added to
    total, first, _ = s.check()
    assert total == 3 and first == (0, 1000, -1, -1, 1), (total, first)
    s.free(a, host)
    assert s.check()[0] == 3 and s.counts() == (2, 2)


def test_pointers_the_shim_never_handed_out_pass_through(fresh):
    s, fake = fresh()
    fake.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    fake.hipFree.argtypes = [C.c_void_p]
    raw = C.c_void_p()
    assert fake.hipMalloc(C.byref(raw), 512) == 0 and raw.value
    before = fake_counts(fake)
    s.free(raw.value)                                                           # not in the list: the runtime's own free gets it
    s.free(None)                                                                # NULL passes through (the fake does not count it)
    s.free(None, host=True)
    assert fake_counts(fake)[1] == before[1] + 1 and s.counts() == (0, 0) and s.check()[0] == 0


def test_other_host_flags_pass_through_untouched(fresh):
    """hipHostMallocMapped (2) and its kin: the library takes a device pointer of its mapped table, so the runtime's pointer goes through as it is"""
    s, fake = fresh()
    p = s.malloc(1000, host=True, flags=2)
    assert s.counts() == (0, 0) and fake_counts(fake)[2] == 1
    poke(p + 1000, 0x33)                                                        # (inside the fake's rounded-up block) nobody looks
    assert s.check()[0] == 0
    s.free(p, host=True)
    assert s.counts() == (0, 0) and fake_counts(fake)[3] == 1


def test_set_changes_later_allocations_only(fresh):
    s, _fake = fresh()
    assert s.so.fdc_test_guard_set(1000, 0xFF) == -1 and s.so.fdc_test_guard_set(0, 0xFF) == -1 and s.so.fdc_test_guard_set(256, 256) == -1
    s.set(MIN_GUARD, 0xFF)
    a = s.malloc(1000)
    s.set(2 * MIN_GUARD, 0x00)
    b = s.malloc(1000)
    assert C.string_at(a - MIN_GUARD, 4) == b"\xff" * 4 and C.string_at(b - 2 * MIN_GUARD, 4) == b"\0" * 4
    assert s.check()[0] == 0                                                    # a is still judged by ITS poison
    poke(a + 1000 + MIN_GUARD - 1, 0x00)                                        # the last byte of a's guard: a's length, not the new one
    poke(b + 1000 + 2 * MIN_GUARD - 1, 0xFF)
    total, first, _ = s.check()
    assert total == 2 and first == (0, 1000, 1000 + MIN_GUARD - 1, 1000 + MIN_GUARD - 1, 1), (total, first)
    poke(a + 1000 + MIN_GUARD - 1, 0xFF)
    total, first, _ = s.check()
    assert total == 1 and first == (1, 1000, 1000 + 2 * MIN_GUARD - 1, 1000 + 2 * MIN_GUARD - 1, 1), (total, first)


@pytest.mark.parametrize("poison", POISONS, ids=["0xFF", "0x00"])
def test_two_threads_allocating_and_freeing(fresh, poison):
    """the library allocates from more than one thread: the list stays consistent (ctypes releases the interpreter lock around every call)"""
    s, fake = fresh()
    s.set(MIN_GUARD, poison)
    rounds, keep = 300, [[], []]
    errors = []

    def run(t):
        try:
            mine = []
            for i in range(rounds):
                n = (17 * i + 5 * t) % 3000
                mine.append((s.malloc(n, host=bool(i & 1)), bool(i & 1)))
                if i % 3 != 2:
                    p, host = mine.pop(0 if i % 2 else -1)
                    s.free(p, host)
            keep[t] = mine
        except Exception as e:                                                  # noqa: BLE001  (reported by the parent thread)
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    live = len(keep[0]) + len(keep[1])
    banded, freed = s.counts()
    assert banded == 2 * rounds and freed == banded - live and live > 0
    assert s.check()[0] == 0
    fc = fake_counts(fake)
    assert fc[0] + fc[2] == banded and fc[1] + fc[3] == freed
    p, host = keep[1][-1]
    poke(p - 1, poison ^ 0xFF)                                                  # every record is still found: its guard ...
    assert s.check()[0] == 1
    for t in (0, 1):
        for p, host in keep[t]:
            s.free(p, host)                                                     # ... and its free
    assert s.counts() == (banded, banded) and s.check()[0] == 1
    fc = fake_counts(fake)
    assert fc[1] + fc[3] == banded
