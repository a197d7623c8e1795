"""Building and driving tests/cpp/hip_guard_alloc.c, the shim that puts guard bands around every allocation the library makes: shared by
tests/test_guard_alloc_cpu.py (the shim proved on a fake runtime), tests/test_guard_bands_gpu.py (the parent: builds it) and tests/guard_scenarios.py
(the child: loads it before the library and checks the guards after every call).  Nothing here needs a GPU or loads the library."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
# 0xFF: NaN as float32, -1 as an integer.  0x00: the most likely stray value, invisible under itself and seen under 0xFF.  They differ in every bit, so
# no stored byte equals both: every scenario runs under both
POISONS = (0xFF, 0x00)
assert len(POISONS) == 2 and POISONS[0] ^ POISONS[1] == 0xFF


def build_shim(path):
    """the shim against the HIP runtime (as tests/test_no_alloc_gpu.py builds its counter)"""
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", os.path.join(CPP, "hip_guard_alloc.c"), "-o", path, "-ldl", "-lpthread",
                           "-L/opt/rocm/lib", "-Wl,--no-as-needed", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return path


def build_on_fake(directory, tag):
    """(shim, fake runtime) in `directory`, the shim linked against the fake INSTEAD of the runtime.  `tag` goes into both file names and sonames: a
    process that loads two builds gets two of each, every one with its own state."""
    fake = os.path.join(directory, "libfakehip_%s.so" % tag)
    shim = os.path.join(directory, "libhipguard_%s.so" % tag)
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", os.path.join(CPP, "fake_hip_runtime.c"), "-o", fake, "-Wl,-soname," + os.path.basename(fake)])
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", os.path.join(CPP, "hip_guard_alloc.c"), "-o", shim, "-Wl,-soname," + os.path.basename(shim),
                           "-ldl", "-lpthread", "-L" + directory, "-Wl,--no-as-needed", "-lfakehip_%s" % tag, "-Wl,-rpath," + directory])
    return shim, fake


class Shim:
    """the loaded shim.  mode: RTLD_GLOBAL in a child that loads the library afterwards; the default (local) where only the shim itself is driven"""

    def __init__(self, path, mode=C.DEFAULT_MODE):
        self.so = so = C.CDLL(path, mode=mode)
        so.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        so.hipFree.argtypes = [C.c_void_p]
        so.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        so.hipHostFree.argtypes = [C.c_void_p]
        so.fdc_test_guard_set.argtypes = [C.c_size_t, C.c_int]
        so.fdc_test_guard_check.argtypes = [C.POINTER(C.c_long), C.c_char_p, C.c_size_t]
        so.fdc_test_guard_check.restype = C.c_long
        so.fdc_test_guard_counts.argtypes = [C.POINTER(C.c_long)]
        so.fdc_test_guard_counts.restype = None

    def set(self, guard_bytes, poison):
        assert self.so.fdc_test_guard_set(guard_bytes, poison) == 0, (guard_bytes, poison)

    def malloc(self, n, host=False, flags=0):
        p = C.c_void_p()
        rc = self.so.hipHostMalloc(C.byref(p), n, flags) if host else self.so.hipMalloc(C.byref(p), n)
        assert rc == 0 and p.value, (rc, p.value)
        return p.value

    def free(self, p, host=False):
        assert (self.so.hipHostFree(p) if host else self.so.hipFree(p)) == 0

    def check(self):
        """(the guard bytes that no longer hold their poison, frees included; (ordinal, payload bytes, first offset, last offset, count) of the first
        offender; the same in words)"""
        out, text = (C.c_long * 5)(), C.create_string_buffer(512)
        total = self.so.fdc_test_guard_check(out, text, len(text))
        return total, tuple(out), text.value.decode()

    def counts(self):
        v = (C.c_long * 2)()
        self.so.fdc_test_guard_counts(v)
        return tuple(v)
