/* The handful of HIP runtime entries tests/cpp/hip_guard_alloc.c forwards to, on plain host memory: tests/test_guard_alloc_cpu.py links the shim against
 * this instead of libamdhip64.so and proves the shim where no GPU is.  "Device" memory is host memory here, so the test writes its stray bytes with
 * ctypes.  The counters let the test see what reached the runtime. */
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

static long n_malloc, n_free, n_host_malloc, n_host_free, n_sync;

static int get(void **p, size_t n)
{
    /* 256-byte alignment, as hipMalloc gives; a size that is no multiple of the alignment is rounded up for aligned_alloc only */
    *p = aligned_alloc(256, (n + 255) / 256 * 256 + 256);
    return *p ? 0 : 2;
}
int hipMalloc(void **p, size_t n) { __atomic_add_fetch(&n_malloc, 1, __ATOMIC_RELAXED); return get(p, n); }
int hipFree(void *p) { if (p) __atomic_add_fetch(&n_free, 1, __ATOMIC_RELAXED); free(p); return 0; }
int hipHostMalloc(void **p, size_t n, unsigned flags) { (void)flags; __atomic_add_fetch(&n_host_malloc, 1, __ATOMIC_RELAXED); return get(p, n); }
int hipHostFree(void *p) { if (p) __atomic_add_fetch(&n_host_free, 1, __ATOMIC_RELAXED); free(p); return 0; }
int hipMemset(void *p, int v, size_t n) { memset(p, v, n); return 0; }
int hipMemcpy(void *dst, const void *src, size_t n, int kind) { (void)kind; memcpy(dst, src, n); return 0; }
int hipDeviceSynchronize(void) { __atomic_add_fetch(&n_sync, 1, __ATOMIC_RELAXED); return 0; }
void fake_hip_counts(long *v5) { v5[0] = n_malloc; v5[1] = n_free; v5[2] = n_host_malloc; v5[3] = n_host_free; v5[4] = n_sync; }
