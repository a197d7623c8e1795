/* Guard bands around every allocation a process makes through the HIP runtime, without LD_PRELOAD and without a change to the library: loaded with
 * RTLD_GLOBAL BEFORE libfdc_amd.so (as hip_alloc_counter.c is), its hipMalloc & co. come first in the global lookup scope, so the library's calls bind
 * here.  Each allocation of n bytes becomes  [guard g | payload n | guard g]  of the runtime's own memory, ALL of it filled with the current poison byte
 * (the payload too: a buffer read before it was written then shows in the outputs); the caller gets base + g.  g is a multiple of 256, so the payload
 * keeps hipMalloc's 256-byte alignment; the back guard starts at byte n exactly.  fdc_test_guard_check() copies every live allocation's guards home and
 * counts the bytes that no longer hold their poison; hipFree does the same for the block it frees and keeps what it found (the sticky count).
 * Device memory (hipMalloc) and plain pinned memory (hipHostMalloc with hipHostMallocDefault) are banded; any other hipHostMalloc flag passes through
 * (the library takes the device address of its mapped table).  tests/test_guard_alloc_cpu.py proves all of it on tests/cpp/fake_hip_runtime.c;
 * tests/test_guard_bands_gpu.py runs every entry of the library inside it. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <pthread.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the runtime's own entry: next in the lookup order, or (the shim linked without the runtime: --as-needed drops an unreferenced library) by handle */
static void *real_sym(const char *name)
{
    void *f = dlsym(RTLD_NEXT, name);
    if (!f) {
        void *h = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
        if (h) f = dlsym(h, name);
    }
    return f;
}
typedef int (*malloc_fn)(void **, size_t);
typedef int (*free_fn)(void *);
typedef int (*host_malloc_fn)(void **, size_t, unsigned);
typedef int (*memset_fn)(void *, int, size_t);
typedef int (*memcpy_fn)(void *, const void *, size_t, int);
typedef int (*sync_fn)(void);
enum { kDeviceToHost = 2 };                       /* hipMemcpyDeviceToHost */

static malloc_fn r_malloc;
static free_fn r_free, r_host_free;
static host_malloc_fn r_host_malloc;
static memset_fn r_memset;
static memcpy_fn r_memcpy;
static sync_fn r_sync;
static pthread_once_t once = PTHREAD_ONCE_INIT;
static void resolve(void)
{
    r_malloc = (malloc_fn)real_sym("hipMalloc");
    r_free = (free_fn)real_sym("hipFree");
    r_host_malloc = (host_malloc_fn)real_sym("hipHostMalloc");
    r_host_free = (free_fn)real_sym("hipHostFree");
    r_memset = (memset_fn)real_sym("hipMemset");
    r_memcpy = (memcpy_fn)real_sym("hipMemcpy");
    r_sync = (sync_fn)real_sym("hipDeviceSynchronize");
}

struct rec {
    struct rec *next;
    char *base;              /* what the runtime gave: g + n + g bytes */
    size_t n, g;
    int poison, host;
    long ordinal;            /* 0, 1, 2, ... in the order of the calls, device and host together */
};
/* what a scan of one allocation's guards found: offsets relative to the payload (negative: in front of it; >= n: behind it) */
struct hit { long ordinal, n, first, last, count; int poison, host, at_free; };

static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
static struct rec *live;
static size_t cur_guard = 64 * 1024;
static int cur_poison = 0xFF;
static long n_banded, n_freed, next_ordinal;
static long sticky_count, n_runtime_errors;
static struct hit sticky_first;          /* the first broken guard found at a free (count 0: none yet) */

/* one guard of `r`, `mem` its bytes at home, `rel` the payload-relative offset of its first byte */
static void scan(const struct rec *r, const unsigned char *mem, long rel, struct hit *h)
{
    const unsigned char want = (unsigned char)r->poison;
    for (size_t i = 0; i < r->g; ++i)
        if (mem[i] != want) {
            if (!h->count) h->first = rel + (long)i;
            h->last = rel + (long)i;
            ++h->count;
        }
}
/* both guards of `r` (the device is synchronised by the caller); 0, or -1 where the runtime refused a copy */
static int look(const struct rec *r, struct hit *h, int at_free)
{
    memset(h, 0, sizeof *h);
    h->ordinal = r->ordinal; h->n = (long)r->n; h->poison = r->poison; h->host = r->host; h->at_free = at_free;
    if (r->host) {
        scan(r, (const unsigned char *)r->base, -(long)r->g, h);
        scan(r, (const unsigned char *)r->base + r->g + r->n, (long)r->n, h);
        return 0;
    }
    unsigned char *tmp = (unsigned char *)malloc(2 * r->g);
    if (!tmp) return -1;
    int rc = r_memcpy(tmp, r->base, r->g, kDeviceToHost);
    if (!rc) rc = r_memcpy(tmp + r->g, r->base + r->g + r->n, r->g, kDeviceToHost);
    if (!rc) {
        scan(r, tmp, -(long)r->g, h);
        scan(r, tmp + r->g, (long)r->n, h);
    }
    free(tmp);
    return rc ? -1 : 0;
}

static int banded_malloc(void **p, size_t n, int host)
{
    pthread_once(&once, resolve);
    pthread_mutex_lock(&mu);
    const size_t g = cur_guard;
    const int poison = cur_poison;
    pthread_mutex_unlock(&mu);
    void *base = NULL;
    const size_t total = g + n + g;
    int rc = host ? r_host_malloc(&base, total, 0) : r_malloc(&base, total);
    if (rc || !base) { *p = NULL; return rc ? rc : 2 /* hipErrorOutOfMemory */; }
    if (host)
        memset(base, poison, total);
    else {
        /* the fill may return before it has run, and the library's streams do not wait for the null stream (tests/footprint.py): without the
         * synchronise the fill can land on top of what the library stores */
        rc = r_memset(base, poison, total);
        if (!rc) rc = r_sync();
        if (rc) { r_free(base); *p = NULL; return rc; }
    }
    struct rec *r = (struct rec *)calloc(1, sizeof *r);
    if (!r) { if (host) r_host_free(base); else r_free(base); *p = NULL; return 2; }
    r->base = (char *)base; r->n = n; r->g = g; r->poison = poison; r->host = host;
    pthread_mutex_lock(&mu);
    r->ordinal = next_ordinal++;
    r->next = live;
    live = r;
    ++n_banded;
    pthread_mutex_unlock(&mu);
    *p = r->base + g;
    return 0;
}

/* 1 and *rc set: p was one of ours and is gone; 0: not in the list */
static int banded_free(void *p, int host, int *rc)
{
    pthread_once(&once, resolve);
    pthread_mutex_lock(&mu);
    struct rec **at = &live, *r = NULL;
    for (; *at; at = &(*at)->next)
        if ((*at)->host == host && (*at)->base + (*at)->g == (char *)p) { r = *at; *at = r->next; break; }
    pthread_mutex_unlock(&mu);
    if (!r) return 0;
    struct hit h;
    int bad = 0;
    if (!host) bad = r_sync() != 0;                  /* work still in flight may be what breaks the guard */
    if (!bad) bad = look(r, &h, 1) != 0;
    pthread_mutex_lock(&mu);
    ++n_freed;
    if (bad) ++n_runtime_errors;
    else if (h.count) {
        if (!sticky_count) sticky_first = h;
        sticky_count += h.count;
    }
    pthread_mutex_unlock(&mu);
    *rc = host ? r_host_free(r->base) : r_free(r->base);
    free(r);
    return 1;
}

int hipMalloc(void **p, size_t n) { return banded_malloc(p, n, 0); }
int hipFree(void *p)
{
    int rc = 0;
    if (p && banded_free(p, 0, &rc)) return rc;
    pthread_once(&once, resolve);
    return r_free(p);                                 /* NULL, and pointers the shim never handed out */
}
int hipHostMalloc(void **p, size_t n, unsigned flags)
{
    if (flags == 0) return banded_malloc(p, n, 1);   /* hipHostMallocDefault */
    pthread_once(&once, resolve);
    return r_host_malloc(p, n, flags);
}
int hipHostFree(void *p)
{
    int rc = 0;
    if (p && banded_free(p, 1, &rc)) return rc;
    pthread_once(&once, resolve);
    return r_host_free(p);
}

/* guard length (a multiple of 256) and poison byte of the allocations made from now on; 0, or -1 for arguments the method does not allow */
int fdc_test_guard_set(size_t guard_bytes, int poison)
{
    if (guard_bytes == 0 || guard_bytes % 256 || poison < 0 || poison > 255) return -1;
    pthread_mutex_lock(&mu);
    cur_guard = guard_bytes;
    cur_poison = poison;
    pthread_mutex_unlock(&mu);
    return 0;
}

/* Synchronises the device and scans every live allocation.  Returns the guard bytes that no longer hold their poison, plus what the frees found; -1
 * where the runtime refused a call.  out[0..4] (may be null): ordinal, payload bytes, first and last offending offset relative to the payload and the
 * count of the FIRST offender (the lowest ordinal); text (may be null): the same in words. */
long fdc_test_guard_check(long *out, char *text, size_t cap)
{
    pthread_once(&once, resolve);
    if (text && cap) text[0] = 0;
    if (r_sync() != 0) return -1;
    pthread_mutex_lock(&mu);
    long total = sticky_count, errors = n_runtime_errors;
    struct hit first = sticky_first, h;
    if (!sticky_count) memset(&first, 0, sizeof first);
    for (const struct rec *r = live; r; r = r->next) {
        if (look(r, &h, 0)) { ++errors; continue; }
        if (h.count) {
            total += h.count;
            if (!first.count || h.ordinal < first.ordinal) first = h;
        }
    }
    pthread_mutex_unlock(&mu);
    if (out) { out[0] = first.ordinal; out[1] = first.n; out[2] = first.first; out[3] = first.last; out[4] = first.count; }
    if (text && cap && first.count)
        snprintf(text, cap, "%s allocation number %ld of %ld payload bytes, poison 0x%02X: %ld guard bytes written, first at offset %ld, last at offset "
                 "%ld (the payload is bytes 0 to %ld)%s", first.host ? "pinned" : "device", first.ordinal, first.n, first.poison, first.count, first.first,
                 first.last, first.n - 1, first.at_free ? ", found when it was freed" : "");
    return errors ? -1 : total;
}

/* v[0]: allocations banded; v[1]: of those, freed */
void fdc_test_guard_counts(long *v)
{
    pthread_mutex_lock(&mu);
    v[0] = n_banded; v[1] = n_freed;
    pthread_mutex_unlock(&mu);
}
