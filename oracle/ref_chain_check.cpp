// TEST INFRASTRUCTURE. main() of oracle/_san/ref_chain_check (`make -C oracle SAN=1`): the reference's three throughput-chain
// blocks, the stand-ins of ref_standins/ and ref_chain_driver.cpp in ONE executable built with AddressSanitizer and
// UndefinedBehaviorSanitizer (CPU build), run as a child process by tests/test_hier_reference_cpu.py.  Every input and output
// lives in a heap buffer of exactly the size the call may touch, so a read behind `in` or a write past `out` is the sanitizer's to
// report.  Each block runs a seeded list of geometries twice, all items in one work() call and in ragged calls (1, 3, 1, 2, ...),
// and both must give the same bytes (overlap_save's history and the window counter cross the calls).
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
const char *ref_chain_last_error(void);
void *ref_overlap_save_create(int, int, int);
void *ref_vector_cut_create(int, int, int, int);
void *ref_phase_window_create(int, int, int, float, float, int);
void ref_chain_destroy(void *);
int ref_chain_work(void *, int, const void *, void *);
}

static unsigned g_state = 2463534242u;
static unsigned rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

// the block over `nitems` items of inb bytes in / outb bytes out: one call, then ragged calls on exactly-sized buffers
static int twice(void *one, void *many, int nitems, size_t inb, size_t outb, const char *what)
{
    if (!one || !many) { printf("FAIL %s: constructor: %s\n", what, ref_chain_last_error()); return 1; }
    std::vector<char> in(inb * (size_t)nitems), a(outb * (size_t)nitems), b(outb * (size_t)nitems);
    for (size_t i = 0; i < in.size(); i++) in[i] = (char)(rnd() % 61u);          // small integers: finite as float32 bit patterns or not, bytes are bytes
    int bad = 0;
    if (ref_chain_work(one, nitems, in.data(), a.data()) != nitems) { printf("FAIL %s: work: %s\n", what, ref_chain_last_error()); bad = 1; }
    static const int ragged[4] = {1, 3, 1, 2};
    for (int done = 0, k = 0; done < nitems; k++) {
        const int n = nitems - done < ragged[k % 4] ? nitems - done : ragged[k % 4];
        std::vector<char> ci(in.begin() + (long)(inb * (size_t)done), in.begin() + (long)(inb * (size_t)(done + n))), co(outb * (size_t)n);
        if (ref_chain_work(many, n, ci.data(), co.data()) != n) { printf("FAIL %s: ragged work: %s\n", what, ref_chain_last_error()); bad = 1; break; }
        memcpy(b.data() + outb * (size_t)done, co.data(), co.size());
        done += n;
    }
    if (!bad && memcmp(a.data(), b.data(), a.size())) { printf("FAIL %s: one call and ragged calls differ\n", what); bad = 1; }
    ref_chain_destroy(one); ref_chain_destroy(many);
    return bad;
}

int main()
{
    int bad = 0, ncase = 0;
    char what[128];
    const int itemsizes[4] = {1, 2, 4, 8};
    for (int rep = 0; rep < 48; rep++) {
        const int isz = itemsizes[rep % 4], nitems = 1 + (int)(rnd() % 9u);
        const int outlen = 2 + (int)(rnd() % 300u), ovl = rep % 6 == 0 ? 1 : rep % 6 == 1 ? outlen / 2 : 1 + (int)(rnd() % (unsigned)(outlen / 2));
        snprintf(what, sizeof what, "overlap_save(%d, %d, %d), %d items", isz, outlen, ovl, nitems);
        bad += twice(ref_overlap_save_create(isz, outlen, ovl), ref_overlap_save_create(isz, outlen, ovl), nitems, (size_t)isz * (size_t)(outlen - ovl),
                     (size_t)isz * (size_t)outlen, what);
        const int veclen = 1 + (int)(rnd() % 500u), blk = 1 + (int)(rnd() % (unsigned)veclen);
        const int off = rep % 3 == 0 ? 0 : rep % 3 == 1 ? veclen - blk : (int)(rnd() % (unsigned)(veclen - blk + 1));
        snprintf(what, sizeof what, "vector_cut_vxx(%d, %d, %d, %d), %d items", isz, veclen, off, blk, nitems);
        bad += twice(ref_vector_cut_create(isz, veclen, off, blk), ref_vector_cut_create(isz, veclen, off, blk), nitems, (size_t)isz * (size_t)veclen,
                     (size_t)isz * (size_t)blk, what);
        const int l = rep % 5 == 0 ? 2 : rep % 5 == 1 ? 2 * (int)(rnd() % 60u) + 3 : 4 << (rnd() % 7u), R = 2 + rep % 15;
        const int shifts = (int)(rnd() % 8000u) - 4000, wt = rep % 3;
        const float pbw = 0.3f + 0.01f * (float)(rnd() % 70u), sbw = pbw < 0.7f ? pbw + 0.25f : 1.0f;
        snprintf(what, sizeof what, "phase_shifting_windowing_vcc(%d, %d, %d, %g, %g, %d), %d items", l, R, shifts, pbw, sbw, wt, nitems);
        bad += twice(ref_phase_window_create(l, R, shifts, pbw, sbw, wt), ref_phase_window_create(l, R, shifts, pbw, sbw, wt), nitems, 8u * (size_t)l,
                     8u * (size_t)l, what);
        ncase += 3;
    }
    // what the phase window's constructor refuses must come back as an error, not as a crash
    if (ref_phase_window_create(64, 4, 1, 0.0f, 1.0f, 1) || ref_phase_window_create(64, 4, 1, 0.5f, 0.0f, 1) || ref_phase_window_create(64, 4, 1, 0.8f, 0.5f, 1)) {
        printf("FAIL: an invalid constructor call was accepted\n");
        bad++;
    }
    if (bad) { printf("%d of %d cases FAILED\n", bad, ncase); return 1; }
    printf("%d cases, all as expected\n", ncase);
    return 0;
}
