// TEST INFRASTRUCTURE. main() of oracle/_san/ref_sinks_check (`make -C oracle SAN=1`): the reference's three sink blocks, the
// stand-ins of ref_standins/ and ref_sinks_driver.cpp in ONE executable built with AddressSanitizer and
// UndefinedBehaviorSanitizer (CPU build), run as a child process by tests/test_sinks_reference_cpu.py.  It drives a built-in list
// of exact-class cases (integer powers: amplitudes 1 and 16 with phases from {1, i, -1, -i}) through every block, one item per
// work() call and all items in one call, single-threaded and threaded, over every maxblocks / delay regime, and checks that both
// call patterns publish the same PDUs.  What it is FOR is the sanitizers' verdict on the reads and writes along the way.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fdc_oracle.h"

struct ref_pdu_list { fdco_pdu *pdu; int n, cap; char **ids; };
extern "C" {
const char *ref_sinks_last_error(void);
void *ref_pac_create(int, float, float, int, float, int, int, int);
void *ref_vcm_create(int, int, const float *, float, int, int, float, int, double, int);
void *ref_sd_create(int, int, int, float, float, float, float, float, int, int, int);
void ref_sinks_destroy(void *);
int ref_sinks_work(void *, const float *, int, int);
void ref_sinks_list_clear(ref_pdu_list *);
int ref_sinks_drain(void *, ref_pdu_list *);
}

static unsigned g_state = 12345u;
static unsigned rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

// nb items of N bins: floor 1, carriers of amplitude 16 keyed on and off; every bin with a phase from {1, i, -1, -i}
static std::vector<float> spectrum(int N, int nb, int ncar)
{
    std::vector<float> s(2 * (size_t)N * nb);
    std::vector<float> amp((size_t)N * nb, 1.0f);
    for (int c = 0; c < ncar; c++) {
        const int lo = (int)(rnd() % (unsigned)(N - N / 8)), w = 1 + (int)(rnd() % (unsigned)(N / 8));
        int m = (int)(rnd() % 3u);                                // may start in the first item
        while (m < nb) {
            const int on = 1 + (int)(rnd() % 5u);
            for (int b = m; b < m + on && b < nb; b++)
                for (int k = lo; k < lo + w && k < N; k++) amp[(size_t)b * N + k] = 16.0f;
            m += on + 1 + (int)(rnd() % 4u);
        }
    }
    for (size_t i = 0; i < (size_t)N * nb; i++) {
        const unsigned ph = rnd() & 3u;
        s[2 * i] = ph == 0 ? amp[i] : ph == 2 ? -amp[i] : 0.0f;
        s[2 * i + 1] = ph == 1 ? amp[i] : ph == 3 ? -amp[i] : 0.0f;
    }
    return s;
}

static bool same(const ref_pdu_list &a, const ref_pdu_list &b, bool ordered)
{
    if (a.n != b.n) return false;
    std::vector<char> used((size_t)b.n, 0);
    for (int i = 0; i < a.n; i++) {
        bool found = false;
        for (int j = ordered ? i : 0; j < (ordered ? i + 1 : b.n) && !found; j++) {
            const fdco_pdu &p = a.pdu[i], &q = b.pdu[j];
            if (used[(size_t)j] || strcmp(a.ids[i] + 20, b.ids[j] + 20) || p.finalized != q.finalized || p.part != q.part || p.has_part != q.has_part ||
                p.blockstart != q.blockstart || p.blockend != q.blockend || p.vectorstart != q.vectorstart || p.vectorend != q.vectorend ||
                p.nsamples != q.nsamples || memcmp(p.samples, q.samples, sizeof(float) * 2 * (size_t)p.nsamples)) continue;
            used[(size_t)j] = 1; found = true;
        }
        if (!found) return false;
    }
    return true;
}

static int run(void *one, void *many, const std::vector<float> &s, int nb, bool ordered, const char *what, long *npdu)
{
    if (!one || !many) { printf("FAIL %s: constructor: %s\n", what, ref_sinks_last_error()); return 1; }
    ref_pdu_list a, b;
    int bad = 0;
    if (ref_sinks_work(one, s.data(), nb, 1) != nb || ref_sinks_work(many, s.data(), nb, 0) != nb) { printf("FAIL %s: work: %s\n", what, ref_sinks_last_error()); bad = 1; }
    if (ref_sinks_drain(one, &a) < 0 || ref_sinks_drain(many, &b) < 0) { printf("FAIL %s: drain: %s\n", what, ref_sinks_last_error()); return 1; }
    if (!bad && !same(a, b, ordered)) { printf("FAIL %s: %d PDUs item by item, %d in one call, or their contents differ\n", what, a.n, b.n); bad = 1; }
    *npdu += a.n;
    ref_sinks_list_clear(&a); ref_sinks_list_clear(&b);
    ref_sinks_destroy(one); ref_sinks_destroy(many);
    return bad;
}

int main()
{
    const int maxblocks[4] = {-1, 0, 1, 3};
    int bad = 0, ncase = 0;
    long npdu = 0;
    char what[128];
    for (int rep = 0; rep < 24; rep++) {
        const int N = rep % 3 == 0 ? 256 : rep % 3 == 1 ? 1024 : 4096, R = 2 << (rep % 3), nb = 10 + rep % 9;
        const int mb = maxblocks[rep % 4], delay = (rep / 4) % 4;
        const std::vector<float> s = spectrum(N, nb, 4);
        // PowerActivationChannel over a band the carriers cross; once against the upper band edge (the reference's clamp)
        const float cf = rep % 6 == 5 ? 0.97f : 0.2f + 0.025f * (float)rep, bw = rep % 6 == 5 ? 0.05f : 0.01f + 0.004f * (float)(rep % 7);
        snprintf(what, sizeof what, "PowerActivationChannel %d (N %d, R %d, maxblocks %d)", rep, N, R, mb);
        bad += run(ref_pac_create(N, cf, bw, R, 7.3f, mb, delay, rep), ref_pac_create(N, cf, bw, R, 7.3f, mb, delay, rep), s, nb, true, what, &npdu);
        const float segs[4] = {0.04f, 0.46f, 0.52f, 0.93f};
        const float mcd = (2.0f * (float)(1 + rep % 16) + 0.5f) / (float)N;
        const double puffer = 0.1 * (double)(rep % 4);
        for (int threads = 0; threads < 2; threads++) {           // threaded: the order inside an item is the threads' (compared as a set)
            snprintf(what, sizeof what, "activity_detection_channelizer_vcm %d (N %d, R %d, maxblocks %d, delay %d, threads %d)", rep, N, R, mb, delay, threads);
            bad += run(ref_vcm_create(N, 2, segs, 9.1f, R, mb, mcd, delay, puffer, threads), ref_vcm_create(N, 2, segs, 9.1f, R, mb, mcd, delay, puffer, threads),
                       s, nb, threads == 0, what, &npdu);
            snprintf(what, sizeof what, "SegmentDetection %d (N %d, R %d, maxblocks %d, delay %d, threads %d)", rep, N, R, mb, delay, threads);
            bad += run(ref_sd_create(rep, N, R, 0.1f, 0.9f, 9.1f, mcd, (float)puffer, mb, delay, threads),
                       ref_sd_create(rep, N, R, 0.1f, 0.9f, 9.1f, mcd, (float)puffer, mb, delay, threads), s, nb, threads == 0, what, &npdu);
            ncase += 2;
        }
        ncase += 1;
    }
    // what the constructors refuse must come back as an error, not as a crash
    const float reversed[2] = {0.5f, 0.3f};
    if (ref_pac_create(256, 0.01f, 0.1f, 2, 6.0f, -1, 0, 0) || ref_vcm_create(256, 1, reversed, 10.0f, 2, -1, 0.0625f, 1, 0.0, 0) ||
        ref_sd_create(0, 256, 2, 0.3f, 0.3f, 10.0f, 0.0625f, 0.0f, -1, 1, 0)) { printf("FAIL: an invalid constructor call was accepted\n"); bad++; }
    if (bad) { printf("%d of %d cases FAILED\n", bad, ncase); return 1; }
    printf("%d cases, all as expected; %ld PDUs\n", ncase, npdu);
    return 0;
}
