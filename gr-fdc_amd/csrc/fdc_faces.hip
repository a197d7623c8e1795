// The single-block faces of the C-ABI (include/fdc_amd.h): overlap_save, vector_cut, phase_shifting_windowing and fft_vcc as blocks of their own,
// each with its stream and its device buffers.
#include "fdc_pipeline.hpp"

using namespace fdc::pipe;

// a face under construction: every error return of its create entry (and anything thrown) frees it with the face's own destroy
template <class T>
using Face = std::unique_ptr<T, void (*)(T *)>;

extern "C" {

struct fdc_overlap_save {
    int dev, itemsize, outlen, ovl; hipStream_t s; fdc::DevBuf<unsigned char> d_ring, d_out; int cap = 0;
};

int fdc_overlap_save_create(int device_id, int itemsize, int outputlen, int overlaplen, fdc_overlap_save **out)
{
    FDC_ENTRY("fdc_overlap_save_create")
    if (!out) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (itemsize < 1 || outputlen < 1 || overlaplen < 0 || overlaplen >= outputlen)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "overlap_save: need itemsize>=1 and 0 <= overlaplen < outputlen");
    if (2 * overlaplen > outputlen)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "overlap_save: overlaplen above outputlen/2 makes the reference read before its input buffer");
    int rc = pick_device(device_id); if (rc) return rc;
    Face<fdc_overlap_save> b(new fdc_overlap_save{device_id, itemsize, outputlen, overlaplen, nullptr}, fdc_overlap_save_destroy);
    HIPCHK(hipStreamCreateWithFlags(&b->s, hipStreamNonBlocking));
    *out = b.release();
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_overlap_save_work(fdc_overlap_save *b, const void *in, int nitems, void *out)
{
    FDC_ENTRY("fdc_overlap_save_work")
    if (!b) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (nitems <= 0) return nitems == 0 ? 0 : set_error(FDC_ERR_INVALID_ARGUMENT, "negative item count");
    HIPCHK(hipSetDevice(b->dev));
    const size_t isz = b->itemsize, inb = isz * (b->outlen - b->ovl), outb = isz * b->outlen, ovb = isz * b->ovl;
    if (nitems > b->cap) {
        // fresh buffers, the history carried over; a failure on the way leaves the old ring and capacity in place (nr / no free themselves)
        fdc::DevBuf<unsigned char> nr, no;
        HIPCHK(nr.alloc(ovb + inb * nitems + 16));
        HIPCHK(no.alloc(outb * nitems));
        // on the block's OWN stream: it is non-blocking, so the null stream's memset would not be ordered in front of the copies and the
        // kernel below (round 6: the first item's history came out as whatever the allocation held, now and then)
        if (b->d_ring) HIPCHK(hipMemcpyAsync(nr, b->d_ring, ovb, hipMemcpyDeviceToDevice, b->s));
        else HIPCHK(hipMemsetAsync(nr, 0, ovb + 16, b->s));
        HIPCHK(hipStreamSynchronize(b->s));
        b->d_ring = std::move(nr); b->d_out = std::move(no); b->cap = nitems;   // (a swap: the old buffers go with nr / no)
    }
    HIPCHK(hipMemcpyAsync(b->d_ring + ovb, in, inb * nitems, hipMemcpyHostToDevice, b->s));
    HIPCHK(fdc::launch_overlap_save(b->d_ring, b->d_out, inb, outb, nitems, b->s));
    HIPCHK(hipMemcpyAsync(out, b->d_out, outb * nitems, hipMemcpyDeviceToHost, b->s));
    if (ovb) HIPCHK(hipMemcpyAsync(b->d_ring, b->d_ring + inb * nitems, ovb, hipMemcpyDeviceToDevice, b->s));
    HIPCHK(hipStreamSynchronize(b->s));
    return nitems;
    FDC_ENTRY_END
}

void fdc_overlap_save_destroy(fdc_overlap_save *b)
{
    if (!b) return;
    if (b->s) (void)hipStreamDestroy(b->s);
    delete b;
}

struct fdc_vector_cut {
    int dev, itemsize, veclen, offset, blocklen; hipStream_t s; fdc::DevBuf<unsigned char> d_in, d_out;
};

int fdc_vector_cut_create(int device_id, int itemsize, int veclen, int offset, int blocklen, fdc_vector_cut **out)
{
    FDC_ENTRY("fdc_vector_cut_create")
    if (!out) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (itemsize < 1 || veclen < 1 || blocklen < 1 || offset < 0 || offset + blocklen > veclen)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "vector_cut: slice [offset, offset+blocklen) must lie inside the vector");
    int rc = pick_device(device_id); if (rc) return rc;
    Face<fdc_vector_cut> b(new fdc_vector_cut{device_id, itemsize, veclen, offset, blocklen, nullptr}, fdc_vector_cut_destroy);
    HIPCHK(hipStreamCreateWithFlags(&b->s, hipStreamNonBlocking));
    *out = b.release();
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_vector_cut_work(fdc_vector_cut *b, const void *in, int nitems, void *out)
{
    FDC_ENTRY("fdc_vector_cut_work")
    if (!b) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (nitems <= 0) return nitems == 0 ? 0 : set_error(FDC_ERR_INVALID_ARGUMENT, "negative item count");
    HIPCHK(hipSetDevice(b->dev));
    const size_t inb = (size_t)b->itemsize * b->veclen, outb = (size_t)b->itemsize * b->blocklen;
    HIPCHK(b->d_in.reserve(inb * nitems, inb * nitems));          // the largest batch seen
    HIPCHK(b->d_out.reserve(outb * nitems, outb * nitems));
    HIPCHK(hipMemcpyAsync(b->d_in, in, inb * nitems, hipMemcpyHostToDevice, b->s));
    HIPCHK(fdc::launch_vector_cut(b->d_in, b->d_out, inb, (size_t)b->offset * b->itemsize, outb, nitems, b->s));
    HIPCHK(hipMemcpyAsync(out, b->d_out, outb * nitems, hipMemcpyDeviceToHost, b->s));
    HIPCHK(hipStreamSynchronize(b->s));
    return nitems;
    FDC_ENTRY_END
}

void fdc_vector_cut_destroy(fdc_vector_cut *b)
{
    if (!b) return;
    if (b->s) (void)hipStreamDestroy(b->s);
    delete b;
}

struct fdc_phase_window {
    int dev, l, R, shift, counter; hipStream_t s; fdc::DevBuf<float2> d_win, d_in, d_out;
};

int fdc_phase_window_create(int device_id, int blocklen, int numphasestates, int shifts, float passbw, float stopbw,
                            int windowtype, fdc_phase_window **out)
{
    FDC_ENTRY("fdc_phase_window_create")
    if (!out) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    // lib/phase_shifting_windowing_vcc_impl.cc:46-53
    if (passbw <= 0.0f) return set_error(FDC_ERR_INVALID_ARGUMENT, "PassBw in phase_shifting_windowing_vcc must not be <= 0");
    if (stopbw <= 0.0f) return set_error(FDC_ERR_INVALID_ARGUMENT, "StopBw in phase_shifting_windowing_vcc must not be <= 0");
    if (stopbw < passbw) return set_error(FDC_ERR_INVALID_ARGUMENT, "StopBw must not be < PassBw in phase_shifting_windowing_vcc");
    if (blocklen < 1 || numphasestates < 1) return set_error(FDC_ERR_INVALID_ARGUMENT, "blocklen and numphasestates must be >= 1");
    int rc = pick_device(device_id); if (rc) return rc;
    Face<fdc_phase_window> b(new fdc_phase_window{device_id, blocklen, numphasestates,
                                                  ((shifts % numphasestates) + numphasestates) % numphasestates, 0, nullptr}, fdc_phase_window_destroy);
    std::vector<std::complex<float>> w((size_t)numphasestates * blocklen);
    fdc::window_table(windowtype, blocklen, passbw, stopbw, numphasestates, 1, false, w.data());
    HIPCHK(hipStreamCreateWithFlags(&b->s, hipStreamNonBlocking));
    HIPCHK(b->d_win.alloc(w.size()));
    HIPCHK(hipMemcpy(b->d_win, w.data(), sizeof(float2) * w.size(), hipMemcpyHostToDevice));
    *out = b.release();
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_phase_window_work(fdc_phase_window *b, const void *in, int nitems, void *out)
{
    FDC_ENTRY("fdc_phase_window_work")
    if (!b) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (nitems <= 0) return nitems == 0 ? 0 : set_error(FDC_ERR_INVALID_ARGUMENT, "negative item count");
    HIPCHK(hipSetDevice(b->dev));
    const size_t pts = (size_t)b->l * nitems, nb = sizeof(float2) * pts;
    HIPCHK(b->d_in.reserve(pts, pts));                              // the largest batch seen
    HIPCHK(b->d_out.reserve(pts, pts));
    HIPCHK(hipMemcpyAsync(b->d_in, in, nb, hipMemcpyHostToDevice, b->s));
    HIPCHK(fdc::launch_phase_window(b->d_in, b->d_out, b->d_win, b->l, b->R, b->shift, b->counter, nitems, b->s));
    HIPCHK(hipMemcpyAsync(out, b->d_out, nb, hipMemcpyDeviceToHost, b->s));
    HIPCHK(hipStreamSynchronize(b->s));
    b->counter = (int)(((long long)b->counter + (long long)(nitems % b->R) * b->shift) % b->R);
    return nitems;
    FDC_ENTRY_END
}

void fdc_phase_window_destroy(fdc_phase_window *b)
{
    if (!b) return;
    if (b->s) (void)hipStreamDestroy(b->s);
    delete b;
}

// fdc_fft_vcc keeps what a transform size needs — twiddle table, device buffers, a stream — in a small per-(device, n) cache: a flowgraph
// calls it item batch after item batch with the same n, and the first form (four allocations, a table rebuilt and uploaded, hipDeviceSynchronize,
// four frees per call) stalled every other stream of the device each time.  Buffers grow to the largest batch seen; at most kFftPlans sizes
// stay cached (the least recently used one goes).
}  // extern "C"
namespace {
struct FftPlan {
    int dev = 0, n = 0;
    fdc::DevBuf<float2> d_in, d_out, d_tmp, d_tw;
    size_t cap_items = 0;
    hipStream_t s = nullptr;
    unsigned long long used = 0;
    std::mutex mu;                               // one caller at a time per plan
    void release()
    {
        (void)hipSetDevice(dev);
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        d_in.release(); d_out.release(); d_tmp.release(); d_tw.release();
    }
};
constexpr size_t kFftPlans = 8;
std::mutex g_fft_mu;
// (never destroyed: the plans that are cached when the process ends are not freed behind the runtime's back — only eviction releases one)
std::vector<std::shared_ptr<FftPlan>> &g_fft_plans = *new std::vector<std::shared_ptr<FftPlan>>();
unsigned long long g_fft_tick = 0;

std::shared_ptr<FftPlan> fft_plan(int dev, int n)
{
    std::lock_guard<std::mutex> g(g_fft_mu);
    for (auto &q : g_fft_plans)
        if (q->dev == dev && q->n == n) { q->used = ++g_fft_tick; return q; }
    if (g_fft_plans.size() >= kFftPlans) {
        auto lru = std::min_element(g_fft_plans.begin(), g_fft_plans.end(), [](const auto &a, const auto &b) { return a->used < b->used; });
        std::shared_ptr<FftPlan> old = *lru;
        g_fft_plans.erase(lru);
        std::lock_guard<std::mutex> busy(old->mu);   // a caller still inside it finishes first
        old->release();
    }
    auto q = std::make_shared<FftPlan>();
    q->dev = dev; q->n = n; q->used = ++g_fft_tick;
    g_fft_plans.push_back(q);
    return q;
}
}  // namespace
extern "C" {

int fdc_fft_vcc(int device_id, int n, int forward, int shift, const void *in, int nitems, void *out)
{
    FDC_ENTRY("fdc_fft_vcc")
    if (!ispow2(n) || n < 2 || n > (1 << 24)) return set_error(FDC_ERR_INVALID_ARGUMENT, "fft size %d must be a power of two in [2, 2^24]", n);
    if (nitems <= 0) return nitems == 0 ? 0 : set_error(FDC_ERR_INVALID_ARGUMENT, "negative item count");
    if (!in || !out) return set_error(FDC_ERR_INVALID_ARGUMENT, "null buffer");
    int rc = pick_device(device_id); if (rc) return rc;
    std::shared_ptr<FftPlan> q = fft_plan(device_id, n);
    std::lock_guard<std::mutex> g(q->mu);
    HIPCHK(hipSetDevice(device_id));
    if (!q->s) HIPCHK(hipStreamCreateWithFlags(&q->s, hipStreamNonBlocking));
    if (!q->d_tw) HIPCHK(q->d_tw.upload(make_twiddles(n)));
    const size_t pts = (size_t)n * nitems, nb = sizeof(float2) * pts;
    if ((size_t)nitems > q->cap_items) {
        HIPCHK(hipStreamSynchronize(q->s));
        q->cap_items = 0;                                           // (a failure below: the next call comes here again)
        HIPCHK(q->d_in.reserve(pts, pts));
        HIPCHK(q->d_out.reserve(pts, pts));
        if (n > fdc::kMaxLdsFft) HIPCHK(q->d_tmp.reserve(pts, pts));
        q->cap_items = (size_t)nitems;
    }
    HIPCHK(hipMemcpyAsync(q->d_in, in, nb, hipMemcpyHostToDevice, q->s));
    // forward+shift: halves of the output swapped; inverse+shift: halves of the input swapped
    const int in_rot = (!forward && shift) ? n / 2 : 0, out_rot = (forward && shift) ? n / 2 : 0;
    HIPCHK(fdc::launch_fft(q->d_in, (size_t)n, q->d_out, q->d_tmp, n, nitems, !forward, in_rot, out_rot, 1.0f, q->d_tw, n, q->s, nullptr));
    HIPCHK(hipMemcpyAsync(out, q->d_out, nb, hipMemcpyDeviceToHost, q->s));
    HIPCHK(hipStreamSynchronize(q->s));
    return nitems;
    FDC_ENTRY_END
}

}  // extern "C"
