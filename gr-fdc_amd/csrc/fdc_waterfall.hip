// Waterfall rows (include/fdc_amd.h, fdc_waterfall_*): the per-block arithmetic of FDC.WaterfallMsgTagging (python/WaterfallMsgTagging.py) on
// the device.  Two stages:
//   rows of blocks  [nblocks][1024] floats, pixel p = the SUM of the power over its bins (:251-252 takes the mean of N/1024 consecutive bins; the
//                   division is left to the finish), or the bin itself where N < 1024 (:254, kron: bin p / (1024 / N)).  Written by the N = 4096
//                   one-launch kernel's epilogue (fdc_fused4096.hip, ROWS), or here from a power vector, a complex spectrum or 16-bin group powers;
//   finish          row r = the mean of the blocks [r D, (r + 1) D) of the stream (:153-164 pxupdate); the group a call leaves unfinished is carried
//                   to the next call in FP64 (ping-pong, so that the first row of a call reads the old carry while the new one is written); then
//                   digitize against the 1023 FP64 edges (:262, :285-287) and, if asked, the colour (:262 colorscheme_cols[...]).
// Every sum runs in one fixed order and in FP64: no atomics, the same bytes whatever the split into calls.
#include "../../include/fdc_amd.h"
#include "fdc_waterfall.hpp"
#include "fdc_guard.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace fdc { int set_error(int code, const char *fmt, ...); int pick_device(int device_id); }

namespace {

#define HIPCHK(expr)                                                                                              \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess) return fdc::set_error(FDC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define FDC_ENTRY(name) return fdc::guarded(name, [&]() -> int {
#define FDC_ENTRY_END });

constexpr int W = fdc::kWfWidth;
constexpr int kEdges = W - 1;     // :285 linspace(minvaldb, maxvaldb, N - 1)

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
// one thread per (block, pixel); the bins of a pixel are summed in order, in FP64
__global__ __launch_bounds__(256) void k_wf_from_power(const float *__restrict__ pw, int N, int nitems, float *__restrict__ blk)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nitems * W) return;
    const int m = (int)(i / W), p = (int)(i % W);
    const float *src = pw + (size_t)m * N;
    if (N < W) { blk[i] = src[p / (W / N)]; return; }
    const int r = N / W;
    double acc = 0.0;
    for (int j = 0; j < r; j++) acc += (double)src[(size_t)p * r + j];
    blk[i] = (float)acc;
}

__global__ __launch_bounds__(256) void k_wf_from_spectrum(const float2 *__restrict__ spec, int N, int nitems, float *__restrict__ blk)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nitems * W) return;
    const int m = (int)(i / W), p = (int)(i % W);
    const float2 *src = spec + (size_t)m * N;
    auto pw = [](float2 v) { return (double)v.x * v.x + (double)v.y * v.y; };
    if (N < W) { blk[i] = (float)pw(src[p / (W / N)]); return; }
    const int r = N / W;
    double acc = 0.0;
    for (int j = 0; j < r; j++) acc += pw(src[(size_t)p * r + j]);
    blk[i] = (float)acc;
}

// gpow[m][g] = power of shifted bins 16 g .. 16 g + 15 (fdc_pipeline_process_device_power): pixel p = groups p r .. p r + r - 1, r = N / 16384
__global__ __launch_bounds__(256) void k_wf_from_groups(const float *__restrict__ gpow, int N, int nitems, float *__restrict__ blk)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nitems * W) return;
    const int m = (int)(i / W), p = (int)(i % W), r = N / (16 * W);
    const float *src = gpow + (size_t)m * (N / 16) + (size_t)p * r;
    double acc = 0.0;
    for (int j = 0; j < r; j++) acc += (double)src[j];
    blk[i] = (float)acc;
}

// grid (1024 / 256, min(nrows + 1, kFinishGridY)); row k = blockIdx.y, blockIdx.y + gridDim.y, ...: k < nrows finishes row k of the call, k = nrows
// writes the new carry.  c0 = blocks in the old carry; row 0 takes the old carry and the call's first D - c0 blocks, row k > 0 the blocks
// D - c0 + (k - 1) D ...; the carry takes what is left.  The edges and the colour table are staged in LDS (the digitize is a binary search over
// them); a workgroup's 256 colours go through LDS to 192 dword stores.
constexpr int kFinishGridY = 4096;
__global__ __launch_bounds__(256) void k_wf_finish(const float *__restrict__ blk, int nblk, int D, int c0, int nrows, double div,
                                                   const double *__restrict__ carry_in, double *__restrict__ carry_out,
                                                   const double *__restrict__ edges, int increasing, const uint8_t *__restrict__ table,
                                                   float *__restrict__ rows, uint16_t *__restrict__ index, uint8_t *__restrict__ rgb)
{
    __shared__ double s_edges[kEdges];
    __shared__ uint8_t s_table[3 * W];
    __shared__ uint32_t s_rgb[3 * 256 / 4];
    const int t = threadIdx.x, p = blockIdx.x * 256 + t;
    for (int i = t; i < kEdges; i += 256) s_edges[i] = edges[i];
    if (rgb)
        for (int i = t; i < 3 * W; i += 256) s_table[i] = table[i];
    __syncthreads();
    // k, nrows and rgb are uniform over the workgroup: the barriers below are reached by all of its threads or by none
    for (int k = blockIdx.y; k <= nrows; k += gridDim.y) {
        const int b0 = k == 0 ? 0 : D - c0 + (k - 1) * D;
        const int nb = k == nrows ? nblk - b0 : (k == 0 ? D - c0 : D);
        double acc = k == 0 ? carry_in[p] : 0.0;
        for (int j = 0; j < nb; j++) acc += (double)blk[(size_t)(b0 + j) * W + p];
        if (k == nrows) { carry_out[p] = acc; continue; }
        const float v = (float)(acc / div);
        const double x = (double)v;
        // numpy.digitize(x, bins, right = False): increasing bins -> the number of edges <= x (NaN: all of them), decreasing -> the number > x
        int lo = 0, hi = kEdges;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const bool below = increasing ? s_edges[mid] <= x : s_edges[mid] > x;
            if (below) lo = mid + 1; else hi = mid;
        }
        const int idx = (increasing && x != x) ? kEdges : lo;
        const size_t o = (size_t)k * W + p;
        if (rows) rows[o] = v;
        if (index) index[o] = (uint16_t)idx;
        if (rgb) {
            uint8_t *sb = reinterpret_cast<uint8_t *>(s_rgb);
            sb[3 * t] = s_table[3 * idx]; sb[3 * t + 1] = s_table[3 * idx + 1]; sb[3 * t + 2] = s_table[3 * idx + 2];
            __syncthreads();
            // 3 x 256 bytes from byte 3 ((size_t)k W + 256 blockIdx.x): a multiple of 768, so dword aligned
            if (t < 3 * 256 / 4) reinterpret_cast<uint32_t *>(rgb + 3 * ((size_t)k * W + (size_t)blockIdx.x * 256))[t] = s_rgb[t];
            __syncthreads();
        }
    }
}

inline unsigned grid_of(int nitems) { return (unsigned)(((long long)nitems * W + 255) / 256); }

// ---- host tables --------------------------------------------------------------------------------------------------------------------
// numpy.linspace(start, stop, num) (float64: start + i * step, the last point = stop exactly; step == 0: i / div * delta)
void linspace(double start, double stop, int num, double *y)
{
    const int div = num - 1;
    const double delta = stop - start, step = delta / div;
    for (int i = 0; i < num; i++) y[i] = step == 0 ? (double)i / div * delta + start : (double)i * step + start;
    if (num > 1) y[num - 1] = stop;
}
// numpy.linspace(a, b, n, dtype = uint8): the float64 points truncated (all >= 0 here, so floor and truncation agree)
void lsp_u8(int a, int b, int n, uint8_t *dst, int stride)
{
    std::vector<double> y((size_t)n);
    linspace(a, b, n, y.data());
    for (int i = 0; i < n; i++) dst[(size_t)i * stride] = (uint8_t)(int)y[(size_t)i];
}
void fill(uint8_t v, int n, uint8_t *dst, int stride) { for (int i = 0; i < n; i++) dst[(size_t)i * stride] = v; }

// cr_colorscheme (:276-312): columns R, G, B of 1024 colours
void color_table(int scheme, uint8_t *t, uint8_t *frame)
{
    uint8_t *r = t, *g = t + 1, *b = t + 2;
    frame[0] = 255; frame[1] = 255; frame[2] = 255;
    if (scheme == 1) {              // black-rainbow, four quarters
        const int q = W / 4;
        lsp_u8(0, 75, q, r, 3); lsp_u8(75, 0, q, r + 3 * q, 3); fill(0, q, r + 6 * q, 3); lsp_u8(0, 255, q, r + 9 * q, 3);
        fill(0, 2 * q, g, 3); lsp_u8(0, 255, q, g + 6 * q, 3); fill(255, q, g + 9 * q, 3);
        lsp_u8(0, 130, q, b, 3); lsp_u8(130, 255, q, b + 3 * q, 3); lsp_u8(255, 0, q, b + 6 * q, 3); fill(0, q, b + 9 * q, 3);
    } else if (scheme == 2) {       // black-red-yellow, two halves
        const int h = W / 2;
        lsp_u8(0, 255, h, r, 3); fill(255, h, r + 3 * h, 3);
        fill(0, h, g, 3); lsp_u8(0, 255, h, g + 3 * h, 3);
        fill(0, W, b, 3);
    } else if (scheme == 3) {       // black-white, green frame
        lsp_u8(0, 255, W, r, 3); lsp_u8(0, 255, W, g, 3); lsp_u8(0, 255, W, b, 3);
        frame[0] = 0; frame[2] = 0;
    } else {                        // black-blue-cyan-white (and every unknown scheme)
        const int h = W / 2;
        fill(0, W, r, 3);
        fill(0, h, g, 3); lsp_u8(0, 255, h, g + 3 * h, 3);
        lsp_u8(0, 255, h, b, 3); fill(255, h, b + 3 * h, 3);
    }
}

void edges_of(int loginput, double minvaldb, double maxvaldb, double *e)
{
    linspace(minvaldb, maxvaldb, kEdges, e);
    if (!loginput)
        for (int i = 0; i < kEdges; i++) e[i] = std::pow(10.0, e[i] / 10.0);
}

bool blocklen_ok(int N) { return N >= 1 && N <= (1 << 24) && (N % W == 0 || W % N == 0); }

}  // namespace

struct fdc_waterfall {
    fdc_waterfall_cfg cfg{};
    int dev = 0, max_items = 0;
    hipStream_t stream = nullptr;
    double *d_edges = nullptr;
    int increasing = 1;
    uint8_t *d_table = nullptr;
    float *d_blk = nullptr;          // [max_items][1024] row sums of the blocks of a call
    float *d_pow = nullptr;          // fdc_waterfall_work: [max_items][N] input powers (at the first call)
    float *d_gpow = nullptr;         // pipeline, group-sum route: [max_items][N / 16] (at the first call)
    double *d_carry[2] = {nullptr, nullptr};
    int carry_sel = 0, carry_n = 0;  // which buffer holds the carry, how many blocks are in it
    int64_t rows_done = 0;
    float *d_rows = nullptr;         // [max_items] rows of one pass
    uint16_t *d_index = nullptr;
    uint8_t *d_rgb = nullptr;
};

namespace {

int upload_levels(fdc_waterfall *w)
{
    double e[kEdges];
    edges_of(w->cfg.loginput, w->cfg.minvaldb, w->cfg.maxvaldb, e);
    // numpy's monotonicity test: non-decreasing (equal edges included) is increasing
    w->increasing = !(e[0] > e[kEdges - 1]);
    HIPCHK(hipSetDevice(w->dev));
    HIPCHK(hipMemcpy(w->d_edges, e, sizeof e, hipMemcpyHostToDevice));
    return FDC_OK;
}

int upload_scheme(fdc_waterfall *w)
{
    uint8_t t[3 * W], fr[3];
    color_table(w->cfg.colorscheme, t, fr);
    HIPCHK(hipSetDevice(w->dev));
    HIPCHK(hipMemcpy(w->d_table, t, sizeof t, hipMemcpyHostToDevice));
    return FDC_OK;
}

int rows_of(const fdc_waterfall *w, int nblocks) { return (w->carry_n + nblocks) / w->cfg.blockdecimation; }

}  // namespace

namespace fdc {

int wf_check_call(const fdc_waterfall *w, int device_id, int N, int nblocks, int cap_rows)
{
    if (!w) return set_error(FDC_ERR_INVALID_ARGUMENT, "null waterfall handle");
    if (w->dev != device_id || w->cfg.blocklen != N)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the waterfall (device %d, blocklen %d) does not match the pipeline (device %d, blocklen %d)",
                         w->dev, w->cfg.blocklen, device_id, N);
    if (nblocks > w->max_items) return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d above the waterfall's max_items %d", nblocks, w->max_items);
    if (rows_of(w, nblocks) > cap_rows) return set_error(FDC_ERR_INVALID_ARGUMENT, "the call finishes %d rows, cap_rows is %d", rows_of(w, nblocks), cap_rows);
    return FDC_OK;
}

float *wf_block_rows(fdc_waterfall *w) { return w->d_blk; }

int wf_group_buffer(fdc_waterfall *w, int nblocks, float **out)
{
    if (nblocks > w->max_items) return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d above max_items %d", nblocks, w->max_items);
    if (!w->d_gpow) HIPCHK(hipMalloc(&w->d_gpow, sizeof(float) * (size_t)w->max_items * (w->cfg.blocklen / 16)));
    *out = w->d_gpow;
    return FDC_OK;
}

hipError_t wf_rows_from_spectrum(fdc_waterfall *w, const float2 *spec, int nblocks, hipStream_t s)
{
    hipLaunchKernelGGL(k_wf_from_spectrum, dim3(grid_of(nblocks)), dim3(256), 0, s, spec, w->cfg.blocklen, nblocks, w->d_blk);
    return hipGetLastError();
}

hipError_t wf_rows_from_groups(fdc_waterfall *w, const float *gpow, int nblocks, hipStream_t s)
{
    hipLaunchKernelGGL(k_wf_from_groups, dim3(grid_of(nblocks)), dim3(256), 0, s, gpow, w->cfg.blocklen, nblocks, w->d_blk);
    return hipGetLastError();
}

int wf_finish(fdc_waterfall *w, int nblocks, hipStream_t s, float *rows, uint16_t *index, uint8_t *rgb, int32_t *nrows)
{
    const int D = w->cfg.blockdecimation, n = rows_of(w, nblocks);
    const double div = (double)D * (w->cfg.blocklen >= W ? w->cfg.blocklen / W : 1);
    hipLaunchKernelGGL(k_wf_finish, dim3(W / 256, (unsigned)std::min(n + 1, kFinishGridY)), dim3(256), 0, s, w->d_blk, nblocks, D, w->carry_n, n, div,
                       w->d_carry[w->carry_sel], w->d_carry[w->carry_sel ^ 1], w->d_edges, w->increasing, w->d_table,
                       rows ? w->d_rows : nullptr, index ? w->d_index : nullptr, rgb ? w->d_rgb : nullptr);
    HIPCHK(hipGetLastError());
    if (n > 0) {
        if (rows) HIPCHK(hipMemcpyAsync(rows, w->d_rows, sizeof(float) * (size_t)n * W, hipMemcpyDeviceToHost, s));
        if (index) HIPCHK(hipMemcpyAsync(index, w->d_index, sizeof(uint16_t) * (size_t)n * W, hipMemcpyDeviceToHost, s));
        if (rgb) HIPCHK(hipMemcpyAsync(rgb, w->d_rgb, (size_t)3 * n * W, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    w->carry_sel ^= 1;
    w->carry_n = (w->carry_n + nblocks) % D;
    w->rows_done += n;
    if (nrows) *nrows = n;
    return FDC_OK;
}

}  // namespace fdc

extern "C" {

int fdc_waterfall_check(const fdc_waterfall_cfg *cfg, fdc_waterfall_cfg *normalized)
{
    FDC_ENTRY("fdc_waterfall_check")
    if (!cfg) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null configuration");
    if (!blocklen_ok(cfg->blocklen))
        return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "blocklen %d: a waterfall row needs a multiple of 1024 or a divisor of 1024", cfg->blocklen);
    if (!std::isfinite(cfg->minvaldb) || !std::isfinite(cfg->maxvaldb)) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "levels must be finite");
    if (normalized) {
        *normalized = *cfg;
        if (normalized->blockdecimation <= 0) normalized->blockdecimation = 1;
    }
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_waterfall_color_table(int32_t scheme, uint8_t *rgb, uint8_t *frame)
{
    FDC_ENTRY("fdc_waterfall_color_table")
    if (!rgb && !frame) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null buffers");
    uint8_t t[3 * W], fr[3];
    color_table(scheme, t, fr);
    if (rgb) std::memcpy(rgb, t, sizeof t);
    if (frame) std::memcpy(frame, fr, sizeof fr);
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_waterfall_edges(int32_t loginput, double minvaldb, double maxvaldb, double *edges)
{
    if (!edges) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null buffer");
    edges_of(loginput, minvaldb, maxvaldb, edges);
    return FDC_OK;
}

void fdc_waterfall_destroy(fdc_waterfall *w)
{
    if (!w) return;
    (void)hipSetDevice(w->dev);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    for (void *ptr : {(void *)w->d_edges, (void *)w->d_table, (void *)w->d_blk, (void *)w->d_pow, (void *)w->d_gpow, (void *)w->d_carry[0],
                      (void *)w->d_carry[1], (void *)w->d_rows, (void *)w->d_index, (void *)w->d_rgb})
        if (ptr) (void)hipFree(ptr);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;
}

int fdc_waterfall_create(int device_id, const fdc_waterfall_cfg *cfg, int32_t max_items, fdc_waterfall **out)
{
    FDC_ENTRY("fdc_waterfall_create")
    if (!out) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    fdc_waterfall_cfg c{};
    int rc = fdc_waterfall_check(cfg, &c);
    if (rc != FDC_OK) return rc;
    if (max_items < 1) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "max_items %d < 1", max_items);
    if ((int64_t)max_items * c.blocklen > (1ll << 31)) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "max_items x blocklen above 2^31 samples");
    if ((rc = fdc::pick_device(device_id)) != FDC_OK) return rc;
    fdc_waterfall *w = new fdc_waterfall;
    w->cfg = c; w->dev = device_id; w->max_items = max_items;
    auto body = [&]() -> int {
        HIPCHK(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
        HIPCHK(hipMalloc(&w->d_edges, sizeof(double) * kEdges));
        HIPCHK(hipMalloc(&w->d_table, 3 * W));
        HIPCHK(hipMalloc(&w->d_blk, sizeof(float) * (size_t)max_items * W));
        for (auto &d : w->d_carry) { HIPCHK(hipMalloc(&d, sizeof(double) * W)); HIPCHK(hipMemset(d, 0, sizeof(double) * W)); }
        HIPCHK(hipMalloc(&w->d_rows, sizeof(float) * (size_t)max_items * W));
        HIPCHK(hipMalloc(&w->d_index, sizeof(uint16_t) * (size_t)max_items * W));
        HIPCHK(hipMalloc(&w->d_rgb, (size_t)3 * max_items * W));
        int r = upload_levels(w);
        return r != FDC_OK ? r : upload_scheme(w);
    };
    if ((rc = body()) != FDC_OK) { fdc_waterfall_destroy(w); return rc; }
    *out = w;
    return FDC_OK;
    FDC_ENTRY_END
}

void fdc_waterfall_reset(fdc_waterfall *w)
{
    if (!w) return;
    // row 0 of the next call starts from the carry: both buffers <- 0 (a call that ends on a row boundary leaves a zero carry the same way)
    w->carry_n = 0;
    w->rows_done = 0;
    (void)hipSetDevice(w->dev);
    for (auto &d : w->d_carry) (void)hipMemsetAsync(d, 0, sizeof(double) * W, w->stream);
    (void)hipStreamSynchronize(w->stream);
}

int fdc_waterfall_set_levels(fdc_waterfall *w, double minvaldb, double maxvaldb)
{
    FDC_ENTRY("fdc_waterfall_set_levels")
    if (!w) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!std::isfinite(minvaldb) || !std::isfinite(maxvaldb)) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "levels must be finite");
    w->cfg.minvaldb = minvaldb; w->cfg.maxvaldb = maxvaldb;
    return upload_levels(w);
    FDC_ENTRY_END
}

int fdc_waterfall_set_colorscheme(fdc_waterfall *w, int32_t scheme)
{
    FDC_ENTRY("fdc_waterfall_set_colorscheme")
    if (!w) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    w->cfg.colorscheme = scheme;
    return upload_scheme(w);
    FDC_ENTRY_END
}

int64_t fdc_waterfall_rows_done(const fdc_waterfall *w) { return w ? w->rows_done : -1; }

int fdc_waterfall_work(fdc_waterfall *w, const float *power, int nitems, float *rows, uint16_t *index, uint8_t *rgb, int cap_rows, int32_t *nrows)
{
    FDC_ENTRY("fdc_waterfall_work")
    if (!w) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (nitems < 0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "negative item count");
    if (nitems > 0 && !power) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null input");
    const int total = rows_of(w, nitems);
    if (total > cap_rows) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "the call finishes %d rows, cap_rows is %d", total, cap_rows);
    HIPCHK(hipSetDevice(w->dev));
    const int N = w->cfg.blocklen;
    if (nitems > 0 && !w->d_pow) HIPCHK(hipMalloc(&w->d_pow, sizeof(float) * (size_t)w->max_items * N));
    int done = 0;
    for (int m0 = 0; m0 < nitems; m0 += w->max_items) {
        const int nb = std::min(w->max_items, nitems - m0);
        HIPCHK(hipMemcpyAsync(w->d_pow, power + (size_t)m0 * N, sizeof(float) * (size_t)nb * N, hipMemcpyHostToDevice, w->stream));
        hipLaunchKernelGGL(k_wf_from_power, dim3(grid_of(nb)), dim3(256), 0, w->stream, w->d_pow, N, nb, w->d_blk);
        HIPCHK(hipGetLastError());
        int32_t got = 0;
        const int rc = fdc::wf_finish(w, nb, w->stream, rows ? rows + (size_t)done * W : nullptr, index ? index + (size_t)done * W : nullptr,
                                      rgb ? rgb + (size_t)3 * done * W : nullptr, &got);
        if (rc != FDC_OK) return rc;
        done += got;
    }
    if (nrows) *nrows = done;
    return nitems;
    FDC_ENTRY_END
}

}  // extern "C"
