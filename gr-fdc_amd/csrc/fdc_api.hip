// C-ABI of the MI355X frequency-domain channelizer (include/fdc_amd.h): the library's plumbing and the pipeline handle's life, accessors and
// settings (fdc_pipeline.hpp says where the rest is).  No CPU compute fallback exists: without a HIP device every create() fails.
#include "fdc_pipeline.hpp"

#include <cstdarg>
#include <stdexcept>
#include <system_error>

using namespace fdc::pipe;

namespace {

thread_local std::string g_err;

// Host ranges the caller pinned with fdc_host_register(): work() DMAs them directly; anything else goes through
// the handle's own pinned staging buffers.
struct HostRange { uintptr_t lo, hi, dev; };   // dev: device-side address of lo
std::mutex g_reg_mu;
std::vector<HostRange> g_reg;

}  // namespace

namespace fdc {
// Environment variables are a debugging override only: nothing is read unless FDC_DEBUG_ENV=1 (include/fdc_amd.h)
const char *debug_env(const char *name)
{
    static const bool on = [] { const char *d = getenv("FDC_DEBUG_ENV"); return d && d[0] == '1'; }();
    return on ? getenv(name) : nullptr;
}
// the text of fdc_last_error(), for every file of the library
int set_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int pick_device(int device_id)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_error(FDC_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= n) return set_error(FDC_ERR_INVALID_ARGUMENT, "device_id %d out of range [0,%d)", device_id, n);
    HIPCHK(hipSetDevice(device_id));
    // the dynamic-LDS limits are function attributes PER DEVICE: set once for every device a handle is opened on
    static std::mutex mu;
    static std::vector<char> ready;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)ready.size() < n) ready.resize((size_t)n, 0);
    if (!ready[(size_t)device_id]) {
        const hipError_t e = fdc::init_kernels();
        if (e != hipSuccess) return set_error(FDC_ERR_HIP, "kernel attribute setup failed: %s", hipGetErrorString(e));
        ready[(size_t)device_id] = 1;
    }
    return FDC_OK;
}

namespace pipe {
std::vector<float2> make_twiddles(int n)
{
    std::vector<float2> t(n);
    for (int k = 0; k < n; k++) {
        const double a = -2.0 * M_PI * double(k) / double(n);
        t[k] = make_float2(float(std::cos(a)), float(std::sin(a)));
    }
    return t;
}

bool host_registered(const void *ptr, size_t bytes, void **devptr)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (const HostRange &r : g_reg)
        if (a >= r.lo && a + bytes <= r.hi) {
            if (devptr) *devptr = reinterpret_cast<void *>(r.dev + (a - r.lo));
            return true;
        }
    return false;
}

// the float results of the host entries, and the staging of integer output where the kernels do not narrow themselves
int out_staging(fdc_pipeline *p)
{
    if (p->sum_lout > 0 && !p->d_out) HIPCHK(p->d_out.alloc((size_t)p->cfg.max_blocks * p->sum_lout));
    return FDC_OK;
}
}  // namespace pipe
}  // namespace fdc

namespace fdc {
// for fdc_group.hip: a member's output format (FDC_OQ_*) and scale — the group places its spans by the members' own setting
int pipeline_output_format(const fdc_pipeline *p, float *scale)
{
    if (scale) *scale = p->out_scale;
    return p->out_form;
}
}  // namespace fdc

extern "C" {

const char *fdc_last_error(void) { return g_err.c_str(); }
const char *fdc_version(void) { return "gr-fdc_amd 0.1 (gfx950)"; }

int fdc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fdc_selftest_exception_barrier(void)
{
    struct Case { int kind, want; };
    const Case cases[] = {{0, FDC_ERR_NOMEM}, {1, FDC_ERR_NOMEM}, {2, FDC_ERR_HIP}, {3, FDC_ERR_HIP}, {4, 7}};
    for (const Case &c : cases) {
        const int got = fdc::guarded("fdc_selftest_exception_barrier", [&]() -> int {
            switch (c.kind) {
            case 0: throw std::bad_alloc();
            case 1: throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again), "thread");
            case 2: throw std::runtime_error("runtime");
            case 3: throw 42;
            default: return 7;                                     // nothing thrown: the body's own status passes through
            }
        });
        if (got != c.want) return set_error(FDC_ERR_HIP, "exception barrier: kind %d came back as %d, expected %d", c.kind, got, c.want);
        if (c.want < 0 && g_err.empty()) return set_error(FDC_ERR_HIP, "exception barrier: kind %d left no text", c.kind);
    }
    return FDC_OK;
}

int fdc_selftest_devices(void)
{
    FDC_ENTRY("fdc_selftest_devices")
    const int ndev = fdc_device_count();
    if (ndev <= 0) return set_error(FDC_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    constexpr int N = 65536, R = 2, C = 256, NB = 96, H = N - N / R, LOUT = 128;
    std::vector<fdc_channel> ch(C);
    for (int c = 0; c < C; c++) ch[(size_t)c] = fdc_channel{256 * c, 256, 0.88f, 1.0f};
    std::vector<float> x((size_t)2 * NB * H);
    uint32_t lcg = 12345u;
    for (float &v : x) { lcg = lcg * 1664525u + 1013904223u; v = (float)((int32_t)(lcg >> 8) - (1 << 23)) * (1.0f / (1 << 23)); }
    std::vector<std::vector<float>> out((size_t)C, std::vector<float>((size_t)2 * NB * LOUT));
    std::vector<void *> outs((size_t)C);
    for (int c = 0; c < C; c++) outs[(size_t)c] = out[(size_t)c].data();
    uint64_t ref = 0;
    auto checksum = [&](double *energy) {                          // FNV-1a over every output byte
        uint64_t h = 1469598103934665603ull;
        *energy = 0.0;
        for (int c = 0; c < C; c++) {
            const unsigned char *b = reinterpret_cast<const unsigned char *>(out[(size_t)c].data());
            for (size_t i = 0; i < out[(size_t)c].size() * sizeof(float); i++) { h ^= b[i]; h *= 1099511628211ull; }
            for (float v : out[(size_t)c]) *energy += (double)v * v;
        }
        return h;
    };
    fdc_pipeline_cfg cfg{};
    cfg.blocklen = N; cfg.relinvovl = R; cfg.windowtype = FDC_WIN_HANN; cfg.nchannels = C; cfg.channels = ch.data();
    cfg.max_blocks = NB; cfg.host_sub_blocks = NB;
    cfg.min_block_launch = 1;          // the one-kernel form whatever the launch length: the group's members get NB / ndev blocks each
    for (int d = 0; d < ndev; d++) {
        cfg.device_id = d;
        fdc_pipeline *p = nullptr;
        int rc = fdc_pipeline_create(&cfg, &p);
        if (rc != FDC_OK) return set_error(rc, "selftest: device %d: create failed: %s", d, std::string(g_err).c_str());
        if (fdc_pipeline_path(p) != 3) { fdc_pipeline_destroy(p); return set_error(FDC_ERR_UNSUPPORTED, "selftest: device %d: not on the one-kernel path", d); }
        rc = fdc_pipeline_work(p, x.data(), NB, outs.data(), nullptr);
        fdc_pipeline_destroy(p);
        if (rc != NB) return set_error(rc < 0 ? rc : FDC_ERR_HIP, "selftest: device %d: work failed: %s", d, std::string(g_err).c_str());
        double energy = 0.0;
        const uint64_t h = checksum(&energy);
        if (!(energy > 0.0)) return set_error(FDC_ERR_HIP, "selftest: device %d produced no output", d);
        if (d == 0) ref = h;
        else if (h != ref) return set_error(FDC_ERR_HIP, "selftest: device %d differs from device 0 (checksum %016llx vs %016llx)", d,
                                       (unsigned long long)h, (unsigned long long)ref);
    }
    // the multi-device handle over ALL visible devices (one device: two virtual members on it), the same call in two pieces so
    // that the second piece's first span takes its halo from the group's history: one work() spread over the node must give
    // device 0's bytes
    {
        std::vector<int32_t> devs;
        for (int d = 0; d < std::max(ndev, 2); d++) devs.push_back(d % ndev);
        fdc_pipeline_group *g = nullptr;
        int rc = fdc_pipeline_group_create(&cfg, devs.data(), (int)devs.size(), 4, &g);
        if (rc != FDC_OK) return set_error(rc, "selftest: group over %d device(s): create failed: %s", ndev, std::string(g_err).c_str());
        for (auto &o : out) std::fill(o.begin(), o.end(), 0.0f);
        const int n1 = NB / 3, n2 = NB - n1;
        std::vector<void *> outs2((size_t)C);
        for (int c = 0; c < C; c++) outs2[(size_t)c] = out[(size_t)c].data() + (size_t)2 * n1 * LOUT;
        rc = fdc_pipeline_group_work(g, x.data(), n1, outs.data(), nullptr);
        if (rc == n1) rc = fdc_pipeline_group_work(g, x.data() + (size_t)2 * n1 * H, n2, outs2.data(), nullptr);
        fdc_pipeline_group_destroy(g);
        if (rc != n2) return set_error(rc < 0 ? rc : FDC_ERR_HIP, "selftest: group over %d device(s): work failed: %s", ndev, std::string(g_err).c_str());
        double energy = 0.0;
        const uint64_t h = checksum(&energy);
        if (h != ref) return set_error(FDC_ERR_HIP, "selftest: the group over %d device(s) differs from device 0 (checksum %016llx vs %016llx)", ndev,
                                  (unsigned long long)h, (unsigned long long)ref);
    }
    return ndev;
    FDC_ENTRY_END
}

int fdc_window_table(int windowtype, int blocklen, float passbw, float stopbw, int numphasestates, int step,
                     int normalize, float *w)
{
    FDC_ENTRY("fdc_window_table")
    if (blocklen < 1 || numphasestates < 1 || !w) return set_error(FDC_ERR_INVALID_ARGUMENT, "bad window table arguments");
    fdc::window_table(windowtype, blocklen, passbw, stopbw, numphasestates, step, normalize != 0,
                      reinterpret_cast<std::complex<float> *>(w));
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_host_register(void *ptr, size_t bytes)
{
    FDC_ENTRY("fdc_host_register")
    if (!ptr || !bytes) return set_error(FDC_ERR_INVALID_ARGUMENT, "fdc_host_register: empty range");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_error(FDC_ERR_NO_DEVICE, "no HIP device visible");
    HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    void *dev = nullptr;
    hipError_t e = hipHostGetDevicePointer(&dev, ptr, 0);
    if (e != hipSuccess) { (void)hipHostUnregister(ptr); return set_error(FDC_ERR_HIP, "hipHostGetDevicePointer failed: %s", hipGetErrorString(e)); }
    const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_reg.push_back(HostRange{a, a + bytes, reinterpret_cast<uintptr_t>(dev)});
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_host_unregister(void *ptr)
{
    FDC_ENTRY("fdc_host_unregister")
    const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        auto it = std::find_if(g_reg.begin(), g_reg.end(), [a](const HostRange &r) { return r.lo == a; });
        if (it == g_reg.end()) return set_error(FDC_ERR_INVALID_ARGUMENT, "fdc_host_unregister: range was not registered here");
        g_reg.erase(it);
    }
    HIPCHK(hipHostUnregister(ptr));
    return FDC_OK;
    FDC_ENTRY_END
}

void fdc_pipeline_destroy(fdc_pipeline *p)
{
    if (!p) return;
    // what has an order: nothing of the handle's runs any more, its events and streams go, then `delete` frees the buffers (fdc_buffers.hpp)
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    if (p->ev_hier) { (void)hipEventSynchronize(p->ev_hier); (void)hipEventDestroy(p->ev_hier); }   // kernels of the pipelined entry ran on the bank's stream
    for (auto st : {p->s_in, p->s_out}) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (auto e : p->events) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; i++)
        for (auto e : {p->ev_in[i], p->ev_k[i], p->ev_out[i]}) if (e) (void)hipEventDestroy(e);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

int fdc_pipeline_create(const fdc_pipeline_cfg *cfg, fdc_pipeline **out)
{
    FDC_ENTRY("fdc_pipeline_create")
    if (!cfg || !out) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    int rc = validate_cfg(cfg);
    if (rc != FDC_OK) return rc;
    rc = pick_device(cfg->device_id);
    if (rc != FDC_OK) return rc;

    fdc_pipeline *p = new fdc_pipeline();
    struct Owner { fdc_pipeline *p; ~Owner() { if (p) fdc_pipeline_destroy(p); } } owner{p};   // error returns and exceptions free the handle
    const int N = cfg->blocklen, R = cfg->relinvovl;
    p->cfg = *cfg; p->cfg.channels = nullptr;
    p->N = N; p->R = R; p->ovl = N / R; p->H = N - p->ovl; p->C = cfg->nchannels;
    std::vector<std::complex<float>> pool;
    build_channel_records(p, cfg, pool);

    const int flags = effective_flags(cfg->flags);
    p->cfg.flags = flags;
    p->cfg_generic = (flags & FDC_PIPE_FORCE_GENERIC) != 0;
    p->block_hints = ((flags & FDC_PIPE_PLAIN_STORES) ? 0 : 1) | ((flags & FDC_PIPE_NT_LOADS) ? 2 : 0);
    if (cfg->min_block_launch >= 1) p->block_min = cfg->min_block_launch;
    if (const char *bm = fdc::debug_env("FDC_BLOCK_MIN_BLOCKS")) if (atoi(bm) >= 1) p->block_min = atoi(bm);

    std::vector<int32_t> flat, rflat;
    group_by_width(p, nullptr, p->groups, p->group_off, p->g_aligned, p->g_out_aligned, flat);
    classify_plan(p, cfg, flags);
    if (p->split) group_by_width(p, &p->rem, p->rgroups, p->rgroup_off, p->rg_aligned, p->rg_out_aligned, rflat);

    // launch groups.  Measured on MI355X (profiles/r01_*): with one stream, short launches (few tiles per
    // persistent workgroup) cost more than cache residency of the intermediates gains, on both paths, so the
    // default takes groups as large as a 2 GiB scratch budget allows (1024 blocks at N = 65536).
    int chunk = cfg->chunk_blocks;
    if (chunk <= 0) chunk = (int)std::max<int64_t>(1, (2048ll << 20) / (2ll * N * 8));
    p->chunk = std::min(chunk, cfg->max_blocks);

    rc = build_device_state(p, cfg, pool, flat, rflat);
    if (rc != FDC_OK) return rc;
    owner.p = nullptr;
    *out = p;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_plan_preview(const fdc_pipeline_cfg *cfg, char *buf, int32_t n, int32_t *assignment)
{
    FDC_ENTRY("fdc_pipeline_plan_preview")
    if (!cfg) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    const int rc = validate_cfg(cfg);
    if (rc != FDC_OK) return rc;
    // steps 1 - 3 of fdc_pipeline_create on a handle that never touches a device (no stream, no tables): host code only
    std::unique_ptr<fdc_pipeline> p(new fdc_pipeline());
    p->cfg = *cfg; p->cfg.channels = nullptr;
    p->N = cfg->blocklen; p->R = cfg->relinvovl; p->ovl = p->N / p->R; p->H = p->N - p->ovl; p->C = cfg->nchannels;
    std::vector<std::complex<float>> pool;
    build_channel_records(p.get(), cfg, pool);
    const int flags = effective_flags(cfg->flags);
    p->cfg.flags = flags;
    p->cfg_generic = (flags & FDC_PIPE_FORCE_GENERIC) != 0;
    classify_plan(p.get(), cfg, flags);
    if (assignment) {
        for (int c = 0; c < p->C; c++) assignment[c] = -1;
        for (size_t k = 0; k < p->banks.size(); k++) for (int c : p->banks[k].chan) assignment[c] = (int32_t)k;
        for (const auto &al : p->bank_alias) assignment[al.first] = -2 - al.second;
    }
    if (buf && n > 0) fdc_pipeline_describe(p.get(), buf, n);
    return fdc_pipeline_path(p.get());
    FDC_ENTRY_END
}

int64_t fdc_pipeline_input_samples(const fdc_pipeline *p, int nblocks) { return p ? (int64_t)nblocks * p->H : 0; }
int64_t fdc_pipeline_output_samples(const fdc_pipeline *p, int nblocks) { return p ? (int64_t)nblocks * p->sum_lout : 0; }
int64_t fdc_pipeline_channel_offset(const fdc_pipeline *p, int c, int nblocks)
{
    if (!p || c < 0 || c >= p->C) return -1;
    return (int64_t)nblocks * p->chans[c].out_off;
}
int32_t fdc_pipeline_channel_lout(const fdc_pipeline *p, int c)
{
    if (!p || c < 0 || c >= p->C) return -1;
    return p->chans[c].lout;
}
void *fdc_pipeline_stream(fdc_pipeline *p) { return p ? (void *)p->stream : nullptr; }
int fdc_pipeline_reserve_compute_units(fdc_pipeline *p, int32_t n)
{
    FDC_ENTRY("fdc_pipeline_reserve_compute_units")
    if (!p) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || n >= p->ncu) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "%d compute units of %d cannot be left out", (int)n, p->ncu);
    p->reserved_cu = n;
    p->reserve_user = n > 0;
    return p->ncu - n;
    FDC_ENTRY_END
}
int32_t fdc_pipeline_chunk_blocks(const fdc_pipeline *p) { return p ? p->chunk : -1; }
int32_t fdc_pipeline_path(const fdc_pipeline *p)
{
    if (!p) return -1;
    if (p->fused) return 5;
    if (p->poly_block && p->split) return 4;
    if (p->poly_block) return 3;
    if (p->poly_ok) return 2;
    if (p->fwd_block || (p->N == 65536 && !p->cfg_generic)) return 1;
    return 0;
}

int32_t fdc_pipeline_describe(const fdc_pipeline *p, char *buf, int32_t n)
{
    if (!p || !buf || n < 1) return -1;
    char t[640];
    const int path = fdc_pipeline_path(p);
    int k = std::snprintf(t, sizeof(t), "N = %d, R = %d, %d channels; path %d: ", p->N, p->R, p->C, path);
    auto add = [&](const char *fmt, auto... a) { if (k < (int)sizeof(t)) k += std::snprintf(t + k, sizeof(t) - (size_t)k, fmt, a...); };
    auto kernel = [](int L) { return L == 256 ? "k_blk256" : L == 512 ? "k_blk512" : L == 1024 ? "k_blk1024" : "k_blknar"; };
    auto where = [](int L, int r) { return r == 0 ? "on the grid" : 2 * r == L ? "half a channel off the grid" : 4 * r == L ? "a quarter of a channel off the grid" : "three quarters of a channel off the grid"; };
    if (p->fused) {
        int nw = 0;
        for (const auto &w : p->f4_wave) nw += !w.empty();
        add("k_f4096, transform + %d channel transforms in one launch (spectrum in LDS, %s per workgroup, rows on %d wave%s)", p->C,
            p->f4_teams == 1 ? "one block" : "two blocks", nw, nw == 1 ? "" : "s");
    } else if (p->poly_block) {
        bool one_width = true, all256 = true;
        for (const auto &b : p->banks) { one_width = one_width && b.L == p->banks[0].L; all256 = all256 && b.L == 256; }
        if (all256) {
            add("k_blk256, %d tiling%s (r =", (int)p->banks.size(), p->banks.size() == 1 ? "" : "s");
            for (const auto &b : p->banks) add(" %d", b.r);
            add("%s", ")");
        } else if (one_width) {
            add("%s, l = %d, bank of %d %s", kernel(p->banks[0].L), p->banks[0].L, (int)p->banks[0].chan.size(), where(p->banks[0].L, p->banks[0].r));
            for (size_t i = 1; i < p->banks.size(); i++) add(" + bank of %d %s", (int)p->banks[i].chan.size(), where(p->banks[i].L, p->banks[i].r));
        } else {
            for (size_t i = 0; i < p->banks.size(); i++) {
                const auto &b = p->banks[i];
                add("%s%s bank of %d, l = %d", i ? " + " : "", kernel(b.L), (int)b.chan.size(), b.L);
                if (b.L == 256) add(" (r = %d)", b.r); else add(" %s", where(b.L, b.r));
            }
        }
        if (p->banks.size() > 1 && !all256) add(" (%s launches)", p->banks.size() == 2 ? "two" : p->banks.size() == 3 ? "three" : "four");
        if (!p->bank_alias.empty()) add(" + %d copies of channels with the same slice", (int)p->bank_alias.size());
        if (p->split) add(" + %d other channels on a partial spectrum", (int)p->rem.size());
    } else if (p->poly_ok) {
        add("two launches (stage 1 + stage 2), l = %d", p->banks[0].L);
    } else {
        add("%s", "forward transform to a spectrum in memory + channel kernels");
    }
    if (!p->wf_route.empty()) add("; waterfall rows: %s", p->wf_route.c_str());
    if (!p->iq_route.empty()) add("; input %s", p->iq_route.c_str());
    if (!p->oq_route.empty()) add("; output %s", p->oq_route.c_str());
    if (!p->fine_route.empty()) add("; fine tuning: %s", p->fine_route.c_str());
    if (!p->levels_route.empty()) add("; levels: %s", p->levels_route.c_str());
    if (!p->gains_route.empty()) add("; gains: %s", p->gains_route.c_str());
    if (!p->lag1_route.empty()) add("; lag1: %s", p->lag1_route.c_str());
    if (!p->demod_route.empty()) add("; demod: %s", p->demod_route.c_str());
    if (!p->audio_route.empty()) add("; audio: %s", p->audio_route.c_str());
    if (!p->squelch_route.empty()) add("; squelch: %s", p->squelch_route.c_str());
    if (!p->tones_route.empty()) add("; tones: %s", p->tones_route.c_str());
    if (!p->tsq_route.empty()) add("; tone squelch: %s", p->tsq_route.c_str());
    std::snprintf(buf, (size_t)n, "%s", t);
    return k;
}

int fdc_pipeline_synchronize(fdc_pipeline *p)
{
    FDC_ENTRY("fdc_pipeline_synchronize")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_enable_timing(fdc_pipeline *p, int enable)
{
    FDC_ENTRY("fdc_pipeline_enable_timing")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    p->timing = enable != 0;
    p->timing_stride = enable > 1 ? enable : 1;
    p->timing_seq = 0;
    p->ev_used = 0; p->ev_spans.clear();
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_last_kernel_ms(fdc_pipeline *p, float *ms, int n)
{
    FDC_ENTRY("fdc_pipeline_last_kernel_ms")
    if (!p || !ms || n < 4) return set_error(FDC_ERR_INVALID_ARGUMENT, "need room for 4 values");
    ms[0] = ms[1] = ms[2] = 0.f;
    ms[3] = (float)p->ev_spans.size();
    for (auto &sp : p->ev_spans) {
        float a = 0, b = 0, c = 0;
        HIPCHK(hipEventSynchronize(p->events[sp[3]]));
        HIPCHK(hipEventElapsedTime(&a, p->events[sp[0]], p->events[sp[1]]));
        HIPCHK(hipEventElapsedTime(&b, p->events[sp[1]], p->events[sp[2]]));
        HIPCHK(hipEventElapsedTime(&c, p->events[sp[2]], p->events[sp[3]]));
        // every span says which form it ran (a call may mix them: a short last launch group takes the two-launch form)
        switch ((int)sp[4]) {
        case kSpanBanks: ms[0] += a; ms[1] += b; ms[2] += c; break;        // bank launches; remainder: forward transform, channel kernels
        case kSpanTwoLaunch: ms[0] += a; ms[1] += c; break;                // stage 1, stage 2 (b = the wait between them)
        case kSpanSpectrumLds: ms[1] += a + b; ms[2] += c; break;
        default: ms[0] += a; ms[1] += b; ms[2] += c;
        }
    }
    p->ev_used = 0; p->ev_spans.clear();
    return 4;
    FDC_ENTRY_END
}

void fdc_pipeline_reset(fdc_pipeline *p)
{
    if (!p) return;
    p->blockcount = 0;
    // (a batch of the pipelined hier entry that sits transformed in the bank stays there: the sink blocks are blocks of their own with their own
    // state, its PDUs come out with the next call or fdc_pipeline_flush_sinks)
    if (p->ev_hier && p->hier_ring_busy) (void)hipEventSynchronize(p->ev_hier);
    if (p->d_ring) {
        (void)hipSetDevice(p->cfg.device_id);
        (void)hipMemsetAsync(p->d_ring, 0, sizeof(float2) * (size_t)p->ovl, p->stream);
        // the integer ring is sized for the widest format (fdc::kIqRingBytes per sample): its history of any format is zeroed
        if (p->d_iq) (void)hipMemsetAsync(p->d_iq, 0, fdc::kIqRingBytes * (size_t)p->ovl, p->stream);
        (void)hipStreamSynchronize(p->stream);
    }
    p->in_form = -1;
    p->in_scale = 0.f;
    p->iq_route.clear();
    p->oq_route.clear();         // (the output format itself is a setting: it stays)
    p->fine_route.clear();       // (and so does fine tuning)
    p->levels_route.clear();     // (and so do the channel levels)
    p->gains_route.clear();      // (and the channel gains)
    p->lag1_route.clear();       // (and the channel lag-1 correlation)
    p->demod_route.clear();      // (and the channel demodulation, whose stream starts anew: no carry in front of the next call)
    p->demod_next = -1;
    p->audio_route.clear();      // (and the channel audio, whose history does not survive either)
    p->audio_next = -1;
    p->squelch_route.clear();    // (and the channel squelch: every channel starts closed again)
    p->squelch_next = -1;
    p->tones_route.clear();      // (and the channel tones: no frame is open)
    p->tones_next = -1;
    p->tones_fill = 0;
    p->tsq_route.clear();        // (and the tone squelch, which goes on where the tones do: every channel starts closed again)
    p->tsq_valid = false;
}

int fdc_pipeline_set_output_format(fdc_pipeline *p, int32_t format, float scale)
{
    FDC_ENTRY("fdc_pipeline_set_output_format")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (format != FDC_OQ_FC32 && format != FDC_OQ_SC16 && format != FDC_OQ_SC8) return set_error(FDC_ERR_INVALID_ARGUMENT, "unknown output format %d", (int)format);
    if (!std::isfinite(scale) || scale == 0.0f) return set_error(FDC_ERR_INVALID_ARGUMENT, "the output scale must be finite and not zero");
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (format && p->demod_mode)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel demodulation writes real float32 samples: switch it off first (fdc_pipeline_set_demod(p, FDC_DEMOD_OFF, 1))");
    if (format && !p->d_out) {
        // the float staging of the plans whose kernels do not narrow themselves: allocated here, once, so that no device entry allocates while it enqueues
        HIPCHK(hipSetDevice(p->cfg.device_id));
        RCCHK(out_staging(p));
    }
    p->out_form = format;
    p->out_scale = format ? scale : 1.0f;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_fine_tuning_increment(double nu, uint64_t *inc)
{
    FDC_ENTRY("fdc_fine_tuning_increment")
    if (!inc) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (!(std::fabs(nu) < 0.5)) return set_error(FDC_ERR_INVALID_ARGUMENT, "the fine-tuning frequency must be inside (-0.5, 0.5) cycles per output sample");
    // nu * 2^64 is exact in double (a power of two), |.| < 2^63; nearbyint rounds half to even in the default rounding mode
    const double r = std::nearbyint(std::ldexp(nu, 64));
    *inc = r < 0 ? (uint64_t)0 - (uint64_t)(-r) : (uint64_t)r;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_set_fine_tuning(fdc_pipeline *p, const double *nu, int n)
{
    FDC_ENTRY("fdc_pipeline_set_fine_tuning")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (n != p->C) return set_error(FDC_ERR_INVALID_ARGUMENT, "fine tuning: %d frequencies for %d channels", n, p->C);
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    std::vector<uint64_t> inc((size_t)p->C, 0);
    bool on = false;
    for (int c = 0; nu && c < p->C; c++) {
        RCCHK(fdc_fine_tuning_increment(nu[c], &inc[(size_t)c]));
        on = on || inc[(size_t)c] != 0;
    }
    if (!on) { p->fine_on = false; p->fine_route.clear(); return FDC_OK; }
    // the tables: per channel (inc, start of its step factors; even, so that a row of them can be read 16 bytes at a time), per schedule row of path 5
    // the same, and step_c[j] = exp(-2 pi i frac(inc_c j / 2^64)) designed in double, rounded once
    std::vector<fdc::FineChan> fc((size_t)p->C), f4(64, fdc::FineChan{0, 0});
    long long off = 0;
    for (int c = 0; c < p->C; c++) { fc[(size_t)c] = fdc::FineChan{inc[(size_t)c], off}; off += (p->chans[(size_t)c].lout + 1) & ~1; }
    std::vector<float2> step((size_t)off, make_float2(1.0f, 0.0f));
    for (int c = 0; c < p->C; c++)
        for (int j = 0; j < p->chans[(size_t)c].lout; j++)
            step[(size_t)(fc[(size_t)c].step_off + j)] = unit(std::ldexp((double)(inc[(size_t)c] * (uint64_t)j), -64));
    if (p->fused)
        for (int w = 0; w < 4 * p->f4_teams; w++)
            for (size_t k = 0; k < p->f4_wave[w].size() && k < 8; k++) f4[(size_t)(8 * w) + k] = fc[(size_t)(p->f4_wave[w][k] >> 1)];
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!p->d_fine) HIPCHK(p->d_fine.alloc(fc.size()));
    if (!p->d_fstep) HIPCHK(p->d_fstep.alloc(step.size()));
    if (p->fused && !p->d_f4fine) HIPCHK(p->d_f4fine.alloc(f4.size()));
    HIPCHK(hipMemcpy(p->d_fine, fc.data(), sizeof(fdc::FineChan) * fc.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_fstep, step.data(), sizeof(float2) * step.size(), hipMemcpyHostToDevice));
    if (p->fused) HIPCHK(hipMemcpy(p->d_f4fine, f4.data(), sizeof(fdc::FineChan) * f4.size(), hipMemcpyHostToDevice));
    p->fine_on = true;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_set_levels(fdc_pipeline *p, int32_t on)
{
    FDC_ENTRY("fdc_pipeline_set_levels")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (!on && p->squelch_on)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel squelch decides on the levels: switch the squelch off first (fdc_pipeline_set_squelch(p, NULL, NULL, C, 0))");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!on) { p->levels_on = false; p->levels_route.clear(); return FDC_OK; }
    // everything the feature needs, once: one (power, peak) pair per block of the longest call and channel, on the device and pinned on the host
    const size_t n = (size_t)p->cfg.max_blocks * (size_t)p->C;
    if (n > 0 && !p->d_levels) HIPCHK(p->d_levels.alloc(n));
    if (n > 0 && !p->pin_levels) HIPCHK(p->pin_levels.alloc(n));
    if (!p->levels_on) p->lev_blocks = -1;            // switched on: no call has levels yet
    p->levels_on = true;
    const char *sep = fdc::debug_env("FDC_LEVELS_SEPARATE");
    p->levels_separate = sep && atoi(sep) > 0;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_levels(fdc_pipeline *p, float *dst, int nblocks)
{
    FDC_ENTRY("fdc_pipeline_levels")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->levels_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel levels are off (fdc_pipeline_set_levels)");
    if (p->lev_blocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "no work call has run since the channel levels were switched on");
    if (nblocks != p->lev_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "the last work call had %d blocks, not %d", p->lev_blocks, nblocks);
    const size_t n = (size_t)nblocks * (size_t)p->C;
    if (n == 0) return FDC_OK;
    if (!dst) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->lev_host) {
        // a device entry's levels: read behind everything enqueued so far on the stream it ran on
        HIPCHK(hipSetDevice(p->cfg.device_id));
        HIPCHK(hipMemcpyAsync(p->pin_levels.get(), p->d_levels.get(), sizeof(float2) * n, hipMemcpyDeviceToHost, p->lev_stream));
        HIPCHK(hipStreamSynchronize(p->lev_stream));
        p->lev_host = true;
    }
    std::memcpy(dst, p->pin_levels.get(), sizeof(float2) * n);
    return FDC_OK;
    FDC_ENTRY_END
}

// the channel lag-1 correlation: the levels' setting and reader, word for word, on a buffer pair of its own
int fdc_pipeline_set_lag1(fdc_pipeline *p, int32_t on)
{
    FDC_ENTRY("fdc_pipeline_set_lag1")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!on) { p->lag1_on = false; p->lag1_route.clear(); return FDC_OK; }
    // everything the feature needs, once: one complex sum per block of the longest call and channel, on the device and pinned on the host
    const size_t n = (size_t)p->cfg.max_blocks * (size_t)p->C;
    if (n > 0 && !p->d_lag1) HIPCHK(p->d_lag1.alloc(n));
    if (n > 0 && !p->pin_lag1) HIPCHK(p->pin_lag1.alloc(n));
    if (!p->lag1_on) p->lag_blocks = -1;              // switched on: no call has a result yet
    p->lag1_on = true;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_lag1(fdc_pipeline *p, float *dst, int nblocks)
{
    FDC_ENTRY("fdc_pipeline_lag1")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->lag1_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel lag-1 correlation is off (fdc_pipeline_set_lag1)");
    if (p->lag_blocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "no work call has run since the channel lag-1 correlation was switched on");
    if (nblocks != p->lag_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "the last work call had %d blocks, not %d", p->lag_blocks, nblocks);
    const size_t n = (size_t)nblocks * (size_t)p->C;
    if (n == 0) return FDC_OK;
    if (!dst) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->lag_host) {
        // a device entry's result: read behind everything enqueued so far on the stream it ran on
        HIPCHK(hipSetDevice(p->cfg.device_id));
        HIPCHK(hipMemcpyAsync(p->pin_lag1.get(), p->d_lag1.get(), sizeof(float2) * n, hipMemcpyDeviceToHost, p->lag_stream));
        HIPCHK(hipStreamSynchronize(p->lag_stream));
        p->lag_host = true;
    }
    std::memcpy(dst, p->pin_lag1.get(), sizeof(float2) * n);
    return FDC_OK;
    FDC_ENTRY_END
}

// the channel demodulation: a setting like the ones above; FM's stream state (the carry) starts anew whenever the mode changes
int fdc_pipeline_set_demod(fdc_pipeline *p, int32_t mode, float gain)
{
    FDC_ENTRY("fdc_pipeline_set_demod")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (mode != FDC_DEMOD_OFF && mode != FDC_DEMOD_FM && mode != FDC_DEMOD_MAG) return set_error(FDC_ERR_INVALID_ARGUMENT, "unknown demodulation mode %d", (int)mode);
    if (mode && (!std::isfinite(gain) || gain == 0.0f)) return set_error(FDC_ERR_INVALID_ARGUMENT, "the demodulation gain must be finite and not zero");
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (mode && p->out_form)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel demodulation writes real float32 samples: set the output format to FDC_OQ_FC32 first");
    if (!mode && p->rs_up)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio resampler filters the demodulated samples: switch it off first (fdc_pipeline_set_audio_resampler(p, 0, 0, NULL, 0, 0, 1))");
    if (!mode && p->audio_decim)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel audio filters the demodulated samples: switch the audio off first (fdc_pipeline_set_audio(p, 0, NULL, 0, 0, 1))");
    if (!mode && p->tones_T)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel tones correlate the demodulated samples: switch the tones off first (fdc_pipeline_set_tones(p, NULL, C, 0, 0, 0))");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!mode) { p->demod_mode = 0; p->demod_gain = 1.0f; p->demod_next = -1; p->demod_route.clear(); return FDC_OK; }
    // everything the feature needs, once: the float staging the kernels write (integer output's) and the two carry buffers
    RCCHK(out_staging(p));
    for (int i = 0; i < 2; i++)
        if (p->C > 0 && !p->d_carry[i]) HIPCHK(p->d_carry[i].alloc((size_t)p->C));
    if (mode != p->demod_mode) p->demod_next = p->audio_next = p->tones_next = -1;    // switched on, or another mode: no sample in front of the next call, no
                                                                      // history in front of its audio, no open tone frame (a new gain alone keeps them)
    p->demod_mode = mode;
    p->demod_gain = gain;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_demod(const fdc_pipeline *p, int32_t *mode, float *gain)
{
    FDC_ENTRY("fdc_pipeline_demod")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (mode) *mode = p->demod_mode;
    if (gain) *gain = p->demod_gain;
    return FDC_OK;
    FDC_ENTRY_END
}

// the demodulating pass alone, on the caller's device buffers: the handle gives its channel table and nothing of its state is read or written
int fdc_pipeline_demod_device(const fdc_pipeline *p, int32_t mode, float gain, const void *d_in, void *d_out, const void *d_carry_in, void *d_carry_out,
                              int nblocks, void *stream)
{
    FDC_ENTRY("fdc_pipeline_demod_device")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (mode != FDC_DEMOD_FM && mode != FDC_DEMOD_MAG) return set_error(FDC_ERR_INVALID_ARGUMENT, "unknown demodulation mode %d", (int)mode);
    if (!std::isfinite(gain) || gain == 0.0f) return set_error(FDC_ERR_INVALID_ARGUMENT, "the demodulation gain must be finite and not zero");
    if (nblocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count");
    if (nblocks == 0 || p->C <= 0) return FDC_OK;
    if ((int64_t)nblocks * p->sum_lout * 8 > 0xFFFFF000ll)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d x %lld output samples per block is more than the 4 GiB one call may produce", nblocks, (long long)p->sum_lout);
    if (!d_in || !d_out || (mode == FDC_DEMOD_FM && !d_carry_out)) return set_error(FDC_ERR_INVALID_ARGUMENT, "null device buffer");
    if (mode == FDC_DEMOD_FM && d_carry_in == d_carry_out) return set_error(FDC_ERR_INVALID_ARGUMENT, "the carry is read from one buffer and written to another");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    const bool fm = mode == FDC_DEMOD_FM;
    HIPCHK(fdc::launch_chan_demod(mode, gain, static_cast<const float2 *>(d_in), static_cast<float *>(d_out), p->d_chans,
                                  fm ? static_cast<const float2 *>(d_carry_in) : nullptr, fm ? static_cast<float2 *>(d_carry_out) : nullptr, p->C, nblocks,
                                  (long long)p->sum_lout, stream ? static_cast<hipStream_t>(stream) : p->stream));
    return FDC_OK;
    FDC_ENTRY_END
}

// the channel audio: a setting that needs the demodulation; everything it needs is allocated here, once per size, and the stream state (the history)
// starts anew whenever the filter changes
int fdc_pipeline_set_audio(fdc_pipeline *p, int32_t decim, const float *taps, int32_t ntaps, int32_t format, float scale)
{
    FDC_ENTRY("fdc_pipeline_set_audio")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (decim) {
        if (decim < 1 || decim > 64) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio decimation %d is not in 1 .. 64", (int)decim);
        if (ntaps < 1 || ntaps > 256 || !taps) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio filter has 1 .. 256 taps");
        for (int k = 0; k < ntaps; k++)
            if (!std::isfinite(taps[k])) return set_error(FDC_ERR_INVALID_ARGUMENT, "audio tap %d is not finite", k);
        if (format != FDC_AUDIO_F32 && format != FDC_AUDIO_S16) return set_error(FDC_ERR_INVALID_ARGUMENT, "unknown audio format %d", (int)format);
        if (format == FDC_AUDIO_S16 && (!std::isfinite(scale) || scale == 0.0f)) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio scale must be finite and not zero");
    }
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (decim && !p->demod_mode)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel audio filters the demodulated samples: switch the channel demodulation on first (fdc_pipeline_set_demod)");
    if (!decim && p->pack_on)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing packs the channel audio: switch the packing off first (fdc_pipeline_set_audio_packing(p, 0))");
    for (int c = 0; decim && c < p->C; c++)
        if (p->chans[(size_t)c].lout % decim)
            return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio decimation %d does not divide the %d output samples per block of channel %d", (int)decim,
                             (int)p->chans[(size_t)c].lout, c);
    if (decim && p->pack_on) {
        // (the packed offsets are 32-bit words: the bound fdc_pipeline_set_audio_packing checked, for the new decimation)
        unsigned long long a = 0;
        for (int c = 0; c < p->C; c++) a += (unsigned long long)(p->chans[(size_t)c].lout / decim);
        if ((unsigned long long)p->cfg.max_blocks * a >= (1ull << 32))
            return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing is on: max_blocks x the audio samples per block must stay below 2^32");
    }
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!decim) {
        p->audio_decim = 0; p->audio_format = FDC_AUDIO_F32; p->audio_scale = 1.0f; p->audio_taps.clear(); p->audio_row = 0;
        p->rs_up = p->rs_down = p->rs_kp = 0; p->rs_taps.clear();       // (whichever form was on)
        p->audio_next = -1; p->aud_blocks = -1; p->audio_route.clear();
        return FDC_OK;
    }
    // the audio's own prefix sums, in channel order (not out_off, which copies of a channel may share)
    std::vector<long long> aoff((size_t)std::max(p->C, 1), 0);
    long long row = 0;
    for (int c = 0; c < p->C; c++) { aoff[(size_t)c] = row; row += p->chans[(size_t)c].lout / decim; }
    // everything the feature needs, once per size: the taps and the columns, the two histories, the rows of the longest call (4 bytes per element: the
    // wider format) and their pinned twin
    const size_t nh = (size_t)p->C * (size_t)(ntaps - 1), na = sizeof(float) * (size_t)p->cfg.max_blocks * (size_t)row;
    if (!p->d_ataps) HIPCHK(p->d_ataps.alloc(256));
    if (p->C > 0 && !p->d_aoff) HIPCHK(p->d_aoff.alloc((size_t)p->C));
    for (int i = 0; i < 2; i++)
        if (nh > p->d_ahist[i].capacity()) HIPCHK(p->d_ahist[i].reserve(nh, nh));
    if (na > p->d_audio.capacity()) HIPCHK(p->d_audio.reserve(na, na));
    if (na > p->pin_audio.capacity()) HIPCHK(p->pin_audio.reserve(na, na));
    HIPCHK(hipMemcpy(p->d_ataps, taps, sizeof(float) * (size_t)ntaps, hipMemcpyHostToDevice));
    if (p->C > 0) HIPCHK(hipMemcpy(p->d_aoff, aoff.data(), sizeof(long long) * (size_t)p->C, hipMemcpyHostToDevice));
    // a new decimation or other taps: another filter, whose stream starts anew; a new format or scale alone keeps the history.  The rows of the last call
    // are in the format and the width of the setting they were made with: a new format or decimation leaves none to fetch
    const bool same = p->audio_decim == decim && p->audio_taps.size() == (size_t)ntaps && std::memcmp(p->audio_taps.data(), taps, sizeof(float) * (size_t)ntaps) == 0;
    if (!same) p->audio_next = -1;
    if (p->audio_decim != decim || p->audio_format != format) p->aud_blocks = -1;
    p->rs_up = p->rs_down = p->rs_kp = 0; p->rs_taps.clear();           // the two forms replace each other (audio_decim was 0 beside it: all of the above)
    p->audio_decim = decim; p->audio_format = format; p->audio_scale = format == FDC_AUDIO_S16 ? scale : 1.0f;
    p->audio_taps.assign(taps, taps + ntaps);
    p->audio_row = row;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_audio_setting(const fdc_pipeline *p, int32_t *decim, int32_t *ntaps, int32_t *format, float *scale, float *taps)
{
    FDC_ENTRY("fdc_pipeline_audio_setting")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (decim) *decim = p->audio_decim;
    if (ntaps) *ntaps = (int32_t)p->audio_taps.size();
    if (format) *format = p->audio_format;
    if (scale) *scale = p->audio_scale;
    if (taps) std::copy(p->audio_taps.begin(), p->audio_taps.end(), taps);
    return FDC_OK;
    FDC_ENTRY_END
}

int64_t fdc_pipeline_audio_row(const fdc_pipeline *p) { return p && fdc::pipe::audio_set(p) ? p->audio_row : 0; }

// the audio rows of the last call: never more than the caller says its buffer holds
int fdc_pipeline_audio(fdc_pipeline *p, void *dst, size_t capacity_bytes, int nblocks)
{
    FDC_ENTRY("fdc_pipeline_audio")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!fdc::pipe::audio_set(p)) return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel audio is off (fdc_pipeline_set_audio, fdc_pipeline_set_audio_resampler)");
    if (p->pack_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing is on: there is no matrix, fetch the packed audio (fdc_pipeline_audio_packed)");
    if (p->aud_blocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "no work call has run since the channel audio was switched on or its format or decimation changed");
    if (nblocks != p->aud_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "the last work call had %d blocks, not %d", p->aud_blocks, nblocks);
    const size_t n = fdc::pipe::audio_bytes(p) * (size_t)nblocks * (size_t)p->audio_row;
    if (n == 0) return FDC_OK;
    if (capacity_bytes < n) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio of %d blocks takes %zu bytes, the buffer holds %zu", nblocks, n, capacity_bytes);
    if (!dst) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->aud_host) {
        // a device entry's rows: read behind everything enqueued so far on the stream it ran on
        HIPCHK(hipSetDevice(p->cfg.device_id));
        HIPCHK(hipMemcpyAsync(p->pin_audio.get(), p->d_audio.get(), n, hipMemcpyDeviceToHost, p->aud_stream));
        HIPCHK(hipStreamSynchronize(p->aud_stream));
        p->aud_host = true;
    }
    std::memcpy(dst, p->pin_audio.get(), n);
    return FDC_OK;
    FDC_ENTRY_END
}

void *fdc_pipeline_audio_device(fdc_pipeline *p) { return p && fdc::pipe::audio_set(p) ? static_cast<void *>(p->d_audio.get()) : nullptr; }

// the audio pass alone, on the caller's device buffers: the handle gives its channel table and the audio setting, nothing of its stream state (but,
// while the squelch is on, the mask of its last work call, which gates the pass)
int fdc_pipeline_audio_pass_device(const fdc_pipeline *p, const void *d_in, void *d_out, const void *d_hist_in, void *d_hist_out, int nblocks, void *stream)
{
    FDC_ENTRY("fdc_pipeline_audio_pass_device")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (p->rs_up) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio resampler is on: its pass alone is fdc_pipeline_audio_resampler_pass_device");
    if (!p->audio_decim) return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel audio is off (fdc_pipeline_set_audio)");
    if (nblocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count");
    if (nblocks == 0 || p->C <= 0) return FDC_OK;
    if ((int64_t)nblocks * p->sum_lout * 8 > 0xFFFFF000ll)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d x %lld output samples per block is more than the 4 GiB one call may produce", nblocks, (long long)p->sum_lout);
    const int K = (int)p->audio_taps.size();
    if (!d_in || !d_out || (K > 1 && !d_hist_out)) return set_error(FDC_ERR_INVALID_ARGUMENT, "null device buffer");
    if (K > 1 && d_hist_in == d_hist_out) return set_error(FDC_ERR_INVALID_ARGUMENT, "the history is read from one buffer and written to another");
    // the squelch on: the gated form, over the handle's mask of the last call (fdc_pipeline_squelch_device), which must have this call's rows
    const unsigned char *gate = squelch_rows(p, 0);
    if (gate && p->sq_blocks != nblocks)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel squelch is on: the gated audio pass reads the mask of the last call, which had %d blocks, not %d",
                         p->sq_blocks, nblocks);
    // the packing on: the packed form, over the offsets of that same call (which count the elements it writes at the front of d_out)
    const unsigned *pack = gate ? pack_rows(p, 0) : nullptr;
    if (pack && p->aud_blocks != nblocks)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing is on: the packed audio pass reads the offsets of the last call, and no call of %d blocks "
                         "has run since the packing was switched on or the audio's format or decimation changed", nblocks);
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(fdc::launch_chan_audio(p->audio_format, p->audio_decim, K, p->audio_scale, p->d_ataps, p->d_aoff, (long long)p->audio_row,
                                  static_cast<const float *>(d_in), d_out, p->d_chans, K > 1 ? static_cast<const float *>(d_hist_in) : nullptr,
                                  K > 1 ? static_cast<float *>(d_hist_out) : nullptr, p->C, nblocks, (long long)p->sum_lout,
                                  stream ? static_cast<hipStream_t>(stream) : p->stream, gate, pack));
    return FDC_OK;
    FDC_ENTRY_END
}

// how many outputs of a resampled stream stand in front of block m of a channel of lout samples per block: ceil(m lout up / down)
static int64_t resampler_first_output(int64_t m, int32_t lout, int32_t up, int32_t down)
{
    return (int64_t)(((__int128)m * lout * up + (down - 1)) / down);
}

// the outputs block first_block + i owns, i = 0 .. nblocks - 1: a function of the absolute block index alone (128-bit products: first_block may be 2^40
// and more)
int fdc_audio_resampler_counts(int32_t lout, int32_t up, int32_t down, int64_t first_block, int32_t nblocks, int32_t *counts)
{
    FDC_ENTRY("fdc_audio_resampler_counts")
    if (lout < 1 || up < 1 || up > 64 || down < 1 || down > 128) return set_error(FDC_ERR_INVALID_ARGUMENT, "resampler counts: lout >= 1, up 1 .. 64, down 1 .. 128");
    if (first_block < 0 || nblocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count/index");
    if (nblocks > 0 && !counts) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (first_block > INT64_MAX - nblocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "resampler counts: the block index does not fit 64 bits");
    if (((__int128)(first_block + nblocks) * lout * up + (down - 1)) / down > (__int128)INT64_MAX)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "resampler counts: the output index does not fit 64 bits");
    int64_t lo = resampler_first_output(first_block, lout, up, down);
    for (int32_t i = 0; i < nblocks; i++) {
        const int64_t hi = resampler_first_output(first_block + i + 1, lout, up, down);
        counts[i] = (int32_t)(hi - lo);
        lo = hi;
    }
    return FDC_OK;
    FDC_ENTRY_END
}

static int gcd_int(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// the audio resampler: the other form of the channel audio; everything it needs is allocated here, once per size, and the stream state (the history)
// starts anew whenever the filter changes
int fdc_pipeline_set_audio_resampler(fdc_pipeline *p, int32_t up, int32_t down, const float *taps, int32_t ntaps, int32_t format, float scale)
{
    FDC_ENTRY("fdc_pipeline_set_audio_resampler")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    int kp = 0;
    if (up) {
        if (up < 1 || up > 64) return set_error(FDC_ERR_INVALID_ARGUMENT, "the resampler's interpolation %d is not in 1 .. 64", (int)up);
        if (down < 1 || down > 128) return set_error(FDC_ERR_INVALID_ARGUMENT, "the resampler's decimation %d is not in 1 .. 128", (int)down);
        const int g = gcd_int(up, down);
        if (g != 1)
            return set_error(FDC_ERR_INVALID_ARGUMENT, "the ratio %d / %d is not reduced, which would leave tap phases unused: give %d / %d", (int)up, (int)down,
                             (int)up / g, (int)down / g);
        if (ntaps < 1 || !taps) return set_error(FDC_ERR_INVALID_ARGUMENT, "the resampler's filter has at least 1 tap");
        kp = (int)(((int64_t)ntaps + up - 1) / up);
        if (kp > 256) return set_error(FDC_ERR_INVALID_ARGUMENT, "the resampler's filter has %d taps per phase (ceil(%d / %d)), more than 256", kp, (int)ntaps, (int)up);
        for (int k = 0; k < ntaps; k++)
            if (!std::isfinite(taps[k])) return set_error(FDC_ERR_INVALID_ARGUMENT, "resampler tap %d is not finite", k);
        if (format != FDC_AUDIO_F32 && format != FDC_AUDIO_S16) return set_error(FDC_ERR_INVALID_ARGUMENT, "unknown audio format %d", (int)format);
        if (format == FDC_AUDIO_S16 && (!std::isfinite(scale) || scale == 0.0f)) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio scale must be finite and not zero");
    }
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (up && !p->demod_mode)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio resampler filters the demodulated samples: switch the channel demodulation on first (fdc_pipeline_set_demod)");
    if (up && p->pack_on)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing packs the decimating form's cells: switch the packing off first (fdc_pipeline_set_audio_packing(p, 0))");
    for (int c = 0; up && c < p->C; c++)
        if ((int64_t)p->chans[(size_t)c].lout * up >= (1ll << 31))
            return set_error(FDC_ERR_INVALID_ARGUMENT, "the %d output samples per block of channel %d times the interpolation %d reach 2^31", (int)p->chans[(size_t)c].lout, c, (int)up);
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!up) {
        if (p->rs_up) {
            p->rs_up = p->rs_down = p->rs_kp = 0; p->rs_taps.clear(); p->audio_format = FDC_AUDIO_F32; p->audio_scale = 1.0f; p->audio_row = 0;
            p->audio_next = -1; p->aud_blocks = -1; p->audio_route.clear();
        }
        return FDC_OK;
    }
    // the columns: W_c = ceil(lout_c up / down) per channel, in channel order
    std::vector<long long> aoff((size_t)std::max(p->C, 1), 0);
    long long row = 0;
    for (int c = 0; c < p->C; c++) { aoff[(size_t)c] = row; row += ((long long)p->chans[(size_t)c].lout * up + down - 1) / down; }
    // the taps as the kernel reads them: phase-major, [up][kp], +0 behind the last
    std::vector<float> pm((size_t)up * (size_t)kp, 0.0f);
    for (int i = 0; i < ntaps; i++) pm[(size_t)(i % up) * (size_t)kp + (size_t)(i / up)] = taps[i];
    // everything the feature needs, once per size: the table and the columns, the two histories, the rows of the longest call (4 bytes per element: the
    // wider format) and their pinned twin
    const size_t nh = (size_t)p->C * (size_t)(kp - 1), na = sizeof(float) * (size_t)p->cfg.max_blocks * (size_t)row;
    if (pm.size() > p->d_rstaps.capacity()) HIPCHK(p->d_rstaps.reserve(pm.size(), pm.size()));
    if (p->C > 0 && !p->d_aoff) HIPCHK(p->d_aoff.alloc((size_t)p->C));
    for (int i = 0; i < 2; i++)
        if (nh > p->d_ahist[i].capacity()) HIPCHK(p->d_ahist[i].reserve(nh, nh));
    if (na > p->d_audio.capacity()) HIPCHK(p->d_audio.reserve(na, na));
    if (na > p->pin_audio.capacity()) HIPCHK(p->pin_audio.reserve(na, na));
    HIPCHK(hipMemcpy(p->d_rstaps, pm.data(), sizeof(float) * pm.size(), hipMemcpyHostToDevice));
    if (p->C > 0) HIPCHK(hipMemcpy(p->d_aoff, aoff.data(), sizeof(long long) * (size_t)p->C, hipMemcpyHostToDevice));
    // a new ratio or other taps: another filter, whose stream starts anew; a new format or scale alone keeps the history.  The rows of the last call
    // are in the format and the width of the setting they were made with: a new ratio or format (or the other form before) leaves none to fetch
    const bool ratio = p->rs_up == up && p->rs_down == down;
    const bool same = ratio && p->rs_taps.size() == (size_t)ntaps && std::memcmp(p->rs_taps.data(), taps, sizeof(float) * (size_t)ntaps) == 0;
    if (!same) p->audio_next = -1;
    if (!ratio || p->audio_format != format) p->aud_blocks = -1;
    p->audio_decim = 0; p->audio_taps.clear();          // the two forms replace each other
    p->rs_up = up; p->rs_down = down; p->rs_kp = kp; p->rs_taps.assign(taps, taps + ntaps);
    p->audio_format = format; p->audio_scale = format == FDC_AUDIO_S16 ? scale : 1.0f;
    p->audio_row = row;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_audio_resampler_setting(const fdc_pipeline *p, int32_t *up, int32_t *down, int32_t *ntaps, int32_t *format, float *scale, float *taps,
                                         int32_t taps_capacity)
{
    FDC_ENTRY("fdc_pipeline_audio_resampler_setting")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (up) *up = p->rs_up;
    if (down) *down = p->rs_down;
    if (ntaps) *ntaps = (int32_t)p->rs_taps.size();
    if (format) *format = p->rs_up ? p->audio_format : FDC_AUDIO_F32;
    if (scale) *scale = p->rs_up ? p->audio_scale : 1.0f;
    if (taps && taps_capacity >= 0 && (size_t)taps_capacity >= p->rs_taps.size()) std::copy(p->rs_taps.begin(), p->rs_taps.end(), taps);
    return FDC_OK;
    FDC_ENTRY_END
}

int64_t fdc_pipeline_audio_first_block(const fdc_pipeline *p) { return p && fdc::pipe::audio_set(p) && p->aud_blocks >= 0 ? p->aud_first : -1; }

// the resampling pass alone, on the caller's device buffers: the handle gives its channel table and the resampler's setting, nothing of its stream state
int fdc_pipeline_audio_resampler_pass_device(const fdc_pipeline *p, const void *d_in, void *d_out, const void *d_hist_in, void *d_hist_out,
                                             int64_t first_block, int nblocks, const void *d_mask, void *stream)
{
    FDC_ENTRY("fdc_pipeline_audio_resampler_pass_device")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->rs_up) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio resampler is off (fdc_pipeline_set_audio_resampler)");
    if (nblocks < 0 || first_block < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count/index");
    if (nblocks == 0 || p->C <= 0) return FDC_OK;
    if ((int64_t)nblocks * p->sum_lout * 8 > 0xFFFFF000ll)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d x %lld output samples per block is more than the 4 GiB one call may produce", nblocks, (long long)p->sum_lout);
    const int K = p->rs_kp;
    if (!d_in || !d_out || (K > 1 && !d_hist_out)) return set_error(FDC_ERR_INVALID_ARGUMENT, "null device buffer");
    if (K > 1 && d_hist_in == d_hist_out) return set_error(FDC_ERR_INVALID_ARGUMENT, "the history is read from one buffer and written to another");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(fdc::launch_chan_resample(p->audio_format, p->rs_up, p->rs_down, K, p->audio_scale, p->d_rstaps, p->d_aoff, (long long)p->audio_row,
                                     static_cast<const float *>(d_in), d_out, p->d_chans, K > 1 ? static_cast<const float *>(d_hist_in) : nullptr,
                                     K > 1 ? static_cast<float *>(d_hist_out) : nullptr, p->C, nblocks, (long long)p->sum_lout, (long long)first_block,
                                     stream ? static_cast<hipStream_t>(stream) : p->stream, static_cast<const unsigned char *>(d_mask)));
    return FDC_OK;
    FDC_ENTRY_END
}

// the audio packing: a setting that needs the audio and the squelch; everything it needs is allocated here, once
int fdc_pipeline_set_audio_packing(fdc_pipeline *p, int on)
{
    FDC_ENTRY("fdc_pipeline_set_audio_packing")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (on && p->rs_up)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio resampler is on: its cells vary in length and are not packed; use the decimating form (fdc_pipeline_set_audio)");
    if (on && (!p->audio_decim || !p->squelch_on))
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing packs the channel audio by the squelch's mask: switch both on first (fdc_pipeline_set_audio, fdc_pipeline_set_squelch)");
    if (on && (unsigned long long)p->cfg.max_blocks * (unsigned long long)p->audio_row >= (1ull << 32))
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing keeps 32-bit offsets: max_blocks %d x %lld audio samples per block is not below 2^32",
                         p->cfg.max_blocks, (long long)p->audio_row);
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (on) {
        // everything the feature needs, once: the offsets of the longest call, the running total and its pinned twin
        const size_t nm = (size_t)p->cfg.max_blocks * (size_t)p->C;
        if (nm > 0 && !p->d_packoff) HIPCHK(p->d_packoff.alloc(nm));
        if (!p->d_packtotal) HIPCHK(p->d_packtotal.alloc(1));
        if (!p->pin_packtotal) HIPCHK(p->pin_packtotal.alloc(1));
    }
    // the audio of the last call is in the form of the setting it was made with: a switch leaves none to fetch
    if (p->pack_on != (on != 0)) { p->aud_blocks = -1; p->pack_count = 0; }
    p->pack_on = on != 0;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_audio_packing(const fdc_pipeline *p) { return p ? (p->pack_on ? 1 : 0) : -1; }

// the packed audio of the last call: its count always, its elements where the caller's buffer holds them
int fdc_pipeline_audio_packed(fdc_pipeline *p, void *dst, size_t capacity_bytes, int nblocks, int64_t *count)
{
    FDC_ENTRY("fdc_pipeline_audio_packed")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!count) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->pack_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing is off (fdc_pipeline_set_audio_packing)");
    if (p->aud_blocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "no work call has run since the audio packing was switched on or the audio's format or decimation changed");
    if (nblocks != p->aud_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "the last work call had %d blocks, not %d", p->aud_blocks, nblocks);
    const size_t esz = fdc::pipe::audio_bytes(p);
    if (!p->aud_host && packing_on(p) && nblocks > 0) {
        // a device entry's: the total first, then that many elements, both behind everything enqueued so far on the stream it ran on
        HIPCHK(hipSetDevice(p->cfg.device_id));
        HIPCHK(hipMemcpyAsync(p->pin_packtotal.get(), p->d_packtotal.get(), sizeof(long long), hipMemcpyDeviceToHost, p->aud_stream));
        HIPCHK(hipStreamSynchronize(p->aud_stream));
        p->pack_count = (int64_t)p->pin_packtotal[0];
        if (p->pack_count > 0) {
            HIPCHK(hipMemcpyAsync(p->pin_audio.get(), p->d_audio.get(), esz * (size_t)p->pack_count, hipMemcpyDeviceToHost, p->aud_stream));
            HIPCHK(hipStreamSynchronize(p->aud_stream));
        }
        p->aud_host = true;
    }
    const int64_t n = packing_on(p) && nblocks > 0 ? p->pack_count : 0;
    *count = n;
    if (!dst || n == 0) return FDC_OK;
    if (capacity_bytes < esz * (size_t)n)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the packed audio takes %zu bytes, the buffer holds %zu", esz * (size_t)n, capacity_bytes);
    std::memcpy(dst, p->pin_audio.get(), esz * (size_t)n);
    return FDC_OK;
    FDC_ENTRY_END
}

// the offsets alone, on the caller's device buffers: the handle gives its channel table and the audio's decimation, nothing of its state
int fdc_pipeline_audio_pack_offsets_device(const fdc_pipeline *p, const void *d_mask, const void *d_base_in, void *d_off, void *d_total_out, int nblocks,
                                           void *stream)
{
    FDC_ENTRY("fdc_pipeline_audio_pack_offsets_device")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->audio_decim) return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel audio is off (fdc_pipeline_set_audio): its decimation makes the cells' sizes");
    if (nblocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count");
    if (nblocks == 0 || p->C <= 0) return FDC_OK;
    if (!d_mask || !d_off || !d_total_out) return set_error(FDC_ERR_INVALID_ARGUMENT, "null device buffer");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(fdc::launch_audio_pack_offsets(static_cast<const unsigned char *>(d_mask), p->d_chans, p->audio_decim, static_cast<const long long *>(d_base_in),
                                          static_cast<unsigned *>(d_off), static_cast<long long *>(d_total_out), p->C, nblocks,
                                          stream ? static_cast<hipStream_t>(stream) : p->stream));
    return FDC_OK;
    FDC_ENTRY_END
}

// the channel squelch: a setting that needs the levels; everything it needs is allocated here, once, and new thresholds or a new hang count keep the
// stream state (which channels are open)
int fdc_pipeline_set_squelch(fdc_pipeline *p, const float *open_thr, const float *close_thr, int n, int32_t hang)
{
    FDC_ENTRY("fdc_pipeline_set_squelch")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (n != p->C) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel squelch: %d thresholds for %d channels", n, p->C);
    if (open_thr) {
        if (!close_thr) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel squelch: no close thresholds");
        if (hang < 0 || hang > 65535) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel squelch: the hang count %d is not in 0 .. 65535", (int)hang);
        for (int c = 0; c < p->C; c++) {
            if (!std::isfinite(open_thr[c]) || !std::isfinite(close_thr[c]) || open_thr[c] < 0.0f || close_thr[c] < 0.0f)
                return set_error(FDC_ERR_INVALID_ARGUMENT, "channel squelch: the thresholds of channel %d are not finite and >= 0", c);
            if (close_thr[c] > open_thr[c])
                return set_error(FDC_ERR_INVALID_ARGUMENT, "channel squelch: the close threshold of channel %d is above its open threshold", c);
        }
    }
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (!open_thr && p->tsq_on)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the tone squelch gates the squelch's mask: switch the tone squelch off first (fdc_pipeline_set_tone_squelch(p, NULL, ...))");
    if (!open_thr && p->pack_on)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the audio packing packs by the squelch's mask: switch the packing off first (fdc_pipeline_set_audio_packing(p, 0))");
    if (open_thr && !p->levels_on)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel squelch decides on the levels: switch the channel levels on first (fdc_pipeline_set_levels(p, 1))");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!open_thr) {
        p->squelch_on = false; p->sq_open.clear(); p->sq_close.clear(); p->sq_hang = 0;
        p->squelch_next = -1; p->sq_blocks = -1; p->squelch_route.clear();
        return FDC_OK;
    }
    // everything the feature needs, once: the two threshold tables, the two states, the mask of the longest call and its pinned twin
    const size_t nc = (size_t)p->C, nm = (size_t)p->cfg.max_blocks * nc;
    for (int i = 0; i < 2; i++) {
        if (nc > 0 && !p->d_sqthr[i]) HIPCHK(p->d_sqthr[i].alloc(nc));
        if (nc > 0 && !p->d_sqstate[i]) HIPCHK(p->d_sqstate[i].alloc(2 * nc));
    }
    if (nm > 0 && !p->d_mask) HIPCHK(p->d_mask.alloc(nm));
    if (nm > 0 && !p->pin_mask) HIPCHK(p->pin_mask.alloc(nm));
    if (nc > 0) {
        HIPCHK(hipMemcpy(p->d_sqthr[0], open_thr, sizeof(float) * nc, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->d_sqthr[1], close_thr, sizeof(float) * nc, hipMemcpyHostToDevice));
    }
    if (p->sq_open.size() != nc) { p->sq_open.resize(nc); p->sq_close.resize(nc); }
    std::copy(open_thr, open_thr + nc, p->sq_open.begin());
    std::copy(close_thr, close_thr + nc, p->sq_close.begin());
    p->sq_hang = hang;
    if (!p->squelch_on) { p->squelch_next = -1; p->sq_blocks = -1; }      // switched on: every channel starts closed, no call has a mask yet
    p->squelch_on = true;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_squelch_setting(const fdc_pipeline *p, float *open_thr, float *close_thr, int32_t *hang)
{
    FDC_ENTRY("fdc_pipeline_squelch_setting")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (hang) *hang = p->squelch_on ? p->sq_hang : -1;
    if (open_thr) std::copy(p->sq_open.begin(), p->sq_open.end(), open_thr);
    if (close_thr) std::copy(p->sq_close.begin(), p->sq_close.end(), close_thr);
    return FDC_OK;
    FDC_ENTRY_END
}

// the mask of the last call: never more than the caller says its buffer holds
int fdc_pipeline_squelch(fdc_pipeline *p, uint8_t *dst, size_t capacity_bytes, int nblocks)
{
    FDC_ENTRY("fdc_pipeline_squelch")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->squelch_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel squelch is off (fdc_pipeline_set_squelch)");
    if (p->sq_blocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "no work call has run since the channel squelch was switched on");
    if (nblocks != p->sq_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "the last work call had %d blocks, not %d", p->sq_blocks, nblocks);
    const size_t n = (size_t)nblocks * (size_t)p->C;
    if (n == 0) return FDC_OK;
    if (capacity_bytes < n) return set_error(FDC_ERR_INVALID_ARGUMENT, "the mask of %d blocks takes %zu bytes, the buffer holds %zu", nblocks, n, capacity_bytes);
    if (!dst) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->sq_host) {
        // a device entry's mask: read behind everything enqueued so far on the stream it ran on
        HIPCHK(hipSetDevice(p->cfg.device_id));
        HIPCHK(hipMemcpyAsync(p->pin_mask.get(), p->d_mask.get(), n, hipMemcpyDeviceToHost, p->sq_stream));
        HIPCHK(hipStreamSynchronize(p->sq_stream));
        p->sq_host = true;
    }
    std::memcpy(dst, p->pin_mask.get(), n);
    return FDC_OK;
    FDC_ENTRY_END
}

void *fdc_pipeline_squelch_device(fdc_pipeline *p) { return p && p->squelch_on ? static_cast<void *>(p->d_mask.get()) : nullptr; }

// the decision alone, on the caller's device buffers: the handle gives its setting, its gains and its channel count, nothing of its stream state
int fdc_pipeline_squelch_pass_device(const fdc_pipeline *p, const void *d_levels, void *d_mask, const void *d_state_in, void *d_state_out, int nblocks,
                                     void *stream)
{
    FDC_ENTRY("fdc_pipeline_squelch_pass_device")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->squelch_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel squelch is off (fdc_pipeline_set_squelch)");
    if (nblocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count");
    if (nblocks == 0 || p->C <= 0) return FDC_OK;
    if (!d_levels || !d_mask || !d_state_out) return set_error(FDC_ERR_INVALID_ARGUMENT, "null device buffer");
    if (d_state_in == d_state_out) return set_error(FDC_ERR_INVALID_ARGUMENT, "the state is read from one buffer and written to another");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(fdc::launch_chan_squelch(static_cast<const float2 *>(d_levels), p->gains_on ? p->d_gain.get() : nullptr, p->d_sqthr[0], p->d_sqthr[1], p->sq_hang,
                                    static_cast<const int *>(d_state_in), static_cast<int *>(d_state_out), static_cast<unsigned char *>(d_mask), p->C, nblocks,
                                    stream ? static_cast<hipStream_t>(stream) : p->stream));
    return FDC_OK;
    FDC_ENTRY_END
}

// the channel tones: a setting that needs the demodulation; everything it needs is allocated here, once per size, and the stream state (the open
// frame) starts anew whenever any part of the setting changes
int fdc_pipeline_set_tones(fdc_pipeline *p, const uint32_t *inc, int nchan, int ntones, int32_t group, int32_t frame_blocks)
{
    FDC_ENTRY("fdc_pipeline_set_tones")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (nchan != p->C) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel tones: increments for %d channels of %d", nchan, p->C);
    if (inc) {
        if (ntones < 1 || ntones > 64) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel tones: %d tones per channel are not in 1 .. 64", ntones);
        if (group < 1) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel tones: the group length %d is not positive", (int)group);
        if (frame_blocks < 1 || frame_blocks > 4096) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel tones: the frame length %d is not in 1 .. 4096 blocks", (int)frame_blocks);
    }
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (p->tsq_on && (!inc || ntones != p->tones_T || group != p->tones_S || frame_blocks != p->tones_W))
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the tone squelch decides on the frame rows of %d tones, groups of %d and frames of %d blocks: switch the tone "
                         "squelch off first (fdc_pipeline_set_tone_squelch(p, NULL, ...))", p->tones_T, p->tones_S, p->tones_W);
    if (inc && !p->demod_mode)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel tones correlate the demodulated samples: switch the channel demodulation on first (fdc_pipeline_set_demod)");
    for (int c = 0; inc && c < p->C; c++)
        if (p->chans[(size_t)c].lout % group)
            return set_error(FDC_ERR_INVALID_ARGUMENT, "the tone group length %d does not divide the %d output samples per block of channel %d", (int)group,
                             (int)p->chans[(size_t)c].lout, c);
    // the frame rows of the longest call, from the deepest fill on
    const size_t nct = inc ? (size_t)p->C * (size_t)ntones : 0;
    const size_t nrows = inc ? ((size_t)p->cfg.max_blocks + (size_t)frame_blocks - 1) / (size_t)frame_blocks : 0;
    if (nrows * nct * sizeof(float2) > ((size_t)1 << 31))
        return set_error(FDC_ERR_INVALID_ARGUMENT, "channel tones: %zu frame rows of %zu tones take more than 2^31 bytes", nrows, nct);
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!inc) {
        p->tones_T = p->tones_S = p->tones_W = 0; p->tones_inc.clear();
        p->tones_next = -1; p->tones_fill = 0; p->tn_blocks = -1; p->tn_frames = 0; p->tones_route.clear();
        return FDC_OK;
    }
    // everything the feature needs, once per size: the table, the increments, the two carries, the rows and their pinned twin
    if (!p->d_ttab) {
        std::vector<float2> tab((size_t)fdc::kToneTable);
        fdc::tone_table(tab.data());
        HIPCHK(p->d_ttab.upload(tab));
    }
    if (nct > p->d_tinc.capacity()) HIPCHK(p->d_tinc.reserve(nct, nct));
    for (int i = 0; i < 2; i++)
        if (nct > p->d_tcarry[i].capacity()) HIPCHK(p->d_tcarry[i].reserve(nct, nct));
    if (nrows * nct > p->d_tones.capacity()) HIPCHK(p->d_tones.reserve(nrows * nct, nrows * nct));
    if (nrows * nct > p->pin_tones.capacity()) HIPCHK(p->pin_tones.reserve(nrows * nct, nrows * nct));
    if (nct > 0) HIPCHK(hipMemcpy(p->d_tinc, inc, sizeof(uint32_t) * nct, hipMemcpyHostToDevice));
    const bool same = p->tones_T == ntones && p->tones_S == group && p->tones_W == frame_blocks && p->tones_inc.size() == nct &&
                      (nct == 0 || std::memcmp(p->tones_inc.data(), inc, sizeof(uint32_t) * nct) == 0);
    if (!same) { p->tones_next = -1; p->tones_fill = 0; p->tn_blocks = -1; p->tn_frames = 0; }      // another bank: its stream starts anew, no call has rows yet
    p->tones_T = ntones; p->tones_S = group; p->tones_W = frame_blocks;
    p->tones_inc.assign(inc, inc + nct);
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_tones_setting(const fdc_pipeline *p, int32_t *ntones, int32_t *group, int32_t *frame_blocks, uint32_t *inc)
{
    FDC_ENTRY("fdc_pipeline_tones_setting")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (ntones) *ntones = p->tones_T;
    if (group) *group = p->tones_S;
    if (frame_blocks) *frame_blocks = p->tones_W;
    if (inc) std::copy(p->tones_inc.begin(), p->tones_inc.end(), inc);
    return FDC_OK;
    FDC_ENTRY_END
}

// the frame rows the last call completed: never more than the caller says its buffer holds
int fdc_pipeline_tones(fdc_pipeline *p, void *dst, size_t capacity_bytes, int nblocks, int32_t *nframes)
{
    FDC_ENTRY("fdc_pipeline_tones")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->tones_T) return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel tones are off (fdc_pipeline_set_tones)");
    if (p->tn_blocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "no work call has run since the channel tones were switched on or their setting changed");
    if (nblocks != p->tn_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "the last work call had %d blocks, not %d", p->tn_blocks, nblocks);
    const size_t n = sizeof(float2) * (size_t)p->tn_frames * tones_row(p);
    if (capacity_bytes < n)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the %d tone frames of the last call take %zu bytes, the buffer holds %zu", p->tn_frames, n, capacity_bytes);
    if (nframes) *nframes = p->tn_frames;
    if (n == 0) return FDC_OK;
    if (!dst) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->tn_host) {
        // a device entry's rows: read behind everything enqueued so far on the stream it ran on
        HIPCHK(hipSetDevice(p->cfg.device_id));
        HIPCHK(hipMemcpyAsync(p->pin_tones.get(), p->d_tones.get(), n, hipMemcpyDeviceToHost, p->tn_stream));
        HIPCHK(hipStreamSynchronize(p->tn_stream));
        p->tn_host = true;
    }
    std::memcpy(dst, p->pin_tones.get(), n);
    return FDC_OK;
    FDC_ENTRY_END
}

void *fdc_pipeline_tones_device(fdc_pipeline *p) { return p && p->tones_T ? static_cast<void *>(p->d_tones.get()) : nullptr; }

// the tones pass alone, on the caller's device buffers: the handle gives its channel table and the tones' setting, nothing of its stream state
int fdc_pipeline_tones_pass_device(const fdc_pipeline *p, const void *d_in, void *d_frames, const void *d_carry_in, void *d_carry_out, int64_t first_block,
                                   int32_t fill, int nblocks, void *stream)
{
    FDC_ENTRY("fdc_pipeline_tones_pass_device")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->tones_T) return set_error(FDC_ERR_INVALID_ARGUMENT, "the channel tones are off (fdc_pipeline_set_tones)");
    if (nblocks < 0 || first_block < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count/index");
    if (fill < 0 || fill >= p->tones_W) return set_error(FDC_ERR_INVALID_ARGUMENT, "the fill %d is not in 0 .. %d, the frame length - 1", (int)fill, p->tones_W - 1);
    if (nblocks == 0 || p->C <= 0) return FDC_OK;
    if ((int64_t)nblocks * p->sum_lout * 8 > 0xFFFFF000ll)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d x %lld output samples per block is more than the 4 GiB one call may produce", nblocks, (long long)p->sum_lout);
    const bool rows = (fill + nblocks) / p->tones_W > 0;
    if (!d_in || !d_carry_out || (rows && !d_frames)) return set_error(FDC_ERR_INVALID_ARGUMENT, "null device buffer");
    if (d_carry_in == d_carry_out) return set_error(FDC_ERR_INVALID_ARGUMENT, "the carry is read from one buffer and written to another");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(fdc::launch_chan_tones(static_cast<const float *>(d_in), p->d_chans, p->d_tinc, p->d_ttab, static_cast<const float2 *>(d_carry_in),
                                  static_cast<float2 *>(d_carry_out), static_cast<float2 *>(d_frames), p->C, p->tones_T, p->tones_S, p->tones_W, fill,
                                  (long long)first_block, nblocks, stream ? static_cast<hipStream_t>(stream) : p->stream));
    return FDC_OK;
    FDC_ENTRY_END
}

// the tone squelch: a setting that needs the tones and the squelch; everything it needs is allocated here, once, and every new setting restarts its
// state (not the tones' frames)
int fdc_pipeline_set_tone_squelch(fdc_pipeline *p, const int32_t *tone, const float *open_thr, const float *close_thr, const float *ratio, int n,
                                  int32_t guard, int32_t hang_frames)
{
    FDC_ENTRY("fdc_pipeline_set_tone_squelch")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (n != p->C) return set_error(FDC_ERR_INVALID_ARGUMENT, "tone squelch: a setting for %d channels of %d", n, p->C);
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    if (tone) {
        if (!open_thr || !close_thr || !ratio) return set_error(FDC_ERR_INVALID_ARGUMENT, "tone squelch: no thresholds or ratios");
        if (!p->tones_T) return set_error(FDC_ERR_INVALID_ARGUMENT, "the tone squelch decides on the tones' frame rows: switch the channel tones on first (fdc_pipeline_set_tones)");
        if (!p->squelch_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "the tone squelch gates the squelch's mask: switch the channel squelch on first (fdc_pipeline_set_squelch)");
        if (guard < 0 || guard > 63) return set_error(FDC_ERR_INVALID_ARGUMENT, "tone squelch: the guard %d is not in 0 .. 63", (int)guard);
        if (hang_frames < 0 || hang_frames > 65535) return set_error(FDC_ERR_INVALID_ARGUMENT, "tone squelch: the hang count %d is not in 0 .. 65535 frames", (int)hang_frames);
        for (int c = 0; c < p->C; c++) {
            if (tone[c] < -1 || tone[c] >= p->tones_T)
                return set_error(FDC_ERR_INVALID_ARGUMENT, "tone squelch: the tone %d of channel %d is not in -1 .. %d", (int)tone[c], c, p->tones_T - 1);
            if (!std::isfinite(open_thr[c]) || !std::isfinite(close_thr[c]) || !std::isfinite(ratio[c]) || open_thr[c] < 0.0f || close_thr[c] < 0.0f || ratio[c] < 0.0f)
                return set_error(FDC_ERR_INVALID_ARGUMENT, "tone squelch: the thresholds and the ratio of channel %d are not finite and >= 0", c);
            if (close_thr[c] > open_thr[c])
                return set_error(FDC_ERR_INVALID_ARGUMENT, "tone squelch: the close threshold of channel %d is above its open threshold", c);
        }
    }
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!tone) {
        p->tsq_on = false; p->tsq_tone.clear(); p->tsq_open.clear(); p->tsq_close.clear(); p->tsq_ratio.clear(); p->tsq_guard = p->tsq_hang = 0;
        p->tsq_valid = false; p->tsq_blocks = -1; p->tsq_frames = 0; p->tsq_route.clear();
        return FDC_OK;
    }
    // everything the feature needs, once: the tone indices, three tables of thresholds, the two states, the decisions of the longest call from the
    // deepest fill on and their pinned twin
    const size_t nc = (size_t)p->C;
    const size_t nd = (((size_t)p->tones_W - 1 + (size_t)p->cfg.max_blocks) / (size_t)p->tones_W) * nc;
    if (nc > 0 && !p->d_tsqtone) HIPCHK(p->d_tsqtone.alloc(nc));
    for (int i = 0; i < 3; i++)
        if (nc > 0 && !p->d_tsqthr[i]) HIPCHK(p->d_tsqthr[i].alloc(nc));
    for (int i = 0; i < 2; i++)
        if (nc > 0 && !p->d_tsqstate[i]) HIPCHK(p->d_tsqstate[i].alloc(2 * nc));
    if (nd > p->d_tdec.capacity()) HIPCHK(p->d_tdec.reserve(nd, nd));
    if (nd > p->pin_tdec.capacity()) HIPCHK(p->pin_tdec.reserve(nd, nd));
    if (nc > 0) {
        HIPCHK(hipMemcpy(p->d_tsqtone, tone, sizeof(int32_t) * nc, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->d_tsqthr[0], open_thr, sizeof(float) * nc, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->d_tsqthr[1], close_thr, sizeof(float) * nc, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->d_tsqthr[2], ratio, sizeof(float) * nc, hipMemcpyHostToDevice));
    }
    p->tsq_tone.assign(tone, tone + nc);
    p->tsq_open.assign(open_thr, open_thr + nc);
    p->tsq_close.assign(close_thr, close_thr + nc);
    p->tsq_ratio.assign(ratio, ratio + nc);
    p->tsq_guard = guard; p->tsq_hang = hang_frames;
    p->tsq_valid = false; p->tsq_blocks = -1; p->tsq_frames = 0;      // a new setting: every channel starts closed, no call has decisions yet
    p->tsq_on = true;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_tone_squelch_setting(const fdc_pipeline *p, int32_t *tone, float *open_thr, float *close_thr, float *ratio, int32_t *guard,
                                      int32_t *hang_frames)
{
    FDC_ENTRY("fdc_pipeline_tone_squelch_setting")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (guard) *guard = p->tsq_on ? p->tsq_guard : -1;
    if (hang_frames) *hang_frames = p->tsq_on ? p->tsq_hang : -1;
    if (tone) std::copy(p->tsq_tone.begin(), p->tsq_tone.end(), tone);
    if (open_thr) std::copy(p->tsq_open.begin(), p->tsq_open.end(), open_thr);
    if (close_thr) std::copy(p->tsq_close.begin(), p->tsq_close.end(), close_thr);
    if (ratio) std::copy(p->tsq_ratio.begin(), p->tsq_ratio.end(), ratio);
    return FDC_OK;
    FDC_ENTRY_END
}

// the decisions of the frames the last call completed: never more than the caller says its buffer holds
int fdc_pipeline_tone_squelch(fdc_pipeline *p, uint8_t *dst, size_t capacity_bytes, int nblocks, int32_t *nframes)
{
    FDC_ENTRY("fdc_pipeline_tone_squelch")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->tsq_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "the tone squelch is off (fdc_pipeline_set_tone_squelch)");
    if (p->tsq_blocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "no work call has run since the tone squelch was switched on or its setting changed");
    if (nblocks != p->tsq_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "the last work call had %d blocks, not %d", p->tsq_blocks, nblocks);
    const size_t n = (size_t)p->tsq_frames * (size_t)p->C;
    if (capacity_bytes < n)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "the decisions of the %d frames of the last call take %zu bytes, the buffer holds %zu", p->tsq_frames, n, capacity_bytes);
    if (nframes) *nframes = p->tsq_frames;
    if (n == 0) return FDC_OK;
    if (!dst) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->tsq_host) {
        // a device entry's decisions: read behind everything enqueued so far on the stream it ran on
        HIPCHK(hipSetDevice(p->cfg.device_id));
        HIPCHK(hipMemcpyAsync(p->pin_tdec.get(), p->d_tdec.get(), n, hipMemcpyDeviceToHost, p->tsq_stream));
        HIPCHK(hipStreamSynchronize(p->tsq_stream));
        p->tsq_host = true;
    }
    std::memcpy(dst, p->pin_tdec.get(), n);
    return FDC_OK;
    FDC_ENTRY_END
}

void *fdc_pipeline_tone_squelch_device(fdc_pipeline *p) { return p && p->tsq_on ? static_cast<void *>(p->d_tdec.get()) : nullptr; }

// the decision and the gate alone, on the caller's device buffers: the handle gives its setting, the tones' T and W and its channel count, nothing of
// its stream state
int fdc_pipeline_tone_squelch_pass_device(const fdc_pipeline *p, const void *d_frames, void *d_dec, const void *d_state_in, void *d_state_out, void *d_mask,
                                          int32_t fill, int nblocks, void *stream)
{
    FDC_ENTRY("fdc_pipeline_tone_squelch_pass_device")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p->tsq_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "the tone squelch is off (fdc_pipeline_set_tone_squelch)");
    if (nblocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count");
    if (fill < 0 || fill >= p->tones_W) return set_error(FDC_ERR_INVALID_ARGUMENT, "the fill %d is not in 0 .. %d, the frame length - 1", (int)fill, p->tones_W - 1);
    if (nblocks == 0 || p->C <= 0) return FDC_OK;
    const bool rows = ((int64_t)fill + nblocks) / p->tones_W > 0;
    if (!d_state_out || (rows && (!d_frames || !d_dec))) return set_error(FDC_ERR_INVALID_ARGUMENT, "null device buffer");
    if (d_state_in == d_state_out) return set_error(FDC_ERR_INVALID_ARGUMENT, "the state is read from one buffer and written to another");
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(fdc::launch_tone_squelch(static_cast<const float2 *>(d_frames), p->d_tsqtone, p->d_tsqthr[0], p->d_tsqthr[1], p->d_tsqthr[2], p->tsq_guard, p->tsq_hang,
                                    static_cast<const int *>(d_state_in), static_cast<int *>(d_state_out), static_cast<unsigned char *>(d_dec),
                                    static_cast<unsigned char *>(d_mask), p->C, p->tones_T, p->tones_W, fill, nblocks,
                                    stream ? static_cast<hipStream_t>(stream) : p->stream));
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_tone_table(float *dst)
{
    FDC_ENTRY("fdc_tone_table")
    if (!dst) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<float2> tab((size_t)fdc::kToneTable);
    fdc::tone_table(tab.data());
    std::memcpy(dst, tab.data(), sizeof(float2) * tab.size());
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_set_gains(fdc_pipeline *p, const float *gain, int n)
{
    FDC_ENTRY("fdc_pipeline_set_gains")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (n != p->C) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel gains: %d gains for %d channels", n, p->C);
    if (p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a pipelined sinks batch is still inside the handle: fdc_pipeline_flush_sinks until it returns 0 first");
    bool on = false;
    for (int c = 0; gain && c < p->C; c++) {
        if (!std::isfinite(gain[c])) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel gains: the gain of channel %d is not finite", c);
        on = on || gain[c] != 1.0f;
    }
    if (!on) { p->gains_on = false; p->gains.clear(); p->gains_route.clear(); return FDC_OK; }
    HIPCHK(hipSetDevice(p->cfg.device_id));
    HIPCHK(hipStreamSynchronize(p->stream));          // (no call of the host entries is in flight; a device entry's caller orders its own stream)
    if (!p->d_gain) HIPCHK(p->d_gain.alloc((size_t)p->C));       // once: an AGC that sets new gains before every call allocates nothing
    HIPCHK(hipMemcpy(p->d_gain, gain, sizeof(float) * (size_t)p->C, hipMemcpyHostToDevice));
    if (p->gains.size() != (size_t)p->C) p->gains.resize((size_t)p->C);
    std::memcpy(p->gains.data(), gain, sizeof(float) * (size_t)p->C);
    p->gains_on = true;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_pipeline_gains(const fdc_pipeline *p, float *dst, int n)
{
    FDC_ENTRY("fdc_pipeline_gains")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (n != p->C) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel gains: room for %d gains of %d channels", n, p->C);
    if (n == 0) return FDC_OK;
    if (!dst) return set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    for (int c = 0; c < n; c++) dst[c] = p->gains_on ? p->gains[(size_t)c] : 1.0f;
    return FDC_OK;
    FDC_ENTRY_END
}

void *fdc_pipeline_lag1_device(fdc_pipeline *p) { return p && p->lag1_on ? static_cast<void *>(p->d_lag1.get()) : nullptr; }

void *fdc_pipeline_levels_device(fdc_pipeline *p) { return p && p->levels_on ? static_cast<void *>(p->d_levels.get()) : nullptr; }

}  // extern "C"
