// Stateful sinks fed with the normalised spectrum: a bank of PowerActivationChannel instances and the segments of an
// activity_detection_channelizer_vcm, sharing one device-resident spectrum (the hier block feeds all of them from the
// same normalize_input output, python/FrequencyDomainChannelizer.py:301-312).
//
// The data-parallel parts run on the GPU for a whole batch of blocks in every bank: per-(block, cell)
// power sums (k_cell_power) and the window * half-swap * IFFT * discard extractions (k_extract, grouped by width).  The
// per-block decisions between them — the work() loops of the reference blocks — have two engines:
//   * the DEVICE engine (fdc_sinks_dev.hip; its host side is here: dev_setup, dev_enqueue, dev_launch_extractions, dev_build,
//     dev_wait): the loops run as kernels, task lists, layout and buffered blocks stay on the device, batches go two deep
//     (fdc_sinks_submit_device / fdc_sinks_flush), payloads may stay in device memory or leave as sc16 / sc8.  The default.
//   * the HOST engine (fdc_sinks_host.hip): power cells to the host, state machines on host threads, extractions, payloads
//     assembled on the host; one synchronous batch per call.  The fall-back: a bank gets it with FDC_SINKS_HOST_DECISIONS,
//     with verbose != 0 (the reference's logs are written where the decisions fall), with a segment above kDetMaxCells cells
//     or tables beyond the device engine's budget (dev_setup decides; fdc_sinks_engine() reports).
// This file holds construction and destruction, every extern "C" entry, and what both engines share: the two ends of a batch
// (batch_begin, batch_end_history, batch_end_swap), the extraction launches (run_extractions) and the reference's logs.  The
// handle and its records are in fdc_sinks_state.hpp.  Behaviour follows lib/PowerActivationChannel_impl.cc and
// lib/activity_detection_channelizer_vcm_impl.cc; line references are given at each decision.  The `threads` flag of the
// reference sizes the host engine's worker pool and nothing else (GPU batching replaces the per-channel std::thread fan-out).
#include "fdc_sinks_state.hpp"
#include "fdc_guard.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

extern "C" const char *fdc_last_error(void);

using namespace fdc::sinks;

// body of an extern "C" entry: nothing thrown inside crosses the C boundary (fdc_guard.hpp)
#define FDC_ENTRY(name) return fdc::guarded(name, [&]() -> int {
#define FDC_ENTRY_END });

// the bank failed mid-call: remember why, refuse everything that follows
#define FDC_DEAD_CHECK(s)                                                                                                     \
    do {                                                                                                                      \
        if ((s)->poisoned)                                                                                                    \
            return fdc::set_error(FDC_ERR_HIP, "the bank failed in an earlier call and must be destroyed (%s)", (s)->poison_why.c_str()); \
    } while (0)

namespace {

bool ispow2i(int k) { return k > 0 && (k & (k - 1)) == 0; }

std::mutex g_log_mu;
fdc_log_fn g_log_fn = nullptr;
void *g_log_user = nullptr;

void start_logfile(const std::string &file)      // constructors: the file is truncated to one empty line
{
    FILE *f = std::fopen(file.c_str(), "w");
    if (!f) std::fprintf(stderr, "Logfile not writable: %s\n", file.c_str());
    else { std::fputc('\n', f); std::fclose(f); }
}

}  // namespace

namespace fdc { namespace sinks {

// get_current_time(), …vcm_impl.cc:56-69 / PowerActivationChannel_impl.cc:435-447 (the reference formats into char p[40]
// with a stated size of 80; 19 characters are written)
// One second of resolution: the string is formatted once per second and thread (localtime_r takes the C library's time-zone
// lock; a bank of 256 channels activates thousands of times per batch).
const std::string &current_time_string()
{
    thread_local time_t last = (time_t)-1;
    thread_local std::string text;
    const time_t t = time(nullptr);
    if (t != last) {
        char buf[40];
        struct tm tmv;
        localtime_r(&t, &tmv);
        strftime(buf, sizeof buf, "%Y-%m-%d-%H-%M-%S", &tmv);
        text = buf; last = t;
    }
    return text;
}

// log(), PowerActivationChannel_impl.cc:396-408 / …vcm_impl.cc:578-591: a line to stdout or appended to the log file
void sink_log(const fdc_sinks *s, const std::string &file, const std::string &line)
{
    {
        fdc_log_fn fn; void *user;
        { std::lock_guard<std::mutex> g(g_log_mu); fn = g_log_fn; user = g_log_user; }
        if (fn) fn(line.c_str(), user);
    }
    if (s->cfg.verbose == 1) { std::fputs(line.c_str(), stdout); std::fputc('\n', stdout); }
    else if (s->cfg.verbose == 2) {
        FILE *f = std::fopen(file.c_str(), "a");
        if (!f) std::fprintf(stderr, "Outputfile not writable: %s\n", file.c_str());
        else { std::fputs(line.c_str(), f); std::fputc('\n', f); std::fclose(f); }
    }
}

// ---- FDC_SINKS_LOOKAHEAD (see the struct): what a batch does at its two ends
// start of a batch: whatever its producer enqueued on the fill stream (forward transform, power cells) comes first
int batch_begin(fdc_sinks *s, int nblocks, bool *have_power)
{
    *have_power = false;
    if (!s->s_fill) {
        // one-buffer bank: fdc_sinks_prepare_from_groups has (enqueued, on this stream) the cells of exactly this batch
        *have_power = s->prepared == nblocks;
        s->prepared = -1;
        return FDC_OK;
    }
    if (s->prepared == nblocks) {
        // fdc_sinks_prepare marked the point of the fill stream where this batch is complete: what the producer has enqueued there SINCE
        // (the next batch's transform) is not waited for — it is what runs beside this batch's decisions
        HIPCHK(hipStreamWaitEvent(s->stream, s->ev_ready, 0));
        *have_power = true;
    } else {
        HIPCHK(hipEventRecord(s->ev_fill, s->s_fill));          // no mark: everything enqueued on the fill stream so far
        HIPCHK(hipStreamWaitEvent(s->stream, s->ev_fill, 0));
    }
    s->prepared = -1;
    return FDC_OK;
}
// end of a batch (enqueued behind its last reader): history <- its last block (save_hist, PowerActivationChannel_impl.cc:173;
// …vcm_impl.cc:571) — slot 0 of the buffer the NEXT batch is read from, which with look-ahead is the other one ...
int batch_end_history(fdc_sinks *s, int nblocks, hipStream_t q)
{
    const size_t N = (size_t)s->N;
    float2 *const next = s->d_spec_ahead ? s->d_spec_ahead : s->d_spec;
    HIPCHK(hipMemcpyAsync(next, s->d_spec + (size_t)nblocks * N, sizeof(float2) * N, hipMemcpyDeviceToDevice, q));
    return FDC_OK;
}
// ... then the buffers swap, and the fill stream may overwrite this batch's buffer once `done` (an event on the bank's stream behind the
// history copy; null: everything enqueued on it so far) has passed
int batch_end_swap(fdc_sinks *s, hipEvent_t done)
{
    if (!s->s_fill) return FDC_OK;
    if (done) HIPCHK(hipStreamWaitEvent(s->s_fill, done, 0));
    else { HIPCHK(hipEventRecord(s->ev_fill, s->stream)); HIPCHK(hipStreamWaitEvent(s->s_fill, s->ev_fill, 0)); }
    std::swap(s->d_spec, s->d_spec_ahead);
    std::swap(s->d_power, s->d_power_ahead);
    std::swap(s->d_gpow, s->d_gpow_ahead);
    std::swap(s->ev_ready, s->ev_ready_ahead);
    s->prepared = s->prepared_ahead; s->prepared_ahead = -1;
    return FDC_OK;
}

// Extractions of one call, one launch (or one gather / batched transform / scatter sequence) per width class.
// tasks: grouped by class, class k (width 2^k) = [first[k], first[k] + cnt[k])
// narrow: the fused payload route (every task is of the 256-bin class): the emitted runs [0, used_a) go to it in the bank's payload format
int run_extractions(fdc_sinks *s, const fdc::ExtractTask *d_tasks, const size_t *first, const size_t *cnt, float2 *d_out, bool trace,
                    hipStream_t q0, void *narrow, long long used_a)
{
    const int N = s->N;
    if (!q0) q0 = s->stream;
    // the classes that fit one workgroup's transform at 16 points per lane (w <= 4096; 256 has a kernel of its own) are independent and
    // each fills a part of the device only: two or more of them go out as ONE launch
    int mw[32], nm = 0;
    size_t mfirst[32], mcnt[32];
    for (int k = 0; k < 32; k++) {
        const int w = 1 << k;
        if (cnt[k] && w <= 4096 && !(w == 256 && s->d_tw256)) { mw[nm] = w; mfirst[nm] = first[k]; mcnt[nm] = cnt[k]; nm++; }
    }
    const bool multi = nm >= 2 && nm <= fdc::kMaxExtractClasses;
    // side streams (look-ahead banks): two or three classes above 4096 points, each in one piece of its own slice of the scratch
    int nwide = 0, wk[3] = {0, 0, 0};
    size_t wneed = 0;
    bool side = s->s_side[0] != nullptr;
    for (int k = 13; k < 32 && side; k++)
        if (cnt[k]) {
            if (nwide == 3 || cnt[k] * ((size_t)1 << k) > ((size_t)64 << 20)) { side = false; break; }
            wk[nwide++] = k; wneed += cnt[k] * ((size_t)1 << k);
        }
    side = side && nwide >= 2;
    if (side) {
        HIPCHK(s->d_wide.reserve(wneed, wneed + wneed / 2));
        HIPCHK(hipEventRecord(s->ev_fork, q0));
        size_t off = 0;
        for (int c = 0; c < nwide; c++) {
            const int k = wk[c], w = 1 << k;
            hipStream_t q = c == 0 ? q0 : s->s_side[c - 1];
            if (c) HIPCHK(hipStreamWaitEvent(q, s->ev_fork, 0));
            if (c == 0 && multi)        // the classes up to 4096 points go first on the bank's own stream, the widest class behind them
                HIPCHK(fdc::launch_extract_multi(s->d_spec, N, d_tasks, mw, mfirst, mcnt, nm, s->R, s->d_wins, d_out, s->d_tw, N, q0));
            HIPCHK(fdc::launch_extract_wide(s->d_spec, N, d_tasks + first[k], (int)cnt[k], w, w / s->R, s->d_wins, s->d_wide + off, d_out, s->d_tw, N, q));
            off += cnt[k] * (size_t)w;
            if (c) HIPCHK(hipEventRecord(s->ev_join[c - 1], q));
        }
    } else if (multi) HIPCHK(fdc::launch_extract_multi(s->d_spec, N, d_tasks, mw, mfirst, mcnt, nm, s->R, s->d_wins, d_out, s->d_tw, N, q0));
    for (int k = 0; k < 32; k++) {
        if (!cnt[k]) continue;
        const int w = 1 << k, skip = w / s->R;
        const size_t i = first[k], j = first[k] + cnt[k];
        if (trace) std::fprintf(stderr, "[fdc_sinks]     width %d: %zu tasks\n", w, j - i);
        if (multi && w <= 4096 && !(w == 256 && s->d_tw256)) continue;
        if (side && w > 4096) continue;
        if (w == 256 && s->d_tw256 && narrow) {
            HIPCHK(fdc::launch_extract256_narrow(s->pay_fmt, s->pay_scale, s->d_spec, N, d_tasks + i, (int)(j - i), skip, s->d_wins, d_out, narrow, used_a,
                                                 s->d_tw256, q0));
        } else if (w == 256 && s->d_tw256) {
            HIPCHK(fdc::launch_extract256(s->d_spec, N, d_tasks + i, (int)(j - i), skip, s->d_wins, d_out, s->d_tw256, q0));
        } else if (w <= 4096) {
            HIPCHK(fdc::launch_extract(s->d_spec, N, d_tasks + i, (int)(j - i), w, skip, s->d_wins, d_out, s->d_tw, N, q0));
        } else {
            // above 4096 points (a carrier, or a run of merged carriers, over 1/16 of a 65536-bin band): the two-pass inverse transform,
            // the whole class in batches of up to 64 Mi points — pass A reads slice * window straight from the spectrum (the half swap is
            // its input rotation), pass B writes [skip, w) to the landing offsets.  The scratch between the passes follows the demand
            // (batch x w points, grown geometrically), not the 64 Mi ceiling.  (One workgroup per 8192-point transform — 32 points per
            // lane, two workgroups per compute unit — was slower than the two passes: 98 us for the 536 extractions of a configs[4] step;
            // that class and the two above it took 271 us with a gathered copy and a scatter around the transform, 212 us this way.)
            const size_t per = std::min(std::max<size_t>(1, ((size_t)64 << 20) / (size_t)w), j - i);
            const size_t wcap = s->d_wide.capacity();
            HIPCHK(s->d_wide.reserve(per * (size_t)w, std::min(std::max(per * (size_t)w, wcap * 2), std::max<size_t>((size_t)64 << 20, (size_t)w))));
            const size_t fit = std::max<size_t>(1, s->d_wide.capacity() / (size_t)w);
            for (size_t k0 = i; k0 < j; k0 += fit) {
                const int n = (int)std::min(fit, j - k0);
                HIPCHK(fdc::launch_extract_wide(s->d_spec, N, d_tasks + k0, n, w, skip, s->d_wins, s->d_wide, d_out, s->d_tw, N, q0));
            }
        }
    }
    if (side) for (int c = 1; c < nwide; c++) HIPCHK(hipStreamWaitEvent(q0, s->ev_join[c - 1], 0));    // the bank's stream goes on behind every class
    return FDC_OK;
}

}}  // namespace fdc::sinks

namespace {

// ---------------------------------------------------------------- device engine: set-up
// Which engine a bank gets, and the device-side tables and lists of the device engine.  Every list is allocated for its
// worst case (a channel toggling in every block, a segment full of one-cell carriers), so no call can overflow one; a bank
// whose worst case does not fit a 2 GiB budget takes the host engine.
constexpr int kEagerPdus = 4096;

int dev_setup(fdc_sinks *s)
{
    auto &d = s->dev;
    const fdc_sinks_cfg &cfg = s->cfg;
    if ((cfg.flags & FDC_SINKS_HOST_DECISIONS) || cfg.verbose != 0) return FDC_OK;
    const int npac = (int)s->pacs.size(), nseg = (int)s->segs.size();
    if (npac + nseg == 0) return FDC_OK;
    {
        int capmax = 1;
        for (const Segment &g : s->segs) { if (g.ncell > fdc::kDetMaxCells) return FDC_OK; capmax = std::max(capmax, g.ncell / 2 + 1); }
        if (nseg && (capmax > 512 || fdc::det_track_staged(cfg.max_blocks, capmax) < 0)) return FDC_OK;   // the tracker's tables would not fit
    }
    const int64_t nbmax = cfg.max_blocks;
    d.carry_width = npac;
    for (const Segment &g : s->segs) d.carry_width = std::max(d.carry_width, std::min(g.ncell, fdc::kDetMaxCells));
    d.npw = npac;                                                              // one list per PowerActivationChannel (one wave each)
    d.nlist = d.npw + nseg;
    d.task_base.assign((size_t)d.nlist + 1, 0); d.pdu_base.assign((size_t)d.nlist + 1, 0);
    d.owner_base.assign((size_t)nseg + 1, npac); d.cand_base.assign((size_t)nseg + 1, 0);
    for (int l = 0; l < d.nlist; l++) {
        int64_t tc, pc;
        if (l < d.npw) { tc = 2 * nbmax; pc = nbmax; }                         // per block: at most two extractions, one emission
        else {
            const int64_t nc = s->segs[(size_t)(l - d.npw)].ncell;
            tc = nbmax * nc + nbmax * (nc / 2 + 1);                            // every live channel once, every activation twice
            pc = nbmax * nc;
        }
        d.task_base[(size_t)l + 1] = d.task_base[(size_t)l] + tc; d.pdu_base[(size_t)l + 1] = d.pdu_base[(size_t)l] + pc;
        d.max_list = std::max<long long>(d.max_list, tc);
    }
    for (int g = 0; g < nseg; g++) {
        const int64_t nc = s->segs[(size_t)g].ncell;
        d.owner_base[(size_t)g + 1] = d.owner_base[(size_t)g] + nc + nbmax * (nc / 2 + 1);
        d.cand_base[(size_t)g + 1] = d.cand_base[(size_t)g] + nbmax * (nc / 2 + 1);
    }
    const int64_t ntask = d.task_base.back(), npdu = d.pdu_base.back(), nown = d.owner_base.back(), ncand = d.cand_base.back();
    const int64_t bytes = ntask * (int64_t)(sizeof(fdc::SinkTask) + sizeof(fdc::ExtractTask)) + npdu * 2 * (int64_t)sizeof(fdc::SinkPdu) +
                          nown * (int64_t)sizeof(fdc::SinkOwner) + ncand * (int64_t)sizeof(int2);
    if (bytes > (2ll << 30)) return FDC_OK;
#define DALLOC(buf, n) HIPCHK((buf).alloc((size_t)(n)))
#define DUP(buf, vec) HIPCHK((buf).upload(vec))
    DUP(d.d_task_base, d.task_base); DUP(d.d_pdu_base, d.pdu_base); DUP(d.d_owner_base, d.owner_base); DUP(d.d_cand_base, d.cand_base);
    DALLOC(d.d_ntask, d.nlist); DALLOC(d.d_npdu, d.nlist); DALLOC(d.d_nowner, nseg + 1); DALLOC(d.d_error, 1); DALLOC(d.d_class_fill, 32);
    HIPCHK(hipMemset(d.d_error, 0, sizeof(int32_t)));
    HIPCHK(hipMemset(d.d_nowner, 0, sizeof(int32_t) * (size_t)(nseg + 1)));
    DALLOC(d.d_tasks, ntask); DALLOC(d.d_sorted, ntask); DALLOC(d.d_pdus, npdu); DALLOC(d.d_pdus_out, std::max<int64_t>(npdu, kEagerPdus)); DALLOC(d.d_owners, nown);
    DALLOC(d.d_sum, 1);
    DALLOC(d.h_sum, 1); DALLOC(d.h_pdus, kEagerPdus);
    if (npac) {
        std::vector<fdc::PacGeom> pg((size_t)npac);
        std::vector<fdc::PacState> ps((size_t)npac);
        for (int i = 0; i < npac; i++) {
            const Pac &p = s->pacs[(size_t)i];
            pg[(size_t)i] = fdc::PacGeom{p.cell, p.extract_start, p.extract_width, 31 - __builtin_clz((unsigned)p.extract_width), p.ovl_offset,
                                         p.output_len, p.deltaphase, p.win_off, p.ID, 0};
            fdc::PacState st{};
            st.lastpower = FLT_MAX;                                            // PowerActivationChannel_impl.cc:92
            ps[(size_t)i] = st;
        }
        DUP(d.d_pgeom, pg); DUP(d.d_pstate, ps);
    }
    if (nseg) {
        std::vector<fdc::DetGeom> dg((size_t)nseg);
        for (int g = 0; g < nseg; g++) {
            const Segment &sg = s->segs[(size_t)g];
            dg[(size_t)g] = fdc::DetGeom{sg.ID, sg.start, sg.ncell, sg.cell0, sg.ncell / 2 + 1, 0};
        }
        DUP(d.d_dgeom, dg);
        std::vector<fdc::DetSegState> st((size_t)nseg, fdc::DetSegState{0, 0});
        DUP(d.d_sst, st);
        DALLOC(d.d_live, (size_t)nseg * fdc::kDetFields * fdc::kDetMaxCells);
        DALLOC(d.d_live2, (size_t)nseg * fdc::kDetFields * fdc::kDetMaxCells);
        DALLOC(d.d_detch, nown);
        DALLOC(d.d_live_off, (size_t)nseg * fdc::kDetMaxCells);
        DALLOC(d.d_cand, ncand);
        DALLOC(d.d_ncand, (size_t)nseg * nbmax);
        std::vector<int32_t> wo(32, -1);
        for (size_t k = 0; k < s->det_win_off.size() && k < 32; k++) wo[k] = s->det_win_off[k];
        DUP(d.d_winoff, wo);
    }
#undef DUP
#undef DALLOC
    {
        // the payload copy's stream at the highest priority (its own hardware-queue pool: see the extraction streams in fdc_sinks_create): all it ever
        // carries are a wait, a copy and a mark, and behind a 250-us forward kernel on a shared queue they start a kernel late
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&d.s_copy, hipStreamNonBlocking, hi));
    }
    HIPCHK(hipEventCreateWithFlags(&d.ev_decide, hipEventDisableTiming));
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipEventCreateWithFlags(&d.ev_extract[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&d.ev_copied[i], hipEventDisableTiming));
    }
    d.on = true;
    return FDC_OK;
}

}  // namespace

extern "C" {

void fdc_sinks_destroy(fdc_sinks *s)
{
    if (!s) return;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->s_fill) { (void)hipStreamSynchronize(s->s_fill); (void)hipStreamDestroy(s->s_fill); }
    for (hipStream_t q : {s->s_side[0], s->s_side[1], s->s_x}) if (q) { (void)hipStreamSynchronize(q); (void)hipStreamDestroy(q); }
    for (hipEvent_t e : {s->ev_fill, s->ev_ready, s->ev_ready_ahead, s->ev_fork, s->ev_join[0], s->ev_join[1], s->ev_tasks}) if (e) (void)hipEventDestroy(e);
    {
        auto &d = s->dev;
        if (d.s_copy) { (void)hipStreamSynchronize(d.s_copy); (void)hipStreamDestroy(d.s_copy); }
        for (hipEvent_t e : {d.ev_decide, d.ev_extract[0], d.ev_extract[1], d.ev_copied[0], d.ev_copied[1]}) if (e) (void)hipEventDestroy(e);
    }
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;                                                  // the buffers go with it (fdc_buffers.hpp)
}

int fdc_sinks_create(const fdc_sinks_cfg *cfg, fdc_sinks **out)
{
    FDC_ENTRY("fdc_sinks_create")
    if (!cfg || !out) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const int N = cfg->blocklen, R = cfg->relinvovl;
    // shared predicates: PowerActivationChannel_impl.cc:64-70, …vcm_impl.cc:106-107,122-123
    if (N < 2 || !ispow2i(N)) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Blocklen invalid.");
    if (R < 1 || !ispow2i(R) || R > N) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Relative inverse overlap is invalid, must be >0 and a power of 2.");
    if (cfg->npac < 0 || cfg->nseg < 0 || (cfg->npac && !cfg->pac) || (cfg->nseg && !cfg->seg) || cfg->max_blocks < 1)
        return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "bad sink lists");
    std::unique_ptr<fdc_sinks> s(new fdc_sinks());
    s->cfg = *cfg; s->cfg.pac = nullptr; s->cfg.seg = nullptr;
    s->N = N; s->R = R;
    std::vector<cfl> pool;
    // ---- PowerActivationChannel instances
    if (cfg->npac > 0) {
        if (cfg->pac_thresh_db <= 0.0f)                                        // set_thresh, :377-381
            return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Threshold is interpreted as dB and must be >0.0");
        s->pac_thr = (float)std::pow(10.0, (double)cfg->pac_thresh_db / 10.0);
    }
    for (int i = 0; i < cfg->npac; i++) {
        float cfreq = cfg->pac[i].cfreq, bw = cfg->pac[i].bw;
        bw = bw > 0.0f ? bw : -bw;                                              // set_startstop, :314-355
        if (bw > 1.0 || cfreq - bw / 2.0f < 0.0f || cfreq + bw / 2.0f > 1.0f)
            return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Desired channel is out of band: cfreq=%f, bw=%f", cfreq, bw);
        const int k = (int)std::ceil((double)bw * (double)N);
        if (k <= 0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Can't eval nextpow2 from %d", k);
        Pac p;
        p.ID = cfg->pac[i].id;
        p.extract_width = std::min(pow2ceil(k), N);
        const int mid = (int)std::round((double)cfreq * (double)N);
        p.extract_start = std::max(0, mid - p.extract_width / 2);
        p.extract_stop = p.extract_start + p.extract_width;
        if (p.extract_stop > N) { p.extract_stop = N; p.extract_start = p.extract_stop - N; }   // reference clamp (App. B.2)
        p.measure_start = std::max((int)std::round((double)(cfreq - bw / 2.0f) * (double)N), p.extract_start);
        p.measure_stop = std::min((int)std::round((double)(cfreq + bw / 2.0f) * (double)N), p.extract_stop);
        if (p.extract_start + p.extract_width > N)
            return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "PowerActivationChannel %d: the reference reads past the block here", i);
        p.deltaphase = p.extract_start % R;
        p.ovl_offset = p.extract_width / R; p.output_len = p.extract_width - p.ovl_offset;
        // cr_windows, :357-375: unit phasor (float polar) with a rising sine edge; only the first extract_width
        // entries of the block-long table are ever used (:267), the mirrored far edge matters only when it falls inside.
        const int ramp = ((p.extract_stop - p.extract_start) - (p.measure_stop - p.measure_start)) / 3;
        p.win_off = (int)pool.size();
        pool.resize(pool.size() + (size_t)R * p.extract_width);
        for (int r = 0; r < R; r++) {
            const float ang = (float)(2.0f * M_PI * (double)r / (double)R);
            const cfl ph(std::cos(ang), std::sin(ang));
            std::vector<cfl> full((size_t)N, ph);
            for (int q = 0; q < ramp; q++) {
                full[q] *= (float)std::sin(0.5 * M_PI * (double)q / (double)(ramp + 1));
                full[N - q - 1] = full[q];
            }
            std::copy(full.begin(), full.begin() + p.extract_width, pool.begin() + p.win_off + (size_t)r * p.extract_width);
        }
        p.cell = (int)s->cells.size();
        s->cells.push_back({p.measure_start, std::max(0, p.measure_stop - p.measure_start), 1.0f, 0});
        s->pacs.push_back(std::move(p));
    }
    // ---- detection segments
    if (cfg->nseg > 0 && cfg->det_variant == 1) {
        // SegmentDetection face (lib/SegmentDetection_impl.cc:68-86, :592-637): one instance per segment in the hier block
        auto mod_f = [](float x) { return (float)std::fmod(std::fmod((double)x, 1.0) + 1.0, 1.0); };   // :700-703
        if (cfg->det_thresh_db < 0.0f) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Threshold is interpreted as dB and must be greater zero to detect channels accordingly.");
        if (cfg->window_flank_puffer < 0.0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Window flank puffer must not be smaller 0.0.");
        const float mcd = mod_f(cfg->minchandist);
        const double dd = (double)N * (double)mcd / 2.0;
        s->dec = dd < 2.0 ? 1 : (int)dd;
        s->det_thr = (float)std::pow(10.0, (double)cfg->det_thresh_db / 10.0);
        for (int i = 0; i < cfg->nseg; i++) {
            float a = mod_f(cfg->seg[i].start), b = mod_f(cfg->seg[i].stop);
            if (a == b) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Start must not be equal to stop.");
            if (a > b) std::swap(a, b);
            size_t width = (size_t)((double)(b - a) * (double)N);
            if (width % (size_t)s->dec) width += (size_t)s->dec - width % (size_t)s->dec;
            if (width > (size_t)N) width = (size_t)(N - N % s->dec);
            const size_t mid = (size_t)((double)(0.5f * (a + b)) * (double)N);
            size_t st = mid < width / 2 ? 0 : mid - width / 2, sp = st + width;
            if (sp > (size_t)N) { sp = (size_t)N; st = sp - (size_t)N; }                 // reference clamp (App. B.2)
            if (st + width > (size_t)N) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "segment %d: the reference reads past the block here", i);
            Segment g;
            g.ID = cfg->seg_id_base + i; g.start = (int)st; g.stop = (int)sp; g.width = (int)width;
            g.ncell = (int)width / s->dec; g.cell0 = (int)s->cells.size();
            for (int c = 0; c < g.ncell; c++) s->cells.push_back({g.start + c * s->dec, s->dec, 1.0f, 0});   // raw sums (:185-190)
            s->segs.push_back(std::move(g));
        }
    }
    if (cfg->nseg > 0 && cfg->det_variant != 1) {
        if (cfg->minchandist <= 0.0f || cfg->minchandist >= 1.0)               // :231-232
            return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Minimum channel distance is invalid. Must be in (0,1)");
        if (cfg->det_thresh_db < 0.0f) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Threshold is interpreted as dB and must be greater zero.");
        if (cfg->det_deactivation_delay < 0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Channel deactication delay must not be smaller 0.");
        if (cfg->window_flank_puffer < 0.0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Window flank puffer must not be smaller 0.0.");
        const double dd = (double)N * (double)cfg->minchandist / 2.0;           // :234-240
        s->dec = dd < 2.0 ? 1 : (int)dd;
        s->det_thr = (float)std::pow(10.0, (double)cfg->det_thresh_db / 10.0);
        for (int i = 0; i < cfg->nseg; i++) {                                   // create_segment, :248-279
            const float v0 = cfg->seg[i].start, v1 = cfg->seg[i].stop;
            if (v0 >= v1 || v0 < 0.0f || v1 > 1.0f) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Segment is incorrect: [%f, %f]", v0, v1);
            const int mid = std::abs((int)std::round(((double)v1 + (double)v0) * 0.5 * (double)N));
            int width = std::abs((int)std::round(((double)v1 - (double)v0) * (double)N));
            if (width % s->dec) width += s->dec - width % s->dec;
            if (width >= N) {
                if (N % s->dec == 0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "segment %d spans the whole block (the reference does not terminate here)", i);
                width = N - N % s->dec;
            }
            Segment g;
            g.ID = cfg->seg_id_base + i;
            g.start = mid - width / 2 <= 0 ? 0 : mid - width / 2;
            g.stop = g.start + width;
            if (g.stop > N) { g.stop = N; g.start = N - width; }
            if (g.start < 0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "Cannot evaluate start and stop of segment %d", i);
            g.width = width; g.ncell = width / s->dec; g.cell0 = (int)s->cells.size();
            const float norm = 1.0f / (float)s->dec;                            // :632
            for (int c = 0; c < g.ncell; c++) s->cells.push_back({g.start + c * s->dec, s->dec, norm, 0});
            s->segs.push_back(std::move(g));
        }
    }
    if (cfg->nseg > 0) {
        // cr_windows (…vcm_impl.cc:199-228, identical in SegmentDetection_impl.cc:551-583): every power-of-two width
        // x R phases, unit amplitude, Hann flanks
        const int nw = (int)std::log2((double)N) + 1;
        s->det_win_off.resize(nw);
        for (int k = 0; k < nw; k++) {
            const int ww = 1 << k, puf = (int)(cfg->window_flank_puffer * (double)ww);
            s->det_win_off[k] = -1;
            // widths above one workgroup's transform get a table only while it stays small (<= 32 MiB); carriers wider
            // than that are skipped at activation like the ones wider than the block
            if (ww > fdc::kMaxLdsFft && (size_t)R * ww * sizeof(cfl) > ((size_t)32 << 20)) continue;
            s->det_win_off[k] = (int)pool.size();
            pool.resize(pool.size() + (size_t)R * ww);
            for (int r = 0; r < R; r++) {
                cfl *w = pool.data() + s->det_win_off[k] + (size_t)r * ww;
                const double ang = 2.0 * M_PI * (double)r / (double)R;
                const cfl ph((float)std::cos(ang), (float)std::sin(ang));
                for (int n = 0; n < ww; n++) w[n] = ph;
                for (int q = 0; q < puf; q++) {
                    const float fl = 0.5f - 0.5f * (float)std::cos(M_PI * (double)q / (double)puf);
                    w[q] *= fl; w[ww - 1 - q] *= fl;
                }
            }
        }
    }
    int rc = fdc::pick_device(cfg->device_id);
    if (rc != FDC_OK) return rc;
    HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    fdc_sinks *raw = s.release();
#define CHKF(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { int _r = fdc::set_error(_e == hipErrorOutOfMemory ? FDC_ERR_NOMEM : FDC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); fdc_sinks_destroy(raw); return _r; } } while (0)
    CHKF(raw->d_spec.alloc(((size_t)cfg->max_blocks + 1) * N));
    CHKF(hipMemset(raw->d_spec, 0, sizeof(float2) * (size_t)N));            // zero history block (…cc:89 / :111)
    if (!pool.empty()) {
        CHKF(raw->d_wins.alloc(pool.size()));
        CHKF(hipMemcpy(raw->d_wins, pool.data(), sizeof(float2) * pool.size(), hipMemcpyHostToDevice));
    }
    {
        std::vector<float2> tw((size_t)N);
        for (int k = 0; k < N; k++) {
            const double a = -2.0 * M_PI * (double)k / (double)N;
            tw[k] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        CHKF(raw->d_tw.alloc((size_t)N));
        CHKF(hipMemcpy(raw->d_tw, tw.data(), sizeof(float2) * (size_t)N, hipMemcpyHostToDevice));
        if (N >= 256) {                                                        // width-256 extractions run on the register kernel
            std::vector<float2> t256(256);
            for (int j = 0; j < 256; j++) t256[(size_t)j] = tw[(size_t)j * (size_t)(N / 256)];
            CHKF(raw->d_tw256.alloc(256));
            CHKF(hipMemcpy(raw->d_tw256, t256.data(), sizeof(float2) * 256, hipMemcpyHostToDevice));
        }
    }
    if (!raw->cells.empty()) {
        CHKF(raw->d_cells.alloc(raw->cells.size()));
        CHKF(hipMemcpy(raw->d_cells, raw->cells.data(), sizeof(fdc::PowerCell) * raw->cells.size(), hipMemcpyHostToDevice));
        CHKF(raw->d_power.alloc(raw->cells.size() * (size_t)cfg->max_blocks));
    }
    if (!raw->cells.empty() && N >= 16) CHKF(raw->d_gpow.alloc((size_t)cfg->max_blocks * (size_t)(N / 16)));
    if (cfg->flags & FDC_SINKS_LOOKAHEAD) {
        if (raw->d_gpow) CHKF(raw->d_gpow_ahead.alloc((size_t)cfg->max_blocks * (size_t)(N / 16)));
        CHKF(raw->d_spec_ahead.alloc(((size_t)cfg->max_blocks + 1) * N));
        if (!raw->cells.empty()) CHKF(raw->d_power_ahead.alloc(raw->cells.size() * (size_t)cfg->max_blocks));
        CHKF(hipStreamCreateWithFlags(&raw->s_fill, hipStreamNonBlocking));
        CHKF(hipEventCreateWithFlags(&raw->ev_fill, hipEventDisableTiming));
        CHKF(hipEventCreateWithFlags(&raw->ev_ready, hipEventDisableTiming));
        CHKF(hipEventCreateWithFlags(&raw->ev_ready_ahead, hipEventDisableTiming));
        CHKF(hipEventCreateWithFlags(&raw->ev_fork, hipEventDisableTiming));
        // The extraction streams get the HIGHEST priority: the runtime maps streams onto a few hardware queues PER PRIORITY LEVEL, and at equal
        // priority the extraction stream shared one with the fill stream — a batch's extractions sat behind the NEXT batch's 250-us forward
        // kernel, whose successor in turn waits for those extractions to release the spectrum buffer (round 6, profiles/r06/timeline_cfg3_before.txt:
        // k_x256 started the moment the forward kernel ended; configs[2] 0.373 ms per 896 blocks for 0.27 of fill-stream work).  They are also the
        // work the buffer hand-over waits for: first in line is right.
        int prio_lo = 0, prio_hi = 0;
        CHKF(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        // (The payload copy's stream too, dev_setup: with the extraction stream gone from the normal pool the round robin put THAT one on the fill
        // stream's queue, and every step's copy started one forward kernel late: configs[2] 2.29 -> 2.55 ms, configs[4] 1.27 -> 1.53 per 896 blocks with
        // PDUs to host memory, profiles/r06/sched_ab.txt.)
        CHKF(hipStreamCreateWithPriority(&raw->s_x, hipStreamNonBlocking, prio_hi));
        CHKF(hipEventCreateWithFlags(&raw->ev_tasks, hipEventDisableTiming));
        for (int i = 0; i < 2; i++) {
            CHKF(hipStreamCreateWithPriority(&raw->s_side[i], hipStreamNonBlocking, prio_hi));
            CHKF(hipEventCreateWithFlags(&raw->ev_join[i], hipEventDisableTiming));
        }
    }
    raw->host_threads = cfg->threads > 0 ? std::min(cfg->threads, 32) : 0;
    raw->pay_all256 = raw->segs.empty() && !raw->pacs.empty() &&
                      std::all_of(raw->pacs.begin(), raw->pacs.end(), [](const Pac &p) { return p.extract_width == 256; });
    if (const char *t = fdc::debug_env("FDC_SINKS_THREADS")) if (atoi(t) >= 1) raw->host_threads = std::min(atoi(t), 32);   // debugging override
    {
        const int rcd = dev_setup(raw);
        if (rcd != FDC_OK) { fdc_sinks_destroy(raw); return rcd; }
    }
#undef CHKF
    // the tables and zeroed buffers above went through the null stream; the bank works on non-blocking streams of its own, which do not wait for it
    if (hipStreamSynchronize(nullptr) != hipSuccess) { (void)hipGetLastError(); fdc_sinks_destroy(raw); return fdc::set_error(FDC_ERR_HIP, "device synchronisation failed"); }
    // ---- logs of the constructors (verbose != 0)
    if (cfg->verbose) {
        fdc_sinks *const sp = raw;
        for (const Pac &pc : sp->pacs) {                                        // PowerActivationChannel_impl.cc:54-62, :113-127
            if (cfg->verbose == 2) start_logfile(pac_logfile(pc));
            const std::string bar("############################\n\n");
            sink_log(sp, pac_logfile(pc), bar + "# gr-FDC.PowActChan." + std::to_string(pc.ID) + "\n\n" + bar +
                     "# extract_start: " + std::to_string(pc.extract_start) + "\n# extract_stop: " + std::to_string(pc.extract_stop) +
                     "\n# extract_width: " + std::to_string(pc.extract_width) + "\n# measure_start: " + std::to_string(pc.measure_start) +
                     "\n# measure_stop: " + std::to_string(pc.measure_stop) + "\n\n# equivalent cfreq: " +
                     std::to_string((double)(pc.extract_start + pc.extract_width / 2) / (double)N) + "\n# equivalent bw: " +
                     std::to_string((double)pc.extract_width / (double)N) + "\n\n");
        }
        if (!sp->segs.empty()) {
            if (cfg->det_variant == 1) {                                        // SegmentDetection_impl.cc:49-61, :109-113
                const int id = cfg->det_id >= 0 && sp->segs.size() == 1 ? cfg->det_id : 0;
                sp->det_logfile = "gr-FDC.ActDetChan.ID_" + std::to_string(id) + ".log";
                if (cfg->verbose == 2) start_logfile(sp->det_logfile);
                for (const Segment &g : sp->segs) {
                    sink_log(sp, sp->det_logfile, "Threshold               " + std::to_string(sp->det_thr));
                    sink_log(sp, sp->det_logfile, "decimation factor       " + std::to_string(sp->dec));
                    sink_log(sp, sp->det_logfile, "start                   " + std::to_string(g.start));
                    sink_log(sp, sp->det_logfile, "stop                    " + std::to_string(g.stop));
                    sink_log(sp, sp->det_logfile, "width                   " + std::to_string(g.width));
                }
            } else {                                                            // …vcm_impl.cc:89-101, :176-186
                sp->det_logfile = "gr-FDC.ActDetChan.log";
                if (cfg->verbose == 2) start_logfile(sp->det_logfile);
                for (const Segment &g : sp->segs)
                    sink_log(sp, sp->det_logfile, "# Segment " + std::to_string(g.ID) + ": \n# start: " + std::to_string(g.start) +
                             " => f_start=" + std::to_string((double)g.start / (double)N) + "\n# stop: " + std::to_string(g.stop) +
                             " => f_stop=" + std::to_string((double)g.stop / (double)N) + "\n# width: " + std::to_string(g.width) +
                             " => f_bw=" + std::to_string((double)g.width / (double)N) + "\n# chan_decimation_fact: " +
                             std::to_string(sp->dec) + "\n");
            }
        }
    }
    *out = raw;
    return FDC_OK;
    FDC_ENTRY_END
}

void *fdc_sinks_spectrum(fdc_sinks *s) { return s ? (void *)(s->d_spec + s->N) : nullptr; }
void *fdc_sinks_stream(fdc_sinks *s) { return s ? (void *)s->stream : nullptr; }
void *fdc_sinks_spectrum_ahead(fdc_sinks *s) { return (s && s->d_spec_ahead) ? (void *)(s->d_spec_ahead + s->N) : nullptr; }
void *fdc_sinks_fill_stream(fdc_sinks *s) { return s ? (void *)s->s_fill : nullptr; }
int fdc_sinks_prepare(fdc_sinks *s, int nblocks, int ahead)
{
    FDC_ENTRY("fdc_sinks_prepare")
    if (!s) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    FDC_DEAD_CHECK(s);
    if (!s->s_fill) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "the bank was created without FDC_SINKS_LOOKAHEAD");
    if (nblocks <= 0 || nblocks > s->cfg.max_blocks) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d outside [1, max_blocks]", nblocks);
    if (!ahead && s->dev.eager_n > 0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "the batch in the current buffer was prepared before and its decisions are enqueued: submit it");
    HIPCHK(hipSetDevice(s->cfg.device_id));
    float2 *const spec = ahead ? s->d_spec_ahead : s->d_spec;
    float *const pw = ahead ? s->d_power_ahead : s->d_power;
    if (!ahead) {
        // the current buffer may have been filled on the bank's own stream (a batch 0 written there, fdc_sinks_work's copy): the cells wait for it
        HIPCHK(hipEventRecord(s->ev_fill, s->stream));
        HIPCHK(hipStreamWaitEvent(s->s_fill, s->ev_fill, 0));
    }
    if (!s->cells.empty()) HIPCHK(fdc::launch_cell_power(spec + s->N, s->N, s->d_cells, (int)s->cells.size(), nblocks, pw, s->s_fill));
    HIPCHK(hipEventRecord(ahead ? s->ev_ready_ahead : s->ev_ready, s->s_fill));
    (ahead ? s->prepared_ahead : s->prepared) = nblocks;
    return FDC_OK;
    FDC_ENTRY_END
}
void *fdc_sinks_group_power(fdc_sinks *s) { return s ? (void *)s->d_gpow : nullptr; }
void *fdc_sinks_group_power_ahead(fdc_sinks *s) { return s ? (void *)s->d_gpow_ahead : nullptr; }
int fdc_sinks_prepare_from_groups(fdc_sinks *s, int nblocks, int ahead)
{
    FDC_ENTRY("fdc_sinks_prepare_from_groups")
    if (!s) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    FDC_DEAD_CHECK(s);
    if (nblocks <= 0 || nblocks > s->cfg.max_blocks) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d outside [1, max_blocks]", nblocks);
    if (ahead && !s->s_fill) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "the bank was created without FDC_SINKS_LOOKAHEAD");
    if (!ahead && s->dev.eager_n > 0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "the batch in the current buffer was prepared before and its decisions are enqueued: submit it");
    float *const gp = ahead ? s->d_gpow_ahead : s->d_gpow;
    if (!s->cells.empty() && !gp) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "the bank has no group-power buffer (block length below 16)");
    HIPCHK(hipSetDevice(s->cfg.device_id));
    float2 *const spec = ahead ? s->d_spec_ahead : s->d_spec;
    float *const pw = ahead ? s->d_power_ahead : s->d_power;
    // look-ahead banks: on the fill stream, behind what the producer enqueued there; other banks: on the bank's own stream (the producer
    // wrote spectrum and group powers on a stream it has synchronised, or on this one: fdc_sinks_spectrum's contract)
    hipStream_t q = s->s_fill ? s->s_fill : s->stream;
    if (s->s_fill && !ahead) {
        HIPCHK(hipEventRecord(s->ev_fill, s->stream));
        HIPCHK(hipStreamWaitEvent(s->s_fill, s->ev_fill, 0));
    }
    if (!s->cells.empty()) HIPCHK(fdc::launch_cell_power_groups(spec + s->N, gp, s->N, s->d_cells, (int)s->cells.size(), nblocks, pw, q));
    if (s->s_fill) HIPCHK(hipEventRecord(ahead ? s->ev_ready_ahead : s->ev_ready, s->s_fill));
    (ahead ? s->prepared_ahead : s->prepared) = nblocks;
    return FDC_OK;
    FDC_ENTRY_END
}
int32_t fdc_sinks_blocklen(const fdc_sinks *s) { return s ? s->N : -1; }
int32_t fdc_sinks_max_blocks(const fdc_sinks *s) { return s ? s->cfg.max_blocks : -1; }

int fdc_sinks_pac_params(const fdc_sinks *s, int i, int32_t *v)
{
    FDC_ENTRY("fdc_sinks_pac_params")
    if (!s || i < 0 || i >= (int)s->pacs.size() || !v) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "bad index");
    const Pac &p = s->pacs[i];
    v[0] = p.extract_start; v[1] = p.extract_stop; v[2] = p.extract_width; v[3] = p.measure_start; v[4] = p.measure_stop;
    v[5] = p.output_len; v[6] = p.ovl_offset; v[7] = p.deltaphase;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_sinks_segment_params(const fdc_sinks *s, int i, int32_t *v)
{
    FDC_ENTRY("fdc_sinks_segment_params")
    if (!s || i < 0 || i >= (int)s->segs.size() || !v) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "bad index");
    const Segment &g = s->segs[i];
    v[0] = g.start; v[1] = g.stop; v[2] = g.width; v[3] = s->dec; v[4] = g.ncell;
    return FDC_OK;
    FDC_ENTRY_END
}

// ---------------------------------------------------------------- device engine: a call
// dev_enqueue(): power cells, decision kernels, layout — nothing here waits for the device.  dev_launch_extractions(): needs
// the summary of the layout kernel (buffer sizes, tasks per width class) on the host, then enqueues the rest: placement of the
// tasks, blocks buffered from the call before, extraction kernels, history block, and the copy of the emitted runs to the host
// on a stream of its own.  dev_complete(): waits for that copy and turns the emission records into fdc_pdu.
// ahead: the chain of the batch that sits PREPARED in the ahead buffer (look-ahead banks, enqueued by the submit in front of it): its power cells are
// marked by ev_ready_ahead
static int dev_enqueue(fdc_sinks *s, int nblocks, bool ahead = false)
{
    auto &d = s->dev;
    const int N = s->N, ncells = (int)s->cells.size(), npac = (int)s->pacs.size(), nseg = (int)s->segs.size();
    const long long now = (long long)time(nullptr), bc0 = s->blockcount;
    bool have_power = false;
    float *const d_power = ahead ? s->d_power_ahead : s->d_power;
    if (ahead) {
        HIPCHK(hipStreamWaitEvent(s->stream, s->ev_ready_ahead, 0));
        s->prepared_ahead = -1;                                    // consumed: after the swap the batch is no longer "prepared", its chain is out
        have_power = true;
    } else { const int rb = batch_begin(s, nblocks, &have_power); if (rb != FDC_OK) return rb; }
    if (ncells && !have_power) HIPCHK(fdc::launch_cell_power(s->d_spec + N, N, s->d_cells, ncells, nblocks, d_power, s->stream));
    HIPCHK(fdc::launch_pac_decide(d_power, ncells, nblocks, d.d_pgeom, d.d_pstate, npac, s->pac_thr, s->cfg.pac_maxblocks, s->R, bc0, now,
                                  d.d_tasks, d.d_pdus, d.d_task_base, d.d_pdu_base, d.d_ntask, d.d_npdu, d.d_owners, s->stream));
    if (nseg) {
        const int sd = s->cfg.det_variant == 1;
        HIPCHK(fdc::launch_det_cands(d_power, ncells, nblocks, d.d_dgeom, nseg, s->dec, s->det_thr, sd, d.d_cand, d.d_cand_base,
                                     d.d_ncand, s->cfg.max_blocks, s->stream));
        fdc::DetParams dp{};
        dp.N = N; dp.R = s->R; dp.dec = s->dec; dp.variant = sd; dp.maxblocks = s->cfg.det_maxblocks; dp.delay = s->cfg.det_deactivation_delay;
        dp.nseg = nseg; dp.npac = npac; dp.nbmax = s->cfg.max_blocks; dp.puffer = s->cfg.window_flank_puffer;
        dp.mb_shift = (dp.maxblocks >= 2 && (dp.maxblocks & (dp.maxblocks - 1)) == 0) ? 31 - __builtin_clz((unsigned)dp.maxblocks) : -1;
        dp.max_cand_cap = 1;
        for (const Segment &g : s->segs) dp.max_cand_cap = std::max(dp.max_cand_cap, g.ncell / 2 + 1);
        dp.segname0 = s->cfg.det_id;
        HIPCHK(fdc::launch_det_track(dp, nblocks, d.d_dgeom, d.d_sst, d.d_live, d.d_live_off, d.d_cand, d.d_cand_base, d.d_ncand, d.d_winoff,
                                     now, d.d_pdus, d.d_pdu_base, d.d_npdu, d.d_owners, d.d_owner_base, d.d_nowner, d.d_detch, d.d_live2,
                                     d.d_error, s->stream));
        HIPCHK(fdc::launch_det_expand(nseg, npac, s->R, d.d_owners, d.d_owner_base, d.d_nowner, d.d_tasks, d.d_task_base, d.d_ntask, s->stream));
    }
    HIPCHK(fdc::launch_sink_layout(d.nlist, d.d_task_base, d.d_pdu_base, d.d_ntask, d.d_npdu, d.d_tasks, d.d_pdus, d.d_pdus_out, d.d_owners,
                                   npac, nseg, d.d_owner_base, d.d_nowner, d.d_pstate, d.d_sst, d.d_live, d.d_live_off, d.d_sum,
                                   d.d_class_fill, d.d_error, s->stream));
    HIPCHK(fdc::launch_sink_publish(d.d_sum, d.d_pdus_out, d.h_sum, d.h_pdus, kEagerPdus, s->stream));
    HIPCHK(hipEventRecord(d.ev_decide, s->stream));
    s->blockcount = bc0 + nblocks;
    return FDC_OK;
}

static int dev_launch_extractions(fdc_sinks *s, int nblocks)
{
    auto &d = s->dev;
    static const bool trace = fdc::debug_env("FDC_SINKS_TRACE") != nullptr;
    const int npac = (int)s->pacs.size(), nseg = (int)s->segs.size();
    HIPCHK(hipEventSynchronize(d.ev_decide));
    const int64_t bc0_this = s->blockcount - nblocks;          // block counter at the start of THIS batch (the next batch's chain may advance it below)
    const int b = d.cur ^ 1;                                   // this call's landing buffer; d.cur still names the previous call's
    const fdc::SinkSummary sum = *d.h_sum;
    if (sum.error) {
        HIPCHK(hipMemsetAsync(d.d_error, 0, sizeof(int32_t), s->stream));
        return fdc::set_error(FDC_ERR_UNSUPPORTED, "detection: more than %d live channels in one segment", fdc::kDetMaxCells);
    }
    d.sum[b] = sum;
    d.recs[b].assign(d.h_pdus.get(), d.h_pdus.get() + std::min(sum.npdu, kEagerPdus));
    if (sum.npdu > kEagerPdus) {
        d.recs[b].resize((size_t)sum.npdu);
        HIPCHK(hipMemcpyAsync(d.recs[b].data() + kEagerPdus, d.d_pdus_out + kEagerPdus, sizeof(fdc::SinkPdu) * (size_t)(sum.npdu - kEagerPdus),
                              hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    const bool devpay = (s->cfg.flags & FDC_SINKS_DEVICE_PAYLOAD) != 0;
    // the buffer last held call k-2: its copy to the host was waited for when that call was completed, its buffered blocks were
    // moved on by call k-1 (enqueued; hipFree waits for the device)
    // grown to 3/2 of the demand, at least 64 Ki samples
    auto roomy = [](size_t n) { return std::max<size_t>(n * 3 / 2, (size_t)1 << 16); };
    HIPCHK(d.d_land[b].reserve((size_t)sum.used_total, roomy((size_t)sum.used_total)));
    // Payload format (fdc_sinks_set_payload_format).  FUSED: every extraction of the batch is of the 256-bin class, whose kernel has narrow stores — it and
    // the move of the buffered blocks write the emitted runs narrow themselves, and [0, used_a) of the float buffer is never written: nothing reads it (the
    // payload comes from the narrow buffer, and what the NEXT batch moves on lies at prev_off = tail_off / live_off = an owner's b_off, k_sink_layout: always
    // in [b_start, used_total)).  NARROWED: any other mix of classes runs as ever, and one pass narrows [0, used_a) behind the extractions.
    const int fmt = s->pay_fmt;
    const size_t sbytes = fdc::iq_bytes(fmt);
    // A batch without extractions (only buffered blocks go out, or nothing does) takes the route of the bank's own kind: fused for a bank that is
    // nothing but 256-bin PowerActivationChannels, narrowed for every other one.
    bool fused = fmt != fdc::kIqFloat && s->d_tw256 != nullptr && (sum.class_cnt[8] > 0 || s->pay_all256);
    for (int k = 0; k < 32 && fused; k++) if (k != 8 && sum.class_cnt[k]) fused = false;
    d.fmt_of[b] = fmt; d.route_of[b] = fmt == fdc::kIqFloat ? 0 : fused ? 2 : 1;
    const size_t used_a = (size_t)sum.used_a;
    if (fmt != fdc::kIqFloat) HIPCHK(d.d_nland[b].reserve(used_a * sbytes, roomy(used_a) * sbytes));
    if (fmt != fdc::kIqFloat && !devpay) HIPCHK(d.h_nland[b].reserve(used_a * sbytes, roomy(used_a) * sbytes));
    if (fmt == fdc::kIqFloat && !devpay) HIPCHK(d.h_land[b].reserve(used_a, roomy(used_a)));
    // look-ahead banks: the extractions run on their own stream.  The batch before's may still be at work there: its landing buffer (the
    // buffered blocks move on from it) and the sorted task list (about to be rewritten) are its to read until it is done
    hipStream_t qx = s->s_x ? s->s_x : s->stream;
    if (s->s_x && d.any) HIPCHK(hipStreamWaitEvent(s->stream, d.ev_extract[d.cur], 0));
    if (sum.ntask)
        // grids from what the layout found, not from the worst case the lists were allocated for
        HIPCHK(fdc::launch_task_scatter(d.nlist, d.d_task_base, d.d_ntask, std::min<long long>(d.max_list, std::max(1, sum.max_list_tasks)), d.d_tasks,
                                        d.d_owners, d.d_sum, d.d_class_fill, d.d_sorted, s->stream));
    if (d.any && sum.ncarry > 0) {
        const int nown = std::min(d.carry_width, std::max(1, sum.max_region_owners));
        if (fused)
            HIPCHK(fdc::launch_carry_copy_narrow(fmt, s->pay_scale, d.d_owners, nown, d.d_owner_base, d.d_nowner, npac, nseg, d.d_land[d.cur], d.d_land[b],
                                                 d.d_nland[b], s->stream));
        else
            HIPCHK(fdc::launch_carry_copy(d.d_owners, nown, d.d_owner_base, d.d_nowner, npac, nseg, d.d_sum, d.d_land[d.cur], d.d_land[b], s->stream));
    }
    if (s->s_x) {
        HIPCHK(hipEventRecord(s->ev_tasks, s->stream));
        HIPCHK(hipStreamWaitEvent(qx, s->ev_tasks, 0));
    }
    // Look-ahead banks: the NEXT batch is already transformed and its power cells are (being) summed (fdc_sinks_prepare(.., ahead) came before this
    // submit): its decision chain goes out NOW, behind this batch's task placement on the bank's stream — the decision arrays are free from there on, the
    // host has its copy of this batch's summary and records — instead of when the caller comes back with the next submit, and in front of this batch's
    // extraction launches: the chain is the long pole of a detector's step (k_det_track: 0.3 ms on two compute units) and used to start a host lap late
    // (profiles/r06/timeline_cfg5_before.txt: 220 us between the end of one k_det_track and the start of the next).  The submit that follows must be
    // for exactly that batch.
    if (s->s_fill && s->prepared_ahead > 0) {
        const int n_next = s->prepared_ahead;
        const int re = dev_enqueue(s, n_next, true);
        if (re != FDC_OK) return re;
        d.eager_n = n_next;
    }
    if (sum.ntask) {
        size_t first[32], cnt[32];
        for (int k = 0; k < 32; k++) { first[k] = (size_t)sum.class_base[k]; cnt[k] = (size_t)sum.class_cnt[k]; }
        const int rce = run_extractions(s, d.d_sorted, first, cnt, d.d_land[b], trace, qx, fused ? d.d_nland[b].get() : nullptr, (long long)sum.used_a);
        if (rce != FDC_OK) return rce;
    }
    if (fmt != fdc::kIqFloat && !fused) HIPCHK(fdc::launch_complex_to_iq(fmt, s->pay_scale, d.d_land[b], d.d_nland[b], (size_t)sum.used_a, qx));
    { const int rh = batch_end_history(s, nblocks, qx); if (rh != FDC_OK) return rh; }
    HIPCHK(hipEventRecord(d.ev_extract[b], qx));
    { const int rh = batch_end_swap(s, d.ev_extract[b]); if (rh != FDC_OK) return rh; }
    if (!devpay && sum.used_a) {
        HIPCHK(hipStreamWaitEvent(d.s_copy, d.ev_extract[b], 0));
        if (fmt != fdc::kIqFloat) HIPCHK(hipMemcpyAsync(d.h_nland[b], d.d_nland[b], sbytes * (size_t)sum.used_a, hipMemcpyDeviceToHost, d.s_copy));
        else HIPCHK(hipMemcpyAsync(d.h_land[b], d.d_land[b], sizeof(float2) * (size_t)sum.used_a, hipMemcpyDeviceToHost, d.s_copy));
        HIPCHK(hipEventRecord(d.ev_copied[b], d.s_copy));
    }
    d.cur = b; d.any = true; d.inflight = true; d.pend[b] = true; d.nb_of[b] = nblocks; d.bc0[b] = bc0_this;
    if (trace) std::fprintf(stderr, "[fdc_sinks dev] %d tasks, %d PDUs, %lld samples emitted, %lld buffered\n", sum.ntask, sum.npdu,
                            (long long)sum.used_a, (long long)(sum.used_total - sum.b_start));
    return FDC_OK;
}

// The PDUs of the batch in landing buffer b become the handle's current PDUs.  Two halves: dev_build() turns the emission records
// into fdc_pdu (host work only: needs the records and the layout, not the payload bytes — it runs while the device works on the
// next batch), dev_wait() waits for the payload (its copy to the host, or the extraction kernels when it stays on the device).
static int dev_wait(fdc_sinks *s, int b)
{
    auto &d = s->dev;
    if (!d.pend[b]) return 0;
    const bool devpay = (s->cfg.flags & FDC_SINKS_DEVICE_PAYLOAD) != 0;
    if (!devpay && d.sum[b].used_a) HIPCHK(hipEventSynchronize(d.ev_copied[b]));
    else HIPCHK(hipEventSynchronize(d.ev_extract[b]));
    d.pend[b] = false;
    d.inflight = d.pend[0] || d.pend[1];
    s->pay_route = d.route_of[b];
    return d.nb_of[b];
}

static int dev_build(fdc_sinks *s, int b)
{
    auto &d = s->dev;
    if (!d.pend[b]) return 0;
    const bool devpay = (s->cfg.flags & FDC_SINKS_DEVICE_PAYLOAD) != 0;
    std::vector<fdc::SinkPdu> &recs = d.recs[b];
    // emission order = key order; the records stay where they are, (key, index) pairs are sorted (16 bytes a piece instead of 56)
    std::vector<std::pair<int64_t, uint32_t>> &order = d.order;
    order.resize(recs.size());
    for (size_t i = 0; i < recs.size(); i++) order[i] = {recs[i].key, (uint32_t)i};
    std::sort(order.begin(), order.end());
    const bool narrow = d.fmt_of[b] != fdc::kIqFloat;       // the narrow landing buffers: same sample offsets, their own sample size
    const size_t sbytes = fdc::iq_bytes(d.fmt_of[b]);
    const void *const land = devpay ? (narrow ? (void *)d.d_nland[b].get() : (void *)d.d_land[b].get())
                                    : (narrow ? (void *)d.h_nland[b].get() : (void *)d.h_land[b].get());
    const char *base = static_cast<const char *>(land);
    s->pdus.resize(recs.size());
    time_t last_t = (time_t)-1;
    char tbuf[40] = "";
    const bool sd = s->cfg.det_variant == 1;
    for (size_t i = 0; i < recs.size(); i++) {
        const fdc::SinkPdu &r = recs[order[i].second];
        PduRec &o = s->pdus[i];
        o.blocks.clear(); o.payload.clear(); o.key = r.key;
        fdc_pdu &m = o.meta;
        m = fdc_pdu{};
        const bool det = (r.flags >> 16) & 1;
        const int64_t blk = r.key >> fdc::kKeyShiftDev;        // block index inside the batch
        int width, vstart, vend;
        if (!det) {
            const Pac &p = s->pacs[(size_t)r.owner];
            // extract_stop, not extract_start + extract_width: they differ after the reference's clamp (…_impl.cc:333-336, :226)
            width = p.extract_width; vstart = p.extract_start; vend = p.extract_stop;
            m.kind = 0; m.source = p.ID; m.has_part = 1;
            m.blockend = d.bc0[b] + blk;                       // blockcount while the item is processed (:226-227)
        } else {
            const int sgi = (int)((r.key >> fdc::kKeySegShiftDev) & 0x7FF);
            width = 1 << ((r.flags >> 8) & 0xFF); vstart = r.vstart; vend = vstart + width;
            m.kind = 1;
            m.source = (sd && s->cfg.det_id >= 0 && s->segs.size() == 1) ? s->cfg.det_id : s->segs[(size_t)sgi].ID;
            m.has_part = (r.flags & 1) ? (r.part > 0) : 1;     // …vcm_impl.cc:419-420
            // the vcm block counts from 1 (…vcm_impl.cc:188), SegmentDetection from 0 (SegmentDetection_impl.cc:118)
            m.blockend = d.bc0[b] + blk - (sd ? 1 : 0);
        }
        o.blocklen = width - width / s->R;
        m.chan_id = r.chan_id; m.finalized = r.flags & 1; m.part = r.part;
        m.rel_bw = (double)width / (double)s->N;
        m.rel_cfreq = (double)(vstart + vend) / 2.0 / (double)s->N;
        // the vcm block's counter is `unsigned int`: blockcount - count wraps at 2^32 for a channel activated in the first item (det_emit)
        m.blockstart = (det && !sd) ? (int64_t)(uint32_t)(m.blockend - r.count) : m.blockend - r.count;
        m.vectorstart = vstart; m.vectorend = vend;
        m.nsamples = (int64_t)(r.q1 - r.q0) * o.blocklen;
        m.samples = m.nsamples ? base + sbytes * (size_t)r.off : nullptr;
        if ((time_t)r.act_time != last_t) {                    // create_ID() / get_ID_for_msg(): local time of the activation
            last_t = (time_t)r.act_time;
            struct tm tmv;
            localtime_r(&last_t, &tmv);
            strftime(tbuf, sizeof tbuf, "%Y-%m-%d-%H-%M-%S", &tmv);
        }
        // "<time>.PowActChan.<ID>.<n>" / "<time>.DETECTED.<segment>.<n>": thousands per batch, and in device-payload mode this loop is what
        // the step waits for on a slow host — digits by hand instead of snprintf
        {
            char *q = m.id, *const qe = m.id + sizeof m.id - 1;
            auto put = [&](const char *t) { while (*t && q < qe) *q++ = *t++; };
            auto num = [&](int v) {
                char tmp[12]; int n = 0;
                unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
                do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
                if (v < 0 && q < qe) *q++ = '-';
                while (n && q < qe) *q++ = tmp[--n];
            };
            put(tbuf); put(det ? ".DETECTED." : ".PowActChan."); num(m.source); put("."); num(r.chan_id);
            *q = 0;
        }
    }
    return d.nb_of[b];
}

// What every batch entry checks first: the handle, that it is alive, the batch size (`what` names the argument in the message), and
// where `flags` ask for it that no submitted batch is in flight and that no batch prepared ahead has its decisions enqueued.
enum { kNotInFlight = 1, kNotEager = 2 };
static int batch_entry_check(const fdc_sinks *s, const char *what, int n, int flags)
{
    if (!s) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    FDC_DEAD_CHECK(s);
    if (n < 0 || n > s->cfg.max_blocks) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "%s %d outside [0, max_blocks]", what, n);
    if ((flags & kNotInFlight) && s->dev.on && s->dev.inflight) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "a submitted batch is in flight: fdc_sinks_flush() first");
    if ((flags & kNotEager) && s->dev.eager_n > 0) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "a batch prepared ahead has its decisions enqueued: submit it before feeding the bank from the host");
    return FDC_OK;
}

// rc < 0 from a step that may have advanced the bank's state: the handle is dead (see fdc_sinks::poisoned)
static int poison(fdc_sinks *s, int rc)
{
    if (rc < 0 && !s->poisoned) {
        s->poisoned = true;
        try { s->poison_why = fdc_last_error(); } catch (...) {}
    }
    return rc;
}

static int dev_complete(fdc_sinks *s, int b)
{
    const int rc = dev_build(s, b);
    return rc <= 0 ? rc : dev_wait(s, b);
}

int fdc_sinks_submit_device(fdc_sinks *s, int nblocks)
{
    FDC_ENTRY("fdc_sinks_submit_device")
    { const int rc0 = batch_entry_check(s, "nblocks", nblocks, 0); if (rc0 != FDC_OK) return rc0; }
    if (!s->dev.on) {                                          // host engine: the batch is done when the call returns
        if (nblocks == 0) { s->pdus.clear(); return 0; }
        HIPCHK(hipSetDevice(s->cfg.device_id));
        return poison(s, host_work_device(s, nblocks));
    }
    HIPCHK(hipSetDevice(s->cfg.device_id));
    auto &d = s->dev;
    if (nblocks == 0) {
        const int done = poison(s, dev_complete(s, d.cur));
        if (done == 0) s->pdus.clear();
        return done;
    }
    // This batch's decision kernels are enqueued; while the device runs them the PDUs of the batch before are built (host work);
    // then the one wait for the layout summary, the extractions of this batch, and last the wait for the payload of the batch
    // before — its copy has been running beside all of that.
    // From the first launch of dev_enqueue on, the channel state on the device, the block counter and the layout of this batch's
    // landing buffer have moved on: a failure anywhere below leaves them ahead of the host's bookkeeping (d.cur, d.pend), so it
    // poisons the handle instead of returning an error that invites a retry.
    int rc;
    if (d.eager_n > 0) {
        // the chain of this batch went out at the end of the submit before (dev_launch_extractions): the state has advanced for exactly eager_n blocks
        if (nblocks != d.eager_n) {
            fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "a batch of %d blocks was prepared ahead and its decisions are enqueued: the submit must be for it, not for %d blocks", d.eager_n, nblocks);
            return poison(s, FDC_ERR_INVALID_ARGUMENT);
        }
        d.eager_n = 0;
    } else {
        rc = poison(s, dev_enqueue(s, nblocks));
        if (rc != FDC_OK) return rc;
    }
    const int before = d.cur;
    const bool had = d.pend[before];
    if (had) { rc = poison(s, dev_build(s, before)); if (rc < 0) return rc; }
    else s->pdus.clear();
    rc = poison(s, dev_launch_extractions(s, nblocks));
    if (rc != FDC_OK) return rc;
    return had ? poison(s, dev_wait(s, before)) : 0;
    FDC_ENTRY_END
}

int fdc_sinks_flush(fdc_sinks *s)
{
    FDC_ENTRY("fdc_sinks_flush")
    if (!s) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    FDC_DEAD_CHECK(s);
    if (!s->dev.on || !s->dev.inflight) return 0;
    HIPCHK(hipSetDevice(s->cfg.device_id));
    return poison(s, dev_complete(s, s->dev.cur));
    FDC_ENTRY_END
}

int32_t fdc_sinks_engine(const fdc_sinks *s) { return s ? (s->dev.on ? 1 : 0) : -1; }

int fdc_sinks_set_payload_format(fdc_sinks *s, int32_t format, float scale)
{
    FDC_ENTRY("fdc_sinks_set_payload_format")
    if (!s) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    FDC_DEAD_CHECK(s);
    if (format != FDC_OQ_FC32 && format != FDC_OQ_SC16 && format != FDC_OQ_SC8)
        return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "unknown payload format %d (FDC_OQ_FC32, FDC_OQ_SC16 or FDC_OQ_SC8)", (int)format);
    if (!(std::isfinite(scale) && scale != 0.0f)) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "the payload scale must be finite and not zero");
    // a batch under way was laid out (and maybe narrowed) for the format it met: flush first.  A pipelined fdc_pipeline_work_sinks that holds batches
    // of the bank shows here too: its newest batch sits prepared in one of the spectrum buffers, the one before is in flight
    if (s->dev.inflight || s->dev.eager_n > 0 || s->prepared >= 0 || s->prepared_ahead >= 0)
        return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "a batch is submitted, prepared ahead or in flight: flush the bank (fdc_sinks_flush / fdc_pipeline_flush_sinks) first");
    if (format != FDC_OQ_FC32 && !s->dev.on)
        return fdc::set_error(FDC_ERR_UNSUPPORTED, "sc16 / sc8 payloads need the device engine: this bank decides on the host (FDC_SINKS_HOST_DECISIONS, verbose, or segments above %d cells)", fdc::kDetMaxCells);
    s->pay_fmt = format; s->pay_scale = scale;
    s->pdus.clear();
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_sinks_payload_format(const fdc_sinks *s, int32_t *format, float *scale)
{
    FDC_ENTRY("fdc_sinks_payload_format")
    if (!s || !format || !scale) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    *format = s->pay_fmt; *scale = s->pay_scale;
    return FDC_OK;
    FDC_ENTRY_END
}

int32_t fdc_sinks_payload_route(const fdc_sinks *s) { return s ? s->pay_route : -1; }

int fdc_sinks_work_device(fdc_sinks *s, int nblocks)
{
    FDC_ENTRY("fdc_sinks_work_device")
    { const int rc0 = batch_entry_check(s, "nblocks", nblocks, kNotInFlight); if (rc0 != FDC_OK) return rc0; }
    if (nblocks == 0) { s->pdus.clear(); return 0; }
    HIPCHK(hipSetDevice(s->cfg.device_id));
    if (!s->dev.on) return poison(s, host_work_device(s, nblocks));
    int rc = fdc_sinks_submit_device(s, nblocks);
    if (rc < 0) return rc;
    rc = poison(s, dev_complete(s, s->dev.cur));
    return rc < 0 ? rc : nblocks;
    FDC_ENTRY_END
}

int fdc_sinks_work(fdc_sinks *s, const void *spectrum, int nitems)
{
    FDC_ENTRY("fdc_sinks_work")
    { const int rc0 = batch_entry_check(s, "nitems", nitems, kNotInFlight | kNotEager); if (rc0 != FDC_OK) return rc0; }
    if (nitems == 0) { s->pdus.clear(); return 0; }
    if (!spectrum) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null buffer");
    HIPCHK(hipSetDevice(s->cfg.device_id));
    s->prepared = -1;                                          // the buffer is overwritten: power cells an earlier fdc_sinks_prepare left for it are stale
    HIPCHK(hipMemcpyAsync(s->d_spec + s->N, spectrum, sizeof(float2) * (size_t)nitems * s->N, hipMemcpyHostToDevice, s->stream));
    return fdc_sinks_work_device(s, nitems);
    FDC_ENTRY_END
}

int fdc_sinks_read_band(const fdc_sinks *s, int32_t *lo, int32_t *hi)
{
    FDC_ENTRY("fdc_sinks_read_band")
    if (!s || !lo || !hi) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null argument");
    int a = s->N, b = 0;
    for (const Pac &p : s->pacs) {
        a = std::min(a, std::min(p.extract_start, p.measure_start));
        b = std::max(b, std::max(std::max(p.extract_stop, p.extract_start + p.extract_width), p.measure_stop));
    }
    for (const Segment &g : s->segs) {
        // a detected channel is at most the segment wide; its extraction is the next power of two above width * (1 + 2 puffer),
        // centred on the channel and clamped to the block (seg_detect): it can reach half that width beyond either end
        const int ew = pow2ceil((int)std::ceil((double)g.width * (1.0 + 2.0 * s->cfg.window_flank_puffer)));
        a = std::min(a, g.start - ew);
        b = std::max(b, g.stop + ew);
    }
    if (b <= a) { a = 0; b = 0; }
    *lo = std::max(0, a); *hi = std::min(s->N, b);
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_sinks_work_band(fdc_sinks *s, const void *spectrum, int nitems, int32_t bin_lo, int32_t bin_hi)
{
    FDC_ENTRY("fdc_sinks_work_band")
    { const int rc0 = batch_entry_check(s, "nitems", nitems, kNotInFlight | kNotEager); if (rc0 != FDC_OK) return rc0; }
    if (bin_lo < 0 || bin_hi > s->N || bin_lo > bin_hi) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "band [%d, %d) outside the block", bin_lo, bin_hi);
    int32_t need_lo = 0, need_hi = 0;
    fdc_sinks_read_band(s, &need_lo, &need_hi);
    if (need_hi > need_lo && (bin_lo > need_lo || bin_hi < need_hi))
        return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "band [%d, %d) does not cover what the bank reads, [%d, %d)", bin_lo, bin_hi, need_lo, need_hi);
    if (nitems == 0) { s->pdus.clear(); return 0; }
    if (!spectrum) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null buffer");
    HIPCHK(hipSetDevice(s->cfg.device_id));
    s->prepared = -1;                                          // as in fdc_sinks_work
    if (bin_hi > bin_lo) {
        const size_t pitch = sizeof(float2) * (size_t)s->N;
        HIPCHK(hipMemcpy2DAsync(s->d_spec + s->N + bin_lo, pitch, static_cast<const float2 *>(spectrum) + bin_lo, pitch,
                                sizeof(float2) * (size_t)(bin_hi - bin_lo), (size_t)nitems, hipMemcpyHostToDevice, s->stream));
    }
    return fdc_sinks_work_device(s, nitems);
    FDC_ENTRY_END
}

int fdc_sinks_pdu_emit_items(const fdc_sinks *s, int32_t *item, int cap)
{
    if (!s) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    const int n = (int)s->pdus.size();
    const int sh = item_shift(s);                              // the order key of a PDU starts with the index of the item that emitted it
    for (int i = 0; i < n && i < cap; i++) item[i] = (int32_t)(s->pdus[(size_t)i].key >> sh);
    return n;
}

int fdc_sinks_pdu_emit_order(const fdc_sinks *s, int32_t *item, int32_t *pac, int cap)
{
    FDC_ENTRY("fdc_sinks_pdu_emit_order")
    if (!s) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    const int n = (int)s->pdus.size();
    // the order key: item index in the high bits (above), and for a PowerActivationChannel its index in this bank's list below the detection bit
    const int sh = item_shift(s);
    for (int i = 0; i < n && i < cap; i++) {
        const PduRec &r = s->pdus[(size_t)i];
        if (item) item[i] = (int32_t)(r.key >> sh);
        if (pac) pac[i] = r.meta.kind == 0 ? (int32_t)(r.key & (fdc::key_det_bit(sh) - 1)) : -1;
    }
    return n;
    FDC_ENTRY_END
}

void fdc_set_log_callback(fdc_log_fn fn, void *user) { std::lock_guard<std::mutex> g(g_log_mu); g_log_fn = fn; g_log_user = user; }

int fdc_sinks_pdu_count(const fdc_sinks *s) { return s ? (int)s->pdus.size() : 0; }

int fdc_sinks_pdu(const fdc_sinks *s, int i, fdc_pdu *out)
{
    FDC_ENTRY("fdc_sinks_pdu")
    if (!s || !out || i < 0 || i >= (int)s->pdus.size()) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "bad PDU index");
    *out = s->pdus[(size_t)i].meta;
    return FDC_OK;
    FDC_ENTRY_END
}

int fdc_sinks_pdus(const fdc_sinks *s, fdc_pdu *out, int cap)
{
    FDC_ENTRY("fdc_sinks_pdus")
    if (!s || (cap > 0 && !out)) return fdc::set_error(FDC_ERR_INVALID_ARGUMENT, "bad PDU array");
    const int n = (int)s->pdus.size();
    for (int i = 0; i < n && i < cap; i++) out[i] = s->pdus[(size_t)i].meta;
    return n;
    FDC_ENTRY_END
}

}  // extern "C"
