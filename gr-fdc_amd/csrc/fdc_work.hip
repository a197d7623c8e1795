// The host entries of the pipeline handle: work, work_real, work_iq and their span forms, work_waterfall, work_sinks (serial and pipelined),
// flush_sinks, work_spectrum — host buffers in, host buffers out, through the handle's rings and staging and the enqueue path (fdc_enqueue.hip).
#include "fdc_pipeline.hpp"

#include <condition_variable>
#include <thread>

using namespace fdc::pipe;

extern "C" {

// the entries that write complex float only (sinks, spectrum items, group powers, waterfall): refused while the output format is not FC32
// (and, but for the flush of a batch that is inside already, while fine tuning is on: they write the channels as they are cut; and while channel
// levels or the lag-1 correlation are on: they give none; and while channel gains are on: they write the channels as they are cut; and while the
// channel demodulation is on: their channel outputs are complex float)
static int check_float_output(const fdc_pipeline *p, const char *entry, bool writes_channels = true)
{
    if (p && p->out_form) return set_error(FDC_ERR_INVALID_ARGUMENT, "%s writes complex float outputs only: set the output format to FDC_OQ_FC32 first", entry);
    if (p && p->fine_on && writes_channels) return set_error(FDC_ERR_INVALID_ARGUMENT, "%s writes the channels as they are cut: switch fine tuning off first (fdc_pipeline_set_fine_tuning(p, NULL, C))", entry);
    if (p && p->levels_on && writes_channels) return set_error(FDC_ERR_INVALID_ARGUMENT, "%s gives no channel levels: switch them off first (fdc_pipeline_set_levels(p, 0))", entry);
    if (p && p->lag1_on && writes_channels) return set_error(FDC_ERR_INVALID_ARGUMENT, "%s gives no channel lag-1 correlation: switch it off first (fdc_pipeline_set_lag1(p, 0))", entry);
    if (p && p->gains_on && writes_channels) return set_error(FDC_ERR_INVALID_ARGUMENT, "%s writes the channels as they are cut: switch the channel gains off first (fdc_pipeline_set_gains(p, NULL, C))", entry);
    if (p && p->demod_mode && writes_channels) return set_error(FDC_ERR_INVALID_ARGUMENT, "%s writes complex float outputs only: switch the channel demodulation off first (fdc_pipeline_set_demod(p, FDC_DEMOD_OFF, 1))", entry);
    return FDC_OK;
}

// Channel levels of a host entry's call: one copy of its nblocks*C (power, peak) pairs to the pinned twin, enqueued in front of the call's synchronise,
// so that fdc_pipeline_levels is a memcpy; and the same of its lag-1 correlation (fdc_pipeline_lag1)
static int levels_home(fdc_pipeline *p, int nblocks, hipStream_t s, int tones_frames = 0)
{
    // the frame rows the call's tones pass completed (fdc_pipeline_tones), by the same rule: no copy where it completed none
    if (tones_on(p) && tones_frames > 0)
        HIPCHK(hipMemcpyAsync(p->pin_tones.get(), p->d_tones.get(), sizeof(float2) * (size_t)tones_frames * tones_row(p), hipMemcpyDeviceToHost, s));
    // ... and the tone squelch's decisions of those frames (fdc_pipeline_tone_squelch), likewise
    if (tone_dec_rows(p, 0) && tones_frames > 0)
        HIPCHK(hipMemcpyAsync(p->pin_tdec.get(), p->d_tdec.get(), (size_t)tones_frames * (size_t)p->C, hipMemcpyDeviceToHost, s));
    if (p->levels_on && p->C > 0)
        HIPCHK(hipMemcpyAsync(p->pin_levels.get(), p->d_levels.get(), sizeof(float2) * (size_t)nblocks * p->C, hipMemcpyDeviceToHost, s));
    if (p->lag1_on && p->C > 0)
        HIPCHK(hipMemcpyAsync(p->pin_lag1.get(), p->d_lag1.get(), sizeof(float2) * (size_t)nblocks * p->C, hipMemcpyDeviceToHost, s));
    // ... and of its squelch mask (fdc_pipeline_squelch)
    if (squelch_rows(p, 0))
        HIPCHK(hipMemcpyAsync(p->pin_mask.get(), p->d_mask.get(), (size_t)nblocks * p->C, hipMemcpyDeviceToHost, s));
    // ... and of its audio rows, which are all the call hands to the host while the channel audio is on (fdc_pipeline_audio); packed audio: only the
    // 8 bytes of its total, the elements follow once the host knows how many they are (packed_home)
    if (packing_on(p))
        HIPCHK(hipMemcpyAsync(p->pin_packtotal.get(), p->d_packtotal.get(), sizeof(long long), hipMemcpyDeviceToHost, s));
    else if (audio_on(p))
        HIPCHK(hipMemcpyAsync(p->pin_audio.get(), p->d_audio.get(), audio_bytes(p) * (size_t)nblocks * (size_t)p->audio_row, hipMemcpyDeviceToHost, s));
    return FDC_OK;
}

// Packed audio of a host entry's call, behind the call's synchronise (the total is home): exactly `count` elements to the pinned twin and one more
// synchronise, neither where no cell was open
static int packed_home(fdc_pipeline *p, hipStream_t s)
{
    if (!packing_on(p)) return FDC_OK;
    p->pack_count = (int64_t)p->pin_packtotal[0];
    if (p->pack_count <= 0) return FDC_OK;
    HIPCHK(hipMemcpyAsync(p->pin_audio.get(), p->d_audio.get(), audio_bytes(p) * (size_t)p->pack_count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return FDC_OK;
}

// The whole-call spectrum of a work() that hands it to the host (debug port, python/FrequencyDomainChannelizer.py:152-158, :314-315) when
// no bank's buffer takes it: allocated at the first such call, kept (no allocation in the steady state of any entry).
static int spec_staging(fdc_pipeline *p, float2 **out)
{
    if (!p->d_specfull) HIPCHK(p->d_specfull.alloc((size_t)p->cfg.max_blocks * p->N));
    *out = p->d_specfull;
    return FDC_OK;
}

static int work_io_setup(fdc_pipeline *p)
{
    if (p->d_ring) return FDC_OK;
    HIPCHK(p->d_ring.alloc((size_t)p->ovl + (size_t)p->cfg.max_blocks * p->H));
    HIPCHK(hipMemsetAsync(p->d_ring, 0, sizeof(float2) * (size_t)p->ovl, p->stream));   // zero history (overlap_save_impl.cc:52)
    RCCHK(out_staging(p));                                                               // (integer-output device calls may have made it)
    HIPCHK(hipStreamCreateWithFlags(&p->s_in, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&p->s_out, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipEventCreateWithFlags(&p->ev_in[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&p->ev_k[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&p->ev_out[i], hipEventDisableTiming));
    }
    // sub-batch: about 8 MiB of input (measured best of 2-16 MiB on MI355X/PCIe5, staged and pinned): long against a
    // transfer's launch cost, short against the call
    int64_t sub = (8ll << 20) / ((int64_t)p->H * 8);
    if (p->cfg.host_sub_blocks > 0) sub = p->cfg.host_sub_blocks;
    if (const char *e = fdc::debug_env("FDC_HOST_SUB")) if (atoi(e) > 0) sub = atoi(e);
    p->sub = (int)std::max<int64_t>(1, std::min<int64_t>(sub, p->cfg.max_blocks));
    if (p->C > 0) {
        // scatter table: pinned and device-mapped, the scatter kernel reads it in place (no per-call upload)
        HIPCHK(p->pin_tab.alloc((size_t)p->C));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&p->d_tab), p->pin_tab.get(), 0));
    }
    return FDC_OK;
}

// The input form of a work call against the form the handle is latched to (the first work call after create / reset latches it): a call in another
// form is refused before it touches anything.  fmt 0 = float input (scale unused).  check_form only compares; begin_work records the form of a
// call that got past its set-up (a first call that fails there leaves the handle unlatched).
static int check_form(const fdc_pipeline *p, int fmt, float scale)
{
    if (p->in_form < 0) return FDC_OK;
    if (p->in_form == fmt && (fmt == 0 || std::memcmp(&p->in_scale, &scale, sizeof(float)) == 0)) return FDC_OK;
    auto name = [](int f, float sc) {
        char b[48];
        if (f == 0) std::snprintf(b, sizeof(b), "float");
        else std::snprintf(b, sizeof(b), "%s x %.9g", f == FDC_IQ_SC16 ? "sc16" : "sc8", (double)sc);
        return std::string(b);
    };
    return set_error(FDC_ERR_INVALID_ARGUMENT, "the handle takes %s input since its first work call (reset it to change the input form), not %s",
                name(p->in_form, p->in_scale).c_str(), name(fmt, scale).c_str());
}

// The host entries' argument checks.  A call of no blocks passes whatever its buffers are: the entry returns 0 before it looks at them.
static int check_work_args(const fdc_pipeline *p, const void *in, int nblocks, void *const *outs)
{
    if (nblocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative item count");
    if (nblocks == 0) return FDC_OK;
    if (nblocks > p->cfg.max_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d above max_blocks %d", nblocks, p->cfg.max_blocks);
    if (!in || (p->C > 0 && !outs && !audio_on(p))) return set_error(FDC_ERR_INVALID_ARGUMENT, "null host buffer");   // (audio on: outs is not looked at)
    return FDC_OK;
}

// What a stream entry does first: the input form against the latch, the device, the buffers of the first call (that needs them); then the form is latched
static int begin_work(fdc_pipeline *p, int fmt, float scale)
{
    RCCHK(check_form(p, fmt, scale));
    HIPCHK(hipSetDevice(p->cfg.device_id));
    RCCHK(work_io_setup(p));
    if (out_code(p) && !p->d_oq && p->sum_lout > 0) HIPCHK(p->d_oq.alloc(fdc::kIqRingBytes * (size_t)p->cfg.max_blocks * p->sum_lout));
    if (fmt && !p->d_iq) {
        // the integer ring, for the WIDEST format (a reset may latch the handle to another one); its history starts at zero, as the float ring's
        HIPCHK(p->d_iq.alloc(fdc::kIqRingBytes * ((size_t)p->ovl + (size_t)p->cfg.max_blocks * p->H)));
        HIPCHK(hipMemsetAsync(p->d_iq, 0, fdc::kIqRingBytes * (size_t)p->ovl, p->stream));
    }
    if (p->in_form < 0) { p->in_form = fmt; p->in_scale = fmt ? scale : 0.f; }
    return FDC_OK;
}

// The scatter table of a call whose outputs (osz bytes per sample) are ALL registered host buffers (else false): the scatter kernels store in place
static bool fill_scatter_table(fdc_pipeline *p, void *const *outs, int nblocks, size_t osz)
{
    bool out_reg = p->C > 0;
    for (int c = 0; c < p->C && out_reg; c++) {
        fdc::ScatterEnt &e = p->pin_tab[c];
        e.dst = nullptr; e.out_off = p->chans[c].out_off; e.lout = p->chans[c].lout; e.pad = 0;
        if (outs[c] && !host_registered(outs[c], osz * (size_t)nblocks * p->chans[c].lout, reinterpret_cast<void **>(&e.dst)))
            out_reg = false;
    }
    return out_reg;
}

// The results of a whole call (src: on the device, [channel][nblocks*lout] samples of osz bytes) to the buffers the caller gave, one copy per channel
static int copy_outputs(const fdc_pipeline *p, void *const *outs, int nblocks, size_t osz, const void *src, hipStream_t s)
{
    for (int c = 0; c < p->C; c++)
        if (outs[c])
            HIPCHK(hipMemcpyAsync(outs[c], static_cast<const unsigned char *>(src) + osz * (size_t)nblocks * p->chans[c].out_off,
                                  osz * (size_t)nblocks * p->chans[c].lout, hipMemcpyDeviceToHost, s));
    return FDC_OK;
}

// span: the call is one contiguous span of a longer stream handed over by a dispatcher (fdc_pipeline_work_span and friends): the history comes from
// `halo` (N/R samples, NULL = zeros) and the block counter from `first_block` instead of from the handle
struct SpanStart { bool span; const void *halo; int64_t first_block; };

// Host entry.  The call is cut into sub-batches; sub-batch k's H2D copy (stream s_in), its kernels (p->stream) and
// its D2H leg (s_out) run beside the neighbouring sub-batches' other legs, so a long call moves at the rate of the
// slower PCIe direction instead of the sum of all legs.  Caller buffers pinned with fdc_host_register() are DMA'd in
// place (input: one async copy; outputs: one scatter kernel storing straight into the caller's per-channel buffers).
// Pageable input is copied by the runtime's pin-on-the-fly path from a feeder thread; pageable outputs come back
// through two pinned staging slots and a CPU copy on this thread.
// call: the entry's (device_call; its spectrum: a device destination of the entry's own, the sinks' buffer or the waterfall's staging).
// call.fmt != 0: `in` and the halo hold complex integers (FDC_IQ_SC16 / FDC_IQ_SC8, times scale): the ring and its history are kept in that format
// (d_iq), the integer kernels read it where the plan has them, the handle's float ring takes the widened launch groups otherwise.
// Integer output (p->out_form): the kernels narrow into d_oq where the plan lets them (oq_fused), else they write d_out and k_complex_to_iq narrows it
// into d_oq; registered outputs are scattered from either (k_scatter_oq: narrowing from d_out, copying from d_oq), staged ones copied from d_oq.
// Channel demodulation (p->demod_mode; it excludes integer output) goes the same way with its 4-byte real samples: the kernels write d_out, k_chan_demod
// writes d_oq behind every sub-batch, registered outputs are scattered from d_oq by the copy form (a real float32 is the size of an sc16 sample).
static int pipeline_work_impl(fdc_pipeline *p, DeviceCall call, const void *in, int nblocks, void *const *outs, void *spectrum, SpanStart from = {})
{
    int rc = check_work_args(p, in, nblocks, outs);
    if (rc != FDC_OK || nblocks == 0) return rc;
    if ((spectrum || (call.spectrum && !call.own_spectrum)) && !p->cfg.keep_spectrum) return set_error(FDC_ERR_INVALID_ARGUMENT, "spectrum output needs keep_spectrum");
    const int fmt = call.fmt;
    RCCHK(begin_work(p, fmt, call.scale));
    hipStream_t s = p->stream;
    const size_t nin = (size_t)nblocks * p->H, esz = fdc::iq_bytes(fmt);
    const int ofmt = out_code(p);
    const bool demod = oq_demod(ofmt);
    const float oscale = demod ? p->demod_gain : p->out_scale;
    const size_t osz = ofmt ? oq_bytes(ofmt) : sizeof(float2);            // bytes per output sample the caller receives
    // the ring the call's samples go to, as bytes: float2 (d_ring) or the integer format (d_iq)
    unsigned char *const ringb = fmt ? static_cast<unsigned char *>(p->d_iq) : reinterpret_cast<unsigned char *>(p->d_ring.get());
    const unsigned char *hin = static_cast<const unsigned char *>(in);
    if (from.span) {
        // every kernel of the call is enqueued on s behind this copy; the previous call ended with s drained
        if (from.halo) HIPCHK(hipMemcpyAsync(ringb, from.halo, esz * (size_t)p->ovl, hipMemcpyHostToDevice, s));
        else HIPCHK(hipMemsetAsync(ringb, 0, esz * (size_t)p->ovl, s));
        p->blockcount = from.first_block;
    }

    // spectrum wanted (debug port / sinks): every sub-batch writes its part of one whole-call buffer
    float2 *d_specfull = static_cast<float2 *>(call.spectrum);
    if (spectrum && !d_specfull && (rc = spec_staging(p, &d_specfull)) != FDC_OK) return rc;

    // channel audio on: the call hands the host its audio rows and nothing else: outs is not looked at, no port is copied or scattered
    const bool audio = audio_on(p), ports = p->C > 0 && !audio;
    // packed audio: the sub-batches append to one packed buffer, each from the running total on, which starts the call at 0
    const bool pack = packing_on(p);
    if (pack) HIPCHK(hipMemsetAsync(p->d_packtotal.get(), 0, sizeof(long long), s));
    const bool in_reg = host_registered(in, esz * nin);
    const bool out_reg = ports && fill_scatter_table(p, outs, nblocks, osz);
    call.wide = fmt ? p->d_ring : nullptr;
    call.ofmt = ofmt; call.oscale = oscale; call.narrow = !out_reg || demod;
    bool oq_all = true;
    int tframes = 0;              // channel tones: the frame rows the call's sub-batches have completed so far; the next one's rows append behind them
    // dok: the float results of the sub-batch starting at block b0.  Integer output: its narrow results go to the same sample offset of d_oq (call.ofused: the
    // kernels wrote them there themselves; otherwise dok holds float and is narrowed into d_oq, unless the outputs are registered: k_scatter_oq narrows)
    // (channel levels: a sub-batch is a call of its own to the enqueue path, so each hands in where ITS block 0 goes)
    auto process = [&](size_t b0, int nb, int64_t first, float2 *dok, float2 *dspec) {
        call.spectrum = dspec; call.fout = dok;
        call.levels = p->levels_on && p->C > 0 ? p->d_levels + b0 * (size_t)p->C : nullptr;
        call.lag1 = p->lag1_on && p->C > 0 ? p->d_lag1 + b0 * (size_t)p->C : nullptr;
        call.audio = audio_rows(p, b0);
        call.squelch = squelch_rows(p, b0);
        if (pack) { call.audio = p->d_audio.get(); call.pack_off = pack_rows(p, b0); call.pack_append = true; }
        call.tones = tones_rows(p, (size_t)tframes);
        call.tone_dec = tone_dec_rows(p, (size_t)tframes);
        const int rc2 = process_device_impl(p, call, ringb + b0 * p->H * esz, first, nb,
                                            ofmt ? static_cast<void *>(p->d_oq + osz * b0 * (size_t)p->sum_lout) : static_cast<void *>(dok));
        oq_all = oq_all && call.ofused;
        if (rc2 == FDC_OK) tframes += call.tones_frames;
        return rc2;
    };
    // what the caller's buffers receive for the sub-batch at b0: float from d_out, or narrow from d_oq
    auto res = [&](size_t b0) -> const void * {
        return ofmt ? static_cast<const void *>(p->d_oq + osz * b0 * (size_t)p->sum_lout) : static_cast<const void *>(p->d_out + b0 * (size_t)p->sum_lout);
    };
    auto scatter = [&](size_t b0, int nb, hipStream_t st) -> hipError_t {
        if (!ofmt) return fdc::launch_scatter_out(p->d_out + b0 * (size_t)p->sum_lout, p->d_tab, p->C, nb, (long long)b0, st);
        if (demod) return fdc::launch_scatter_oq(fdc::kIqSc16, res(b0), fdc::kIqSc16, 1.0f, p->d_tab, p->C, nb, (long long)b0, st);   // 4-byte elements, copied
        return call.ofused ? fdc::launch_scatter_oq(ofmt, res(b0), ofmt, oscale, p->d_tab, p->C, nb, (long long)b0, st)
                      : fdc::launch_scatter_oq(fdc::kIqFloat, p->d_out + b0 * (size_t)p->sum_lout, ofmt, oscale, p->d_tab, p->C, nb, (long long)b0, st);
    };
    const int sub = p->sub;
    if (!out_reg && ports && !p->pin_out[0])
        for (int i = 0; i < 2; i++)
            HIPCHK(p->pin_out[i].alloc((size_t)sub * p->sum_lout));
    // staged outputs: the pieces of the sub-batch (b0, nb) that has arrived in pin_out[slot] go to the caller's per-channel buffers
    auto deliver = [&](int slot, int b0, int nb) {
        const unsigned char *src = reinterpret_cast<const unsigned char *>(p->pin_out[slot].get());
        for (int c = 0; c < p->C; c++) {
            if (!outs[c]) continue;
            const size_t lo = (size_t)p->chans[c].lout;
            std::memcpy(static_cast<unsigned char *>(outs[c]) + osz * (size_t)b0 * lo, src + osz * (size_t)nb * p->chans[c].out_off, osz * nb * lo);
        }
    };
    auto drain = [&](int j) -> int {                                      // ... behind sub-batch j's D2H
        HIPCHK(hipEventSynchronize(p->ev_out[j & 1]));
        deliver(j & 1, j * sub, std::min(sub, nblocks - j * sub));
        return FDC_OK;
    };
    const int K = (nblocks + sub - 1) / sub;
    if (K == 1) {
        // short call (the usual work() of a running flowgraph): nothing to overlap, one stream, one synchronisation
        HIPCHK(hipMemcpyAsync(ringb + esz * p->ovl, hin, esz * nin, hipMemcpyHostToDevice, s));
        rc = process(0, nblocks, p->blockcount, p->d_out, d_specfull);
        if (rc != FDC_OK) return rc;
        if (ports) {
            if (out_reg) HIPCHK(scatter(0, nblocks, s));
            else HIPCHK(hipMemcpyAsync(p->pin_out[0], res(0), osz * (size_t)nblocks * p->sum_lout, hipMemcpyDeviceToHost, s));
        }
        if (spectrum) HIPCHK(hipMemcpyAsync(spectrum, d_specfull, sizeof(float2) * (size_t)nblocks * p->N, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(ringb, ringb + esz * nin, esz * (size_t)p->ovl, hipMemcpyDeviceToDevice, s));
        RCCHK(levels_home(p, nblocks, s, tframes));
        HIPCHK(hipStreamSynchronize(s));
        RCCHK(packed_home(p, s));
        if (p->levels_on) levels_written(p, nblocks, s, true);
    if (p->lag1_on) lag1_written(p, nblocks, s, true);
        if (audio) audio_written(p, p->blockcount, nblocks, s, true);
        if (squelch_rows(p, 0)) squelch_written(p, nblocks, s, true);
        if (tones_on(p)) tones_written(p, nblocks, tframes, s, true);
        if (tone_dec_rows(p, 0)) tone_squelch_written(p, nblocks, tframes, s, true);
        if (fmt) p->iq_route = route(fmt, call.all_fused, "widened");
        if (p->out_form) p->oq_route = route(ofmt, oq_all, "narrowed");
        if (ports && !out_reg) deliver(0, 0, nblocks);
        p->blockcount += nblocks;
        return nblocks;
    }
    // Pageable input: the runtime pins the pages of each copy on the fly and DMAs from them (measured faster than a CPU
    // copy into pinned staging), but such a copy holds its calling thread until it is done — so a feeder thread issues
    // them, and this thread spends that time launching kernels and draining finished outputs.
    struct Feeder {
        std::thread th; std::mutex mu; std::condition_variable cv; int done = 0; hipError_t err = hipSuccess;
        ~Feeder() { if (th.joinable()) th.join(); }
    } feeder;
    if (!in_reg) {
        const int dev = p->cfg.device_id, Hs = p->H;
        unsigned char *ring_in = ringb + esz * p->ovl;
        hipStream_t sin = p->s_in;
        feeder.th = std::thread([&feeder, dev, Hs, ring_in, sin, hin, K, sub, nblocks, esz] {
            hipError_t e = hipSetDevice(dev);
            for (int k = 0; k < K; k++) {
                const int b0 = k * sub, nb = std::min(sub, nblocks - b0);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(ring_in + (size_t)b0 * Hs * esz, hin + (size_t)b0 * Hs * esz, esz * (size_t)nb * Hs,
                                       hipMemcpyHostToDevice, sin);
                if (e == hipSuccess) e = hipStreamSynchronize(sin);
                std::lock_guard<std::mutex> lk(feeder.mu);
                feeder.done = k + 1; feeder.err = e;
                feeder.cv.notify_one();
            }
        });
    }
    for (int k = 0; k < K; k++) {
        const int slot = k & 1, b0 = k * sub, nb = std::min(sub, nblocks - b0);
        if (in_reg) {
            HIPCHK(hipMemcpyAsync(ringb + esz * (p->ovl + (size_t)b0 * p->H), hin + esz * (size_t)b0 * p->H,
                                  esz * (size_t)nb * p->H, hipMemcpyHostToDevice, p->s_in));
            HIPCHK(hipEventRecord(p->ev_in[slot], p->s_in));
            HIPCHK(hipStreamWaitEvent(s, p->ev_in[slot], 0));
        } else {
            std::unique_lock<std::mutex> lk(feeder.mu);
            feeder.cv.wait(lk, [&] { return feeder.done > k; });               // sub-batch k is on the device
            if (feeder.err != hipSuccess) return set_error(FDC_ERR_HIP, "input copy failed: %s", hipGetErrorString(feeder.err));
        }
        float2 *dok = p->d_out + (size_t)b0 * p->sum_lout;                    // [channel][nb*lout] of this sub-batch
        rc = process((size_t)b0, nb, p->blockcount + b0, dok, d_specfull ? d_specfull + (size_t)b0 * p->N : nullptr);
        if (rc != FDC_OK) return rc;
        if (!ports) continue;
        HIPCHK(hipEventRecord(p->ev_k[slot], s));
        HIPCHK(hipStreamWaitEvent(p->s_out, p->ev_k[slot], 0));
        if (out_reg) {
            HIPCHK(scatter((size_t)b0, nb, p->s_out));
        } else {
            HIPCHK(hipMemcpyAsync(p->pin_out[slot], res((size_t)b0), osz * (size_t)nb * p->sum_lout, hipMemcpyDeviceToHost, p->s_out));
            HIPCHK(hipEventRecord(p->ev_out[slot], p->s_out));
            if (k >= 1 && (rc = drain(k - 1)) != FDC_OK) return rc;
        }
    }
    if (!out_reg && ports && (rc = drain(K - 1)) != FDC_OK) return rc;
    if (spectrum) HIPCHK(hipMemcpyAsync(spectrum, d_specfull, sizeof(float2) * (size_t)nblocks * p->N, hipMemcpyDeviceToHost, s));
    // history <- last ovl samples of this call (overlap_save_impl.cc:78); src and dst never overlap (H >= ovl)
    HIPCHK(hipMemcpyAsync(ringb, ringb + esz * nin, esz * (size_t)p->ovl, hipMemcpyDeviceToDevice, s));
    RCCHK(levels_home(p, nblocks, s, tframes));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipStreamSynchronize(p->s_out));
    RCCHK(packed_home(p, s));
    if (p->levels_on) levels_written(p, nblocks, s, true);
    if (p->lag1_on) lag1_written(p, nblocks, s, true);
    if (audio) audio_written(p, p->blockcount, nblocks, s, true);
    if (squelch_rows(p, 0)) squelch_written(p, nblocks, s, true);
    if (tones_on(p)) tones_written(p, nblocks, tframes, s, true);
    if (tone_dec_rows(p, 0)) tone_squelch_written(p, nblocks, tframes, s, true);
    if (fmt) p->iq_route = route(fmt, call.all_fused, "widened");
    if (p->out_form) p->oq_route = route(ofmt, oq_all, "narrowed");
    p->blockcount += nblocks;
    return nblocks;
}

int fdc_pipeline_work(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum)
{
    FDC_ENTRY("fdc_pipeline_work")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    return pipeline_work_impl(p, device_call(p, nullptr, nullptr), in, nblocks, outs, spectrum);
    FDC_ENTRY_END
}

// The hier block with the waterfall on its spectrum (include/fdc_amd.h).  Path 5: the one-launch kernel's ROWS form sums the pixels from the spectrum in
// LDS, no spectrum reaches memory.  Other paths: the call writes the handle's whole-call spectrum (the spectrum path of every plan, as a debug-port call)
// and the rows are summed from its 16-bin group powers (N a multiple of 16384: the block kernel's epilogue or a pass over the spectrum) or from its bins.
int fdc_pipeline_work_waterfall(fdc_pipeline *p, fdc_waterfall *w, const void *in, int nblocks, void *const *outs, float *rows, uint16_t *index,
                                uint8_t *rgb, int cap_rows, int32_t *nrows)
{
    FDC_ENTRY("fdc_pipeline_work_waterfall")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (int rcf = check_float_output(p, "fdc_pipeline_work_waterfall")) return rcf;
    if (nblocks < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative item count");
    if (nblocks > p->cfg.max_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d above max_blocks %d", nblocks, p->cfg.max_blocks);
    int rc = fdc::wf_check_call(w, p->cfg.device_id, p->N, nblocks, cap_rows);
    if (rc != FDC_OK) return rc;
    if (nblocks == 0) { if (nrows) *nrows = 0; return 0; }
    HIPCHK(hipSetDevice(p->cfg.device_id));
    const bool fused = p->fused, groups = !fused && p->N % (16 * fdc::kWfWidth) == 0;
    float2 *spec = nullptr;
    float *gpow = nullptr;
    if (!fused && (rc = spec_staging(p, &spec)) != FDC_OK) return rc;
    if (groups && (rc = fdc::wf_group_buffer(w, nblocks, &gpow)) != FDC_OK) return rc;
    DeviceCall call = device_call(p, nullptr, spec);
    call.own_spectrum = true;                                   // the staging the rows are summed from: no keep_spectrum needed
    call.rows = fused ? fdc::wf_block_rows(w) : nullptr;
    call.rows_first = p->blockcount;
    call.gpow = gpow; call.gpow_origin = gpow ? spec : nullptr;
    p->gpow_src = 0;
    rc = pipeline_work_impl(p, call, in, nblocks, outs, nullptr);
    if (rc < 0) return rc;
    p->wf_route = fused ? "k_f4096 epilogue (pixels from the spectrum in LDS)"
                : groups ? "k_wf_from_groups (pixels from the 16-bin group powers of the internal spectrum)"
                         : "k_wf_from_spectrum (pixels from the bins of the internal spectrum)";
    // which transform of the call's launch groups summed the group powers (a call may mix them: a short last launch group takes the two-pass transform)
    if (groups)
        p->wf_route += p->gpow_src == 1 ? ", group powers: block kernel epilogue"
                     : p->gpow_src == 2 ? ", group powers: k_group_power behind the two-pass transform"
                                        : ", group powers: block kernel epilogue and k_group_power";
    if (groups) HIPCHK(fdc::wf_rows_from_groups(w, gpow, nblocks, p->stream));
    else if (!fused) HIPCHK(fdc::wf_rows_from_spectrum(w, spec, nblocks, p->stream));
    rc = fdc::wf_finish(w, nblocks, p->stream, rows, index, rgb, nrows);
    return rc < 0 ? rc : nblocks;
    FDC_ENTRY_END
}

int fdc_pipeline_work_span(fdc_pipeline *p, const void *halo, const void *in, int64_t first_block, int nblocks, void *const *outs,
                           void *spectrum)
{
    FDC_ENTRY("fdc_pipeline_work_span")
    if (first_block < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block index");
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    return pipeline_work_impl(p, device_call(p, nullptr, nullptr), in, nblocks, outs, spectrum, {true, halo, first_block});
    FDC_ENTRY_END
}

// Real input: the float items are copied to the device and widened there into the complex ring (imaginary part 0); the
// rest of the call is the one-stream form of the complex entry.
static int pipeline_work_real_impl(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum, SpanStart from = {})
{
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    int rc = check_work_args(p, in, nblocks, outs);
    if (rc != FDC_OK || nblocks == 0) return rc;
    if (spectrum && !p->cfg.keep_spectrum) return set_error(FDC_ERR_INVALID_ARGUMENT, "spectrum output needs keep_spectrum");
    RCCHK(begin_work(p, 0, 0.f));
    hipStream_t s = p->stream;
    const size_t nin = (size_t)nblocks * p->H;
    // d_real: [N/R history samples of a span call][max_blocks*H new samples]
    if (!p->d_real) HIPCHK(p->d_real.alloc((size_t)p->ovl + (size_t)p->cfg.max_blocks * p->H));
    float2 *d_specfull = nullptr;
    if (spectrum && (rc = spec_staging(p, &d_specfull)) != FDC_OK) return rc;
    HIPCHK(hipMemcpyAsync(p->d_real + p->ovl, in, sizeof(float) * nin, hipMemcpyHostToDevice, s));
    if (from.span) {
        if (from.halo) HIPCHK(hipMemcpyAsync(p->d_real, from.halo, sizeof(float) * (size_t)p->ovl, hipMemcpyHostToDevice, s));
        else HIPCHK(hipMemsetAsync(p->d_real, 0, sizeof(float) * (size_t)p->ovl, s));
        HIPCHK(fdc::launch_real_to_complex(p->d_real, p->d_ring, (size_t)p->ovl + nin, s));
        p->blockcount = from.first_block;
    } else {
        HIPCHK(fdc::launch_real_to_complex(p->d_real + p->ovl, p->d_ring + p->ovl, nin, s));
    }
    // integer output (p->out_form): the narrow results in d_oq (the kernels' own stores, or k_complex_to_iq behind them), copied as they are;
    // channel demodulation (p->demod_mode): the real results in d_oq likewise
    const int ofmt = out_code(p);
    const size_t osz = ofmt ? oq_bytes(ofmt) : sizeof(float2);
    void *const res = ofmt ? static_cast<void *>(p->d_oq) : static_cast<void *>(p->d_out);
    DeviceCall call = device_call(p, nullptr, d_specfull);
    call.ofmt = ofmt; call.oscale = oq_demod(ofmt) ? p->demod_gain : p->out_scale; call.fout = p->d_out;
    call.levels = p->levels_on && p->C > 0 ? p->d_levels.get() : nullptr;
    call.lag1 = p->lag1_on && p->C > 0 ? p->d_lag1.get() : nullptr;
    call.audio = audio_rows(p, 0);
    call.squelch = squelch_rows(p, 0);
    if (packing_on(p)) { call.audio = p->d_audio.get(); call.pack_off = pack_rows(p, 0); call.pack_append = false; }
    call.tones = tones_rows(p, 0);
    call.tone_dec = tone_dec_rows(p, 0);
    RCCHK(process_device_impl(p, call, p->d_ring, p->blockcount, nblocks, res));
    if (!call.audio) RCCHK(copy_outputs(p, outs, nblocks, osz, res, s));     // (audio on: the rows go home with the levels, outs is not looked at)
    if (spectrum) HIPCHK(hipMemcpyAsync(spectrum, d_specfull, sizeof(float2) * (size_t)nblocks * p->N, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(p->d_ring, p->d_ring + nin, sizeof(float2) * (size_t)p->ovl, hipMemcpyDeviceToDevice, s));
    RCCHK(levels_home(p, nblocks, s, call.tones_frames));
    HIPCHK(hipStreamSynchronize(s));
    RCCHK(packed_home(p, s));
    if (p->levels_on) levels_written(p, nblocks, s, true);
    if (p->lag1_on) lag1_written(p, nblocks, s, true);
    if (call.audio) audio_written(p, p->blockcount, nblocks, s, true);
    if (call.squelch) squelch_written(p, nblocks, s, true);
    if (call.tones) tones_written(p, nblocks, call.tones_frames, s, true);
    if (call.tone_dec) tone_squelch_written(p, nblocks, call.tones_frames, s, true);
    if (p->out_form) p->oq_route = route(ofmt, call.ofused, "narrowed");
    p->blockcount += nblocks;
    return nblocks;
}

int fdc_pipeline_work_real(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum)
{
    FDC_ENTRY("fdc_pipeline_work_real")
    return pipeline_work_real_impl(p, in, nblocks, outs, spectrum);
    FDC_ENTRY_END
}

int fdc_pipeline_work_span_real(fdc_pipeline *p, const void *halo, const void *in, int64_t first_block, int nblocks, void *const *outs,
                                void *spectrum)
{
    FDC_ENTRY("fdc_pipeline_work_span_real")
    if (first_block < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block index");
    return pipeline_work_real_impl(p, in, nblocks, outs, spectrum, {true, halo, first_block});
    FDC_ENTRY_END
}

int fdc_pipeline_work_iq(fdc_pipeline *p, int32_t format, float scale, const void *in, int nblocks, void *const *outs, void *spectrum)
{
    FDC_ENTRY("fdc_pipeline_work_iq")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    RCCHK(check_iq_form(format, scale));
    return pipeline_work_impl(p, device_call(p, nullptr, nullptr, format, scale), in, nblocks, outs, spectrum);
    FDC_ENTRY_END
}

int fdc_pipeline_work_span_iq(fdc_pipeline *p, int32_t format, float scale, const void *halo, const void *in, int64_t first_block, int nblocks,
                              void *const *outs, void *spectrum)
{
    FDC_ENTRY("fdc_pipeline_work_span_iq")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    RCCHK(check_iq_form(format, scale));
    if (first_block < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block index");
    return pipeline_work_impl(p, device_call(p, nullptr, nullptr, format, scale), in, nblocks, outs, spectrum, {true, halo, first_block});
    FDC_ENTRY_END
}

// fdc_pipeline_work_sinks on a bank created with FDC_SINKS_LOOKAHEAD: the pipelined hier block.  What one call does:
//   - the items' copy to the device (own stream), their forward transform (+ channel kernels) into the bank's NEXT-batch buffer and its
//     power cells (fdc_sinks_prepare) — all on the bank's fill stream, behind the copy;
//   - fdc_sinks_submit_device for the batch the call BEFORE left there: its decision chains, the host's one wait for their summary, its
//     extractions — beside this call's copy and transform — and the hand-out of the batch before that one (its payload copy ran meanwhile);
//   - the wait for this call's input copy (the caller's buffer is not retained), and for the channel outputs / the debug spectrum if any.
// So the items of call n come back as PDUs from call n + 2 (device engine; n + 1 on the host engine, whose submit is synchronous), and
// fdc_pipeline_flush_sinks hands out what is still inside at stop().  Nothing here waits for the transform of the call's own items unless
// the call has stream outputs: with pinned input the call costs what its input copy costs.
static int work_sinks_pipelined(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum, fdc_sinks *sinks)
{
    int rc = check_work_args(p, in, nblocks, outs);
    if (rc != FDC_OK || nblocks == 0) return rc;
    if (!p->cfg.keep_spectrum) return set_error(FDC_ERR_INVALID_ARGUMENT, "spectrum output needs keep_spectrum");
    if (p->hier_bank && p->hier_bank != sinks && p->hier_filled > 0)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "a batch of another bank is still inside this pipeline: fdc_pipeline_flush_sinks() with that bank first");
    if (p->hier_broken) return set_error(FDC_ERR_HIP, "an earlier pipelined call failed after it had advanced the stream state: destroy the pipeline and the bank");
    RCCHK(begin_work(p, 0, 0.f));
    if (!p->ev_hier) {
        HIPCHK(hipEventCreateWithFlags(&p->ev_hier, hipEventDisableTiming));
        HIPCHK(hipStreamSynchronize(p->stream));                  // work_io_setup zeroes the history on the handle's own stream; this entry runs on others
    }
    p->hier_bank = sinks;
    hipStream_t fs = static_cast<hipStream_t>(fdc_sinks_fill_stream(sinks));
    const bool first = p->hier_filled == 0;                       // stream start, or everything was flushed: the bank's current buffer is free
    float2 *dst = static_cast<float2 *>(first ? fdc_sinks_spectrum(sinks) : fdc_sinks_spectrum_ahead(sinks));
    // the power of the spectrum's 16-bin groups comes out of the forward kernel's epilogue: the bank's cells are summed from it (no pass over the spectrum)
    float *const gpw = static_cast<float *>(first ? fdc_sinks_group_power(sinks) : fdc_sinks_group_power_ahead(sinks));
    DeviceCall call = device_call(p, fs, dst);
    call.gpow = gpw; call.gpow_origin = dst;
    // the persistent block kernels take every compute unit; the decision chains of the batch before run beside them on a few units left free
    // (long launch groups only: a group of one round is over before a chain would notice).  The user's own reservation goes first.
    if (!p->reserve_user) call.ncu = p->ncu - (std::min(nblocks, p->chunk) >= 2 * p->ncu ? p->ncu / 8 : 0);

    const size_t nin = (size_t)nblocks * p->H;
    // input: one copy on s_in.  The ring is read by the transform of the call before (fill stream) until ev_hier.
    if (p->hier_ring_busy) HIPCHK(hipStreamWaitEvent(p->s_in, p->ev_hier, 0));
    HIPCHK(hipMemcpyAsync(p->d_ring + p->ovl, in, sizeof(float2) * nin, hipMemcpyHostToDevice, p->s_in));
    HIPCHK(hipEventRecord(p->ev_in[0], p->s_in));
    HIPCHK(hipStreamWaitEvent(fs, p->ev_in[0], 0));
    RCCHK(process_device_impl(p, call, p->d_ring, p->blockcount, nblocks, p->d_out));
    // history <- last ovl samples of this call (overlap_save_impl.cc:78)
    HIPCHK(hipMemcpyAsync(p->d_ring, p->d_ring + nin, sizeof(float2) * (size_t)p->ovl, hipMemcpyDeviceToDevice, fs));
    HIPCHK(hipEventRecord(p->ev_hier, fs));
    p->hier_ring_busy = true;
    p->blockcount += nblocks;
    // from here on the call has happened as far as the stream state goes (history, block counter, the bank's buffer): a failure below cannot be
    // retried with the same items nor skipped — the pair is marked broken and every later call says so
    struct Broken { fdc_pipeline *p; bool ok = false; ~Broken() { if (!ok) p->hier_broken = true; } } guard{p};
    RCCHK(gpw ? fdc_sinks_prepare_from_groups(sinks, nblocks, first ? 0 : 1) : fdc_sinks_prepare(sinks, nblocks, first ? 0 : 1));
    if (fill_scatter_table(p, outs, nblocks, sizeof(float2))) HIPCHK(fdc::launch_scatter_out(p->d_out, p->d_tab, p->C, nblocks, 0, fs));
    else RCCHK(copy_outputs(p, outs, nblocks, sizeof(float2), p->d_out, fs));
    if (spectrum) HIPCHK(hipMemcpyAsync(spectrum, dst, sizeof(float2) * (size_t)nblocks * p->N, hipMemcpyDeviceToHost, fs));
    const int before = p->hier_filled;
    p->hier_filled = nblocks;
    const int rs = fdc_sinks_submit_device(sinks, before);         // 0: nothing to submit yet, it hands out a batch still in flight, or no PDUs
    if (rs < 0) return rs;
    HIPCHK(hipEventSynchronize(p->ev_in[0]));
    if (p->C > 0 || spectrum) HIPCHK(hipStreamSynchronize(fs));
    guard.ok = true;
    return nblocks;
}

int fdc_pipeline_work_sinks(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum,
                            fdc_sinks *sinks)
{
    FDC_ENTRY("fdc_pipeline_work_sinks")
    if (!sinks) return set_error(FDC_ERR_INVALID_ARGUMENT, "null sinks handle");
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (int rcf = check_float_output(p, "fdc_pipeline_work_sinks")) return rcf;
    if (fdc_sinks_blocklen(sinks) != p->N || nblocks > fdc_sinks_max_blocks(sinks))
        return set_error(FDC_ERR_INVALID_ARGUMENT, "sinks were created for blocklen %d / %d blocks per call, pipeline call has %d / %d",
                    fdc_sinks_blocklen(sinks), fdc_sinks_max_blocks(sinks), p->N, nblocks);
    if (fdc_sinks_fill_stream(sinks)) return work_sinks_pipelined(p, in, nblocks, outs, spectrum, sinks);
    // the spectrum goes straight into the sinks' device buffer (no PCIe round trip), then the sinks run on it; their power cells are summed from
    // the group powers the forward kernel leaves beside the spectrum
    float *const gpw = static_cast<float *>(fdc_sinks_group_power(sinks));
    DeviceCall call = device_call(p, nullptr, fdc_sinks_spectrum(sinks));
    call.gpow = gpw; call.gpow_origin = static_cast<const float2 *>(call.spectrum);
    int rc = pipeline_work_impl(p, call, in, nblocks, outs, spectrum);
    if (rc < 0) return rc;
    if (gpw && rc > 0) { const int rp = fdc_sinks_prepare_from_groups(sinks, nblocks, 0); if (rp != FDC_OK) return rp; }
    const int rs = fdc_sinks_work_device(sinks, nblocks);
    return rs < 0 ? rs : rc;
    FDC_ENTRY_END
}

int fdc_pipeline_flush_sinks(fdc_pipeline *p, fdc_sinks *sinks)
{
    FDC_ENTRY("fdc_pipeline_flush_sinks")
    if (!p || !sinks) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (int rcf = check_float_output(p, "fdc_pipeline_flush_sinks", false)) return rcf;
    if (p->hier_broken) return set_error(FDC_ERR_HIP, "an earlier pipelined call failed after it had advanced the stream state: destroy the pipeline and the bank");
    if (p->hier_bank == sinks && p->hier_filled > 0) {
        const int n = p->hier_filled;
        p->hier_filled = 0;
        const int rs = fdc_sinks_submit_device(sinks, n);
        if (rs != 0) return rs;                                    // an older batch's PDUs (or the host engine's: this batch's), or a failure
    }
    return fdc_sinks_flush(sinks);
    FDC_ENTRY_END
}

int32_t fdc_pipeline_sinks_latency(const fdc_pipeline *p, const fdc_sinks *sinks)
{
    if (!p || !sinks) return -1;
    if (!fdc_sinks_fill_stream(const_cast<fdc_sinks *>(sinks))) return 0;
    return fdc_sinks_engine(sinks) == 1 ? 2 : 1;
}

int fdc_pipeline_work_spectrum(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum,
                               fdc_sinks *sinks)
{
    FDC_ENTRY("fdc_pipeline_work_spectrum")
    // hier block with inpveclen > 1 (py:284-290): items are spectra already; only multiply_const(1/N) and the channel /
    // sink branches remain.  The front-end state (overlap history) is untouched; the block counter advances.
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (int rcf = check_float_output(p, "fdc_pipeline_work_spectrum")) return rcf;
    const int rca = check_work_args(p, in, nblocks, outs);
    if (rca != FDC_OK || nblocks == 0) return rca;
    if (sinks && (fdc_sinks_blocklen(sinks) != p->N || nblocks > fdc_sinks_max_blocks(sinks)))
        return set_error(FDC_ERR_INVALID_ARGUMENT, "sinks were created for blocklen %d / %d blocks per call, pipeline call has %d / %d",
                    fdc_sinks_blocklen(sinks), fdc_sinks_max_blocks(sinks), p->N, nblocks);
    HIPCHK(hipSetDevice(p->cfg.device_id));
    hipStream_t s = p->stream;
    float2 *d_full = sinks ? static_cast<float2 *>(fdc_sinks_spectrum(sinks)) : nullptr;
    if (!d_full) { const int rcs = spec_staging(p, &d_full); if (rcs != FDC_OK) return rcs; }
    RCCHK(out_staging(p));
    const size_t n = (size_t)nblocks * p->N;
    HIPCHK(hipMemcpyAsync(d_full, in, sizeof(float2) * n, hipMemcpyHostToDevice, s));
    HIPCHK(fdc::launch_scale(d_full, d_full, n, 1.0f / (float)p->N, s));
    // (not run_channel_groups: this loop sends 512- and 1024-bin groups to launch_channels, not launch_channels_wide — merging would change which kernel runs)
    for (size_t g = 0; g < p->groups.size(); g++) {
        const int l = p->groups[g].first;
        if (l > 4096)
            RCCHK(channels_wide(p, d_full, p->d_out, p->d_groups + p->group_off[g], (int)p->groups[g].second.size(), l,
                                Span{nblocks, 0, nblocks, p->blockcount}, s));
        else if (l == 256 && ((256 / p->R) & 1) == 0 && !p->cfg_generic)
            HIPCHK(fdc::launch_channels256(d_full, p->d_out, p->d_chans, p->d_groups + p->group_off[g],
                                           (int)p->groups[g].second.size(), p->g_aligned[g] != 0, p->g_out_aligned[g] != 0,
                                           p->N, p->R, nblocks, 0, nblocks, p->blockcount, p->d_wins, p->d_tw256, s));
        else
            HIPCHK(fdc::launch_channels(d_full, p->d_out, p->d_chans, p->d_groups + p->group_off[g],
                                        (int)p->groups[g].second.size(), l, p->N, p->R, nblocks, 0, nblocks, p->blockcount,
                                        p->d_wins, p->d_tw, p->ntab, s));
    }
    RCCHK(copy_outputs(p, outs, nblocks, sizeof(float2), p->d_out, s));
    if (spectrum) HIPCHK(hipMemcpyAsync(spectrum, d_full, sizeof(float2) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    p->blockcount += nblocks;
    if (sinks) {
        const int rs = fdc_sinks_work_device(sinks, nblocks);
        if (rs < 0) return rs;
    }
    return nblocks;
    FDC_ENTRY_END
}

}  // extern "C"
