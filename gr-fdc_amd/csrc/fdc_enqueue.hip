// The enqueue path of the pipeline handle: what one call brings (DeviceCall), its launch groups and their kernels (process_device_impl), and the
// device entries fdc_pipeline_process_device*.
#include "fdc_pipeline.hpp"

namespace fdc { namespace pipe {

static int get_event(fdc_pipeline *p, size_t *idx)
{
    if (p->ev_used == p->events.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        p->events.push_back(e);
    }
    *idx = p->ev_used++;
    return FDC_OK;
}

DeviceCall device_call(const fdc_pipeline *p, void *stream, void *d_spectrum, int fmt, float scale)
{
    DeviceCall call;
    call.fmt = fmt; call.scale = scale;
    call.stream = stream ? static_cast<hipStream_t>(stream) : p->stream;
    call.spectrum = d_spectrum;
    call.ncu = p->ncu - p->reserved_cu;
    call.gain = p->gains_on && p->C > 0 ? p->d_gain.get() : nullptr;
    return call;
}

// Channels wider than 4096 bins: all channels of one width and all blocks of the launch group as ONE batch of the task-addressed two-pass
// inverse transform (fdc_kernels.hip: pass A reads slice * window straight from the spectrum, the ifftshift is its input rotation; pass B
// writes the kept samples, times l, into the channel streams) — in pieces of up to 32 Mi points of scratch between the passes.
// gids: the group's channel ids in the device list p->d_groups.
int channels_wide(fdc_pipeline *p, const float2 *spec, float2 *d_out, const int32_t *d_gids, int ngroup, int l, const Span &span, hipStream_t s)
{
    const int nb = span.nb;
    const int per = (int)std::max<long long>(1, std::min<long long>(nb, (long long)p->big_pts / ((long long)ngroup * l)));   // blocks per piece
    const int lout = l - l / p->R;
    for (int m0 = 0; m0 < nb; m0 += per) {
        const int n = std::min(per, nb - m0);
        HIPCHK(fdc::launch_wide_tasks(p->d_wtasks, p->d_chans, d_gids, ngroup, p->R, n, span.m0 + m0, span.nblocks, span.first_block, s));
        HIPCHK(fdc::launch_extract_wide(spec + (size_t)m0 * p->N, p->N, p->d_wtasks, n * ngroup, l, l - lout, p->d_wins, p->d_big, d_out, p->d_tw, p->ntab, s,
                                        (float)l));
    }
    return FDC_OK;
}

// The channel kernels of one launch group over the plan's channels by width (rem: over the remainder of a split plan only)
static int run_channel_groups(fdc_pipeline *p, bool rem, const float2 *spec, float2 *d_out, const Span &span, hipStream_t s)
{
    const auto &groups = rem ? p->rgroups : p->groups;
    const auto &off = rem ? p->rgroup_off : p->group_off;
    const auto &al = rem ? p->rg_aligned : p->g_aligned;
    const auto &oal = rem ? p->rg_out_aligned : p->g_out_aligned;
    const int32_t *ids = rem ? p->d_rgroups : p->d_groups;
    for (size_t g = 0; g < groups.size(); g++) {
        const int l = groups[g].first, ng = (int)groups[g].second.size();
        if (l > 4096)
            RCCHK(channels_wide(p, spec, d_out, ids + off[g], ng, l, span, s));
        else if (l == 256 && ((256 / p->R) & 1) == 0 && !p->cfg_generic)
            HIPCHK(fdc::launch_channels256(spec, d_out, p->d_chans, ids + off[g], ng, al[g] != 0, oal[g] != 0, p->N, p->R, span.nb, span.m0, span.nblocks,
                                           span.first_block, p->d_wins, p->d_tw256, s));
        else if ((l == 512 || l == 1024) && l <= p->N && !p->cfg_generic)
            HIPCHK(fdc::launch_channels_wide(spec, d_out, p->d_chans, ids + off[g], ng, l, p->N, p->R, span.nb, span.m0, span.nblocks, span.first_block,
                                             p->d_wins, p->d_tw, p->ntab, s));
        else
            HIPCHK(fdc::launch_channels(spec, d_out, p->d_chans, ids + off[g], ng, l, p->N, p->R, span.nb, span.m0, span.nblocks, span.first_block, p->d_wins,
                                        p->d_tw, p->ntab, s));
    }
    return FDC_OK;
}

// The remainder of a split plan for one launch group: forward transform into the handle's internal (partial) spectrum, channel kernels
// over the remainder's groups.  ev2 / ev3 (timing): recorded behind the forward transform and behind the channel kernels.
static int run_remainder(fdc_pipeline *p, const DeviceCall &call, const float2 *in0, float2 *d_out, const Span &span, hipEvent_t ev2, hipEvent_t ev3)
{
    hipStream_t s = call.stream;
    const int nb = span.nb;
    if (p->fwd_block && nb >= p->block_min)
        HIPCHK(fdc::launch_block_fft(p->N, in0, (size_t)p->H, p->d_spec, nb, p->d_tw256, p->d_ftwq, p->d_fcbt, p->d_fshn,
                                          p->d_fslot, p->d_fscr, call.ncu, p->block_hints, s, nullptr, p->d_keep));
    else if (p->N == 65536)
        HIPCHK(fdc::launch_fft65536(in0, (size_t)p->H, p->d_spec, p->d_tmp, nb, p->N / 2, 1.0f / (float)p->N, p->d_tw256,
                                    p->d_twf, s, nullptr));
    else
        HIPCHK(fdc::launch_fft(in0, (size_t)p->H, p->d_spec, p->d_tmp, p->N, nb, false, 0, p->N / 2, 1.0f / (float)p->N, p->d_tw, p->ntab,
                               s, nullptr, p->d_twf, p->cfg_generic));
    if (ev2) HIPCHK(hipEventRecord(ev2, s));
    RCCHK(run_channel_groups(p, true, p->d_spec, d_out, span, s));
    if (ev3) HIPCHK(hipEventRecord(ev3, s));
    return FDC_OK;
}

// one launch of the bank's block kernel over a launch group.  b: the group's part of the launch (its samples and their formats, its blocks, the events the
// dispatch itself stamps); the handle's and the bank's part is filled in here.  Integer samples: the 256-bin kernel only
static int launch_bank(fdc_pipeline *p, const DeviceCall &call, const fdc_pipeline::Bank &bk, fdc::BlockLaunch b)
{
    b.in_stride = (size_t)p->H;
    b.iscale = call.scale; b.oscale = call.oscale;
    b.slot_off = bk.d_slot_off;
    b.ncu = call.ncu; b.hints = p->block_hints;
    b.s = call.stream;
    b.N = p->N; b.R = p->R; b.scratch = p->d_fscr;
    b.L = bk.L; b.r = bk.r;
    b.cbt = bk.d_cbt; b.shn = bk.d_shn; b.tab = bk.d_tab;
    b.tw256 = p->d_tw256;
    b.twq = bk.L == 512 ? p->d_twq512 : bk.L == 1024 ? p->d_twq1k : p->d_twq;
    b.twl = bk.L == 512 ? p->d_tw512 : bk.L == 1024 ? p->d_tw1k : nullptr;
    if (bk.L != 256 && (b.ifmt || b.ofmt)) return set_error(FDC_ERR_UNSUPPORTED, "integer %s in a %d-bin bank", b.ofmt ? "stores" : "loads", bk.L);
    switch (bk.L) {
    case 256: HIPCHK(fdc::launch_poly_block(b)); break;
    case 512: HIPCHK(fdc::launch_poly_block512(b)); break;
    case 1024: HIPCHK(fdc::launch_poly_block1024(b)); break;
    default: HIPCHK(fdc::launch_poly_block_narrow(b));
    }
    return FDC_OK;
}

// whether the plan's kernels take complex integers themselves, in their loads or their stores: path 5 (k_f4096) and the banks of 256-bin channels
// (k_blk256) without a remainder — not with a spectrum or waterfall rows to write
static bool int_kernels(const fdc_pipeline *p, const DeviceCall &call)
{
    if (call.spectrum || call.rows || p->cfg_generic) return false;
    if (p->fused) return true;
    if (!p->poly_ok || !p->poly_block || p->split) return false;
    for (const auto &b : p->banks) if (b.L != 256) return false;
    return true;
}

// integer input: whether a launch group (few: shorter than block_min) reads it in its own loads; every other form reads a float ring the group is
// widened into first (k_iq_to_complex)
static bool iq_fused(const fdc_pipeline *p, const DeviceCall &call, bool few)
{
    return int_kernels(p, call) && (p->fused || !(few && two_launch_possible(p)));
}

// Path 5 (k_f4096, one launch per group) serves the call: the plan has it and no spectrum is asked for
static bool path5(const fdc_pipeline *p, const DeviceCall &call) { return p->fused && !call.spectrum; }

// THE RULE of the passes behind a plan's kernels (fdc_postpass.hip), on which oq_fused and PostPass both rest: they go over the kernels' complex
// float results in the order rotation -> gain -> levels, lag-1 -> narrowing or demodulation.  Path 5 turns its samples in its own stores; every other kernel leaves
// fine tuning to the rotation pass.  The levels are of the float samples the caller gets (turned and gained), and the gain multiplies float samples.
// The lag-1 correlation is of the same samples as the levels.
// So a call with a rotation pass, gains, levels or lag-1 has its kernels store float, and narrows behind the last of them.
static bool rotation_pass(const fdc_pipeline *p, const DeviceCall &call) { return p->fine_on && !path5(p, call); }
static bool float_passes(const fdc_pipeline *p, const DeviceCall &call) { return rotation_pass(p, call) || call.gain || call.levels || call.lag1; }

// integer output: whether EVERY launch group of a call of nblocks narrows in its own kernel's stores (k_blk256: streamed stores; not N = 65536 at R = 4
// on float input, whose forms would spill: fdc_block256.hip kOqR4Narrowed); otherwise the call writes complex float and k_complex_to_iq narrows it
// (whole call: one layout)
static bool oq_fused(const fdc_pipeline *p, const DeviceCall &call, int nblocks)
{
    if (float_passes(p, call)) return false;  // THE RULE: float, the passes, then narrowed (every path, path 5 included)
    if (oq_demod(call.ofmt)) return false;    // demodulation: never in a kernel's own stores
    if (!int_kernels(p, call)) return false;
    if (p->fused) return true;
    if (!(p->block_hints & 1) || (!call.fmt && p->N == 65536 && p->R == 4)) return false;
    for (int m0 = 0; m0 < nblocks; m0 += p->chunk)
        if (std::min(p->chunk, nblocks - m0) < p->block_min && two_launch_possible(p)) return false;
    return true;
}

// What one call runs behind its kernels: per launch group (run_post_passes), then once over the call (run_post_tail).  Filled once per call
// (post_pass) from THE RULE: a pass carries what stands behind it in that order where it can, so that a group's samples are gone over once.
struct PostPass {
    bool fine_fused = false;    // fine tuning on, and path 5 turns the samples in its own stores: no rotation pass
    bool rotate = false;        // k_fine_rotate behind the group's kernels: fine tuning on, off path 5 ...
    bool rot_gain = false;      //   ... which multiplies the turned samples by the gains
    bool rot_levels = false;    //   ... and reduces them to the levels (not under FDC_LEVELS_SEPARATE)
    bool gain_pass = false;     // k_chan_gain: gains on and no rotation pass; it sums the levels too, where they are on ...
    bool gain_narrows = false;  //   ... and stores the narrow samples, where the call narrows behind its kernels
    bool levels_pass = false;   // k_chan_levels: levels on and neither pass above carries them
    bool narrow_tail = false;   // the call-wide k_complex_to_iq from the float staging
    const float *gain = nullptr;
    float2 *levels = nullptr;
    float2 *lag1 = nullptr;     // k_chan_lag1, always a pass of its own over the group's final float results: lag-1 on
    int demod = 0;              // the call-wide k_chan_demod from the float staging, in the place of the narrowing: FDC_DEMOD_FM / _MAG
    bool demod_cont = false;    //   ... FM: the call continues the stream of the last demodulating call, whose carry stands in front of its first sample
    void *audio = nullptr;      // the call-wide k_chan_audio behind it, over the demodulated samples: the audio on (where row 0 of the call's audio goes)
    bool audio_cont = false;    //   ... the call continues the audio stream: the handle's history stands in front of its first sample
    unsigned char *squelch = nullptr;   // the call-wide k_chan_squelch over the call's levels, in front of the audio (which it gates): the squelch on
    bool squelch_cont = false;  //   ... the call continues the squelch's stream: the handle's state stands in front of its first block
    unsigned *pack_off = nullptr;   // the offsets of the call's cells in the packed audio, behind the squelch and in front of the audio (which then packs): packing on
    float2 *tones = nullptr;    // the call-wide k_chan_tones behind the demodulation, beside the audio and independent of it: the tones on (where the call's
                                // first completed frame row goes)
    bool tones_cont = false;    //   ... the call continues the tones' stream: the handle's accumulators stand in front of its first block ...
    int tones_fill = 0;         //   ... which is block tones_fill of the open frame (0 where the stream starts anew)
    unsigned char *tone_dec = nullptr;  // the call-wide k_tone_decide and k_tone_gate behind the tones and in front of the offsets and the audio: the tone squelch
                                // on (where the decisions of the call's first completed frame go).  It changes the order of the tail (run_post_tail)
    bool tsq_cont = false;      //   ... the call continues the tones' stream and the handle's tone-squelch state is valid
};

static PostPass post_pass(const fdc_pipeline *p, const DeviceCall &call, bool ofused)
{
    PostPass pp;
    if (p->C <= 0) return pp;
    pp.demod = oq_demod(call.ofmt) ? call.ofmt - kOqDemod : 0;
    const bool narrow = call.ofmt && !pp.demod && !ofused && call.narrow;
    pp.gain = call.gain; pp.levels = call.levels; pp.lag1 = call.lag1;
    pp.fine_fused = p->fine_on && path5(p, call);
    pp.rotate = rotation_pass(p, call);
    pp.rot_gain = pp.rotate && pp.gain;
    pp.rot_levels = pp.rotate && pp.levels && !p->levels_separate;
    pp.gain_pass = pp.gain && !pp.rotate;
    pp.gain_narrows = pp.gain_pass && narrow;
    pp.levels_pass = pp.levels && !pp.rot_levels && !pp.gain_pass;
    pp.narrow_tail = narrow && !pp.gain_narrows;
    pp.audio = pp.demod ? call.audio : nullptr;
    pp.squelch = pp.levels ? call.squelch : nullptr;
    pp.pack_off = pp.audio && pp.squelch ? call.pack_off : nullptr;
    pp.tones = pp.demod ? call.tones : nullptr;
    pp.tone_dec = pp.tones && pp.squelch ? call.tone_dec : nullptr;
    return pp;
}

// behind the kernels of launch group g, whose float results are in o (d_out: the call's output, narrow where the gain pass narrows)
static int run_post_passes(const fdc_pipeline *p, const DeviceCall &call, const PostPass &pp, const Span &g, float2 *o, void *d_out)
{
    hipStream_t s = call.stream;
    if (pp.rotate)
        HIPCHK(fdc::launch_fine_rotate(o, p->d_chans, p->d_fine, p->d_fstep, p->C, g.nb, g.m0, g.nblocks, g.first_block, s, pp.rot_levels ? pp.levels : nullptr,
                                       pp.rot_gain ? pp.gain : nullptr));
    if (pp.gain_pass)
        HIPCHK(fdc::launch_chan_gain(o, p->d_chans, pp.gain, pp.levels, pp.gain_narrows ? call.ofmt : 0, call.oscale, pp.gain_narrows ? d_out : nullptr, p->C, g.nb,
                                     g.m0, g.nblocks, s));
    if (pp.levels_pass) HIPCHK(fdc::launch_chan_levels(o, p->d_chans, pp.levels, p->C, g.nb, g.m0, g.nblocks, s));
    // (the narrowing gain pass has left o as it was cut: the lag-1 pass multiplies what it reads, which gives the bits of the gained samples)
    if (pp.lag1) HIPCHK(fdc::launch_chan_lag1(o, p->d_chans, pp.gain_narrows ? pp.gain : nullptr, pp.lag1, p->C, g.nb, g.m0, g.nblocks, s));
    return FDC_OK;
}

// behind the last launch group: the call-wide narrowing, and how the call was served (fdc_pipeline_describe)
static int run_post_tail(fdc_pipeline *p, const DeviceCall &call, const PostPass &pp, int64_t first_block, int nblocks, void *d_out)
{
    if (pp.squelch) {
        // the last launch group's levels are enqueued: the decision over all the call's rows.  The state is read from one buffer and written to the other,
        // which is the handle's behind the enqueue, for the call that goes on at the next block
        HIPCHK(fdc::launch_chan_squelch(pp.levels, pp.gain, p->d_sqthr[0], p->d_sqthr[1], p->sq_hang,
                                        pp.squelch_cont ? p->d_sqstate[p->sqstate_cur].get() : nullptr, p->d_sqstate[p->sqstate_cur ^ 1].get(), pp.squelch, p->C,
                                        nblocks, call.stream));
        p->sqstate_cur ^= 1; p->squelch_next = first_block + nblocks;
        p->squelch_route = "pass";
    }
    // ... and of the mask the offsets of the call's cells: from the running total on where the call appends to a host call's packed buffer
    auto pack_offsets = [&]() -> int {
        HIPCHK(fdc::launch_audio_pack_offsets(pp.squelch, p->d_chans, p->audio_decim, call.pack_append ? p->d_packtotal.get() : nullptr, pp.pack_off,
                                              p->d_packtotal, p->C, nblocks, call.stream));
        return FDC_OK;
    };
    // the tone bank over the demodulated samples, ungated: the open frame's accumulators are read from one buffer and written to the other, which
    // is the handle's behind the enqueue, with the blocks now inside the open frame, for the call that goes on at the next block
    auto tones = [&]() -> int {
        HIPCHK(fdc::launch_chan_tones(static_cast<const float *>(d_out), p->d_chans, p->d_tinc, p->d_ttab, pp.tones_cont ? p->d_tcarry[p->tcarry_cur].get() : nullptr,
                                      p->d_tcarry[p->tcarry_cur ^ 1].get(), pp.tones, p->C, p->tones_T, p->tones_S, p->tones_W, pp.tones_fill, (long long)first_block,
                                      nblocks, call.stream));
        p->tcarry_cur ^= 1; p->tones_next = first_block + nblocks; p->tones_fill = (pp.tones_fill + nblocks) % p->tones_W;
        p->tones_route = "pass";
        return FDC_OK;
    };
    // WITHOUT the tone squelch the order is squelch, offsets, demodulation, audio, tones.  WITH it the offsets and the audio must see the combined mask,
    // which needs the call's frame rows: squelch, demodulation, tones, the decision and the gate, offsets, audio
    if (pp.pack_off && !pp.tone_dec) RCCHK(pack_offsets());
    if (pp.demod) {
        // FM reads one carry buffer and writes the other; behind the enqueue the written one is the handle's, for the call that goes on at the next block
        const bool fm = pp.demod == FDC_DEMOD_FM;
        HIPCHK(fdc::launch_chan_demod(pp.demod, call.oscale, call.fout, static_cast<float *>(d_out), p->d_chans,
                                      fm && pp.demod_cont ? p->d_carry[p->carry_cur].get() : nullptr, fm ? p->d_carry[p->carry_cur ^ 1].get() : nullptr,
                                      p->C, nblocks, (long long)p->sum_lout, call.stream));
        if (fm) { p->carry_cur ^= 1; p->demod_next = first_block + nblocks; }
        p->demod_route = fm ? "fm" : "mag";
    }
    if (pp.tone_dec) {
        RCCHK(tones());
        // the decision over the frame rows the tones have just completed, and the carrier mask combined with the decision in force at each block.  The state
        // is read from one buffer (by both kernels) and written to the other, which is the handle's behind the enqueue
        HIPCHK(fdc::launch_tone_squelch(pp.tones, p->d_tsqtone, p->d_tsqthr[0], p->d_tsqthr[1], p->d_tsqthr[2], p->tsq_guard, p->tsq_hang,
                                        pp.tsq_cont ? p->d_tsqstate[p->tsqstate_cur].get() : nullptr, p->d_tsqstate[p->tsqstate_cur ^ 1].get(), pp.tone_dec,
                                        pp.squelch, p->C, p->tones_T, p->tones_W, pp.tones_fill, nblocks, call.stream));
        p->tsqstate_cur ^= 1; p->tsq_valid = true;
        p->tsq_route = "pass";
        if (pp.pack_off) RCCHK(pack_offsets());
    }
    if (pp.audio) {
        // the demodulated samples are where the demodulation has just written them; the history is read from one buffer and written to the other,
        // which is the handle's behind the enqueue, for the call that goes on at the next block
        // (the resampler in the decimating FIR's place: the same history, of Kp - 1 samples, and the call's first block, which sets its phase and counts)
        const int K = p->rs_up ? p->rs_kp : (int)p->audio_taps.size();
        if (p->rs_up)
            HIPCHK(fdc::launch_chan_resample(p->audio_format, p->rs_up, p->rs_down, K, p->audio_scale, p->d_rstaps, p->d_aoff, (long long)p->audio_row,
                                             static_cast<const float *>(d_out), pp.audio, p->d_chans,
                                             pp.audio_cont && K > 1 ? p->d_ahist[p->ahist_cur].get() : nullptr, K > 1 ? p->d_ahist[p->ahist_cur ^ 1].get() : nullptr,
                                             p->C, nblocks, (long long)p->sum_lout, (long long)first_block, call.stream, pp.squelch));
        else
            HIPCHK(fdc::launch_chan_audio(p->audio_format, p->audio_decim, K, p->audio_scale, p->d_ataps, p->d_aoff, (long long)p->audio_row,
                                          static_cast<const float *>(d_out), pp.audio, p->d_chans,
                                          pp.audio_cont && K > 1 ? p->d_ahist[p->ahist_cur].get() : nullptr, K > 1 ? p->d_ahist[p->ahist_cur ^ 1].get() : nullptr,
                                          p->C, nblocks, (long long)p->sum_lout, call.stream, pp.squelch, pp.pack_off));
        p->ahist_cur ^= 1; p->audio_next = first_block + nblocks;
        p->audio_route = p->rs_up ? (pp.squelch ? "resampled, gated" : "resampled") : pp.pack_off ? "pass, gated, packed" : pp.squelch ? "pass, gated" : "pass";
    }
    if (pp.tones && !pp.tone_dec) RCCHK(tones());
    if (pp.narrow_tail) HIPCHK(fdc::launch_complex_to_iq(call.ofmt, call.oscale, call.fout, d_out, (size_t)nblocks * p->sum_lout, call.stream));
    if (pp.fine_fused || pp.rotate) p->fine_route = pp.fine_fused ? "fused" : "rotated";
    if (pp.levels) p->levels_route = pp.rot_levels ? "with the rotation" : pp.gain_pass ? "with the gains" : "pass";
    if (pp.lag1) p->lag1_route = "pass";
    if (pp.gain) p->gains_route = pp.rot_gain ? "with the rotation" : pp.gain_narrows ? "with the narrowing" : "pass";
    return FDC_OK;
}

// The enqueue path of every entry: nblocks blocks from d_ring (the stream's block first_block first) to d_out, as `call` says; its results say how
int process_device_impl(fdc_pipeline *p, DeviceCall &call, const void *d_ring, int64_t first_block, int nblocks, void *d_out)
{
    if (nblocks < 0 || first_block < 0) return set_error(FDC_ERR_INVALID_ARGUMENT, "negative block count/index");
    if (nblocks == 0) return FDC_OK;
    if (!d_ring || (p->C > 0 && !d_out)) return set_error(FDC_ERR_INVALID_ARGUMENT, "null device buffer");
    void *const d_spectrum = call.spectrum;
    if (d_spectrum && !p->cfg.keep_spectrum && !call.own_spectrum) return set_error(FDC_ERR_INVALID_ARGUMENT, "spectrum output needs keep_spectrum");
    // one call produces less than 4 GiB (32-bit output offsets; checked for max_blocks at create): a longer call is refused, not sent down
    // a path whose internal spectrum may be partial (a split plan's remainder-only spectrum under the channel kernels of ALL channels)
    if ((int64_t)nblocks * p->sum_lout * 8 > 0xFFFFF000ll)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "nblocks %d x %lld output samples per block is more than the 4 GiB one call may produce", nblocks, (long long)p->sum_lout);
    HIPCHK(hipSetDevice(p->cfg.device_id));
    hipStream_t s = call.stream;
    const int fmt = call.fmt, ofmt = call.ofmt;
    const float2 *ring = static_cast<const float2 *>(d_ring);
    const unsigned char *iring = static_cast<const unsigned char *>(d_ring);
    const size_t esz = fdc::iq_bytes(fmt);
    const bool ofused = ofmt && oq_fused(p, call, nblocks);
    call.ofused = ofused;
    if (ofmt && !ofused && !call.fout) return set_error(FDC_ERR_INVALID_ARGUMENT, "integer output: no float staging");
    float2 *o = ofmt && !ofused ? call.fout : static_cast<float2 *>(d_out);
    const size_t osz = ofused ? fdc::iq_bytes(ofmt) : sizeof(float2);       // bytes per sample the kernels store
    unsigned char *const ob = ofused ? static_cast<unsigned char *>(d_out) : reinterpret_cast<unsigned char *>(o);
    const bool use_poly = p->poly_ok && !d_spectrum;
    const unsigned out_bytes = (unsigned)((int64_t)nblocks * p->sum_lout * (int64_t)osz);
    PostPass pp = post_pass(p, call, ofused);            // what runs behind the kernels of every launch group and behind the call: decided here, once
    if (pp.demod == FDC_DEMOD_FM) {
        // the carry is the sample in front of this call's first only where the call goes on at the block after the last demodulating call's last;
        // a call that fails from here on leaves nothing to continue
        pp.demod_cont = p->demod_next == first_block;
        p->demod_next = -1;
    }
    if (pp.audio) {
        // the same rule for the audio's history, in both modes
        pp.audio_cont = p->audio_next == first_block;
        p->audio_next = -1;
    }
    if (pp.squelch) {
        // ... and for the squelch's state
        pp.squelch_cont = p->squelch_next == first_block;
        p->squelch_next = -1;
    }
    call.tones_frames = 0;
    if (pp.tones) {
        // ... and for the tones' open frame: its accumulators and how many blocks are inside it
        pp.tones_cont = p->tones_next == first_block;
        pp.tones_fill = pp.tones_cont ? p->tones_fill : 0;
        p->tones_next = -1;
    }
    if (pp.tone_dec) {
        // ... and the tone squelch goes on exactly where the tones do, unless its setting is new
        pp.tsq_cont = pp.tones_cont && p->tsq_valid;
        p->tsq_valid = false;
    }
    // path 5: the call's part of every group's launch (the group's: its input, its blocks and its waterfall rows)
    fdc::F4Launch f4{};
    if (p->fused && !d_spectrum) {
        f4.iscale = call.scale; f4.in_stride = (size_t)p->H;
        f4.out = ofused ? d_out : o; f4.ofmt = ofused ? ofmt : 0; f4.oscale = call.oscale;
        f4.R = p->R; f4.nb_call = nblocks; f4.first_block = first_block;
        f4.tw = p->d_tw; f4.ntab = p->ntab; f4.wins = p->d_wins;
        f4.rows = p->d_f4rows; f4.wcls = p->f4_cls; f4.teams = p->f4_teams;
        if (pp.fine_fused) { f4.fine_rows = p->d_f4fine; f4.fine_step = p->d_fstep; }
        f4.s = s;
    }
    for (int m0 = 0; m0 < nblocks; m0 += p->chunk) {
        const int nb = std::min(p->chunk, nblocks - m0);
        const Span grp{nb, m0, nblocks, first_block};
        float2 *spec = d_spectrum ? static_cast<float2 *>(d_spectrum) + (size_t)m0 * p->N : p->d_spec;
        hipEvent_t ev[3]; hipEvent_t *evp = nullptr; std::array<size_t, 5> span{};
        // events on every timing_stride-th launch group only: a sample of the launches, so that the packets between the
        // kernels (measured 7-17 us per group) do not slow the region they time
        const bool tg = p->timing && (p->timing_seq++ % p->timing_stride) == 0;
        if (tg) {
            for (int i = 0; i < 4; i++) RCCHK(get_event(p, &span[i]));
            for (int i = 0; i < 3; i++) ev[i] = p->events[span[i]];
            evp = ev;
        }
        const float2 *in0 = ring + (size_t)m0 * p->H;
        const void *raw0 = iring + (size_t)m0 * p->H * esz;
        const bool few = nb < p->block_min;
        const bool ifused = fmt && iq_fused(p, call, few);
        if (fmt && !ifused) {
            // this launch group's samples (nb blocks and the history in front of the last one) widened into the float ring the kernels read
            HIPCHK(fdc::launch_iq_to_complex(fmt, call.scale, raw0, call.wide, (size_t)nb * p->H + (size_t)p->ovl, s));
            in0 = call.wide;
            call.all_fused = false;
        }
        // overlap-save gather fused into the load (item m at ring + m*H), fftshift + 1/N into the store.
        // A block kernel gives a whole block to one compute unit: a launch group of fewer blocks than the device has compute
        // units leaves the rest idle (one block takes ~42 us there, however few there are).  Short calls — a scheduler handing
        // over a few items — take the two-launch form where the plan has one (ONE bank on its grid), which spreads every block over the device.
        if (p->fused && !d_spectrum) {
            // N = 4096: one launch, nothing but the input samples and the output samples crosses the memory interface
            if (tg) HIPCHK(hipEventRecord(p->events[span[0]], s));
            float *wf = call.rows ? call.rows + (size_t)(first_block - call.rows_first + m0) * fdc::kWfWidth : nullptr;
            f4.in = ifused ? raw0 : in0; f4.ifmt = ifused ? fmt : 0;
            f4.nb_chunk = nb; f4.mbase = m0; f4.wf = wf;
            HIPCHK(fdc::launch_fused4096(f4));
            if (tg) { HIPCHK(hipEventRecord(p->events[span[1]], s)); span[2] = span[3] = span[1]; span[4] = kSpanBanks; p->ev_spans.push_back(span); }
            RCCHK(run_post_passes(p, call, pp, grp, o, d_out));
            continue;
        }
        if (use_poly && p->poly_block && !(few && two_launch_possible(p))) {
            // one launch per bank: nothing but the input rows and the output samples crosses the memory interface.
            // timing: the first launch's begin and the last one's end are the dispatches' own stamps, no packets around the kernels
            fdc::BlockLaunch b{};
            b.in = ifused ? raw0 : in0; b.ifmt = ifused ? fmt : 0;
            b.out = ofused ? d_out : o; b.ofmt = ofused ? ofmt : 0;
            b.nb_chunk = nb; b.mbase = m0; b.nb_call = nblocks;
            b.first_block = first_block + m0; b.out_bytes = out_bytes;
            for (size_t k = 0; k < p->banks.size(); k++) {
                b.ev_start = tg && k == 0 ? p->events[span[0]] : nullptr;
                b.ev_stop = tg && k + 1 == p->banks.size() ? p->events[span[1]] : nullptr;
                RCCHK(launch_bank(p, call, p->banks[k], b));
            }
            for (const auto &al : p->bank_alias) {
                const fdc::ChanDev &dc = p->chans[(size_t)al.first], &sc = p->chans[(size_t)al.second];
                HIPCHK(hipMemcpyAsync(ob + osz * ((size_t)nblocks * dc.out_off + (size_t)m0 * dc.lout), ob + osz * ((size_t)nblocks * sc.out_off + (size_t)m0 * sc.lout),
                                      osz * (size_t)nb * dc.lout, hipMemcpyDeviceToDevice, s));
            }
            if (p->split) RCCHK(run_remainder(p, call, in0, o, grp, tg ? p->events[span[2]] : nullptr, tg ? p->events[span[3]] : nullptr));
            else if (tg) span[2] = span[3] = span[1];
            if (tg) { span[4] = kSpanBanks; p->ev_spans.push_back(span); }
            RCCHK(run_post_passes(p, call, pp, grp, o, d_out));
            continue;
        }
        if (use_poly) {
            // ONE bank on its grid: window + IFFT commuted in front of pass B; only G (lout * N / l per block) between the two launches
            const fdc_pipeline::Bank &bk = p->banks[0];
            if (tg) HIPCHK(hipEventRecord(p->events[span[0]], s));
            if (bk.L != 256)
                HIPCHK(fdc::launch_poly_stage1_generic(in0, (size_t)p->H, p->d_g, p->N, bk.L, p->R, nb, bk.d_shn, p->d_tw, p->ntab, p->d_t2g, s));
            else
                HIPCHK(fdc::launch_poly_stage1(in0, (size_t)p->H, p->d_g, p->N / 256, p->R, nb, p->d_tw256, p->d_twq, bk.d_cbt, bk.d_shn, call.ncu, s));
            if (tg) { HIPCHK(hipEventRecord(p->events[span[1]], s)); span[2] = span[1]; }   // the end of stage 1 IS the start of stage 2
            if (bk.L != 256)
                HIPCHK(fdc::launch_poly_stage2_generic(p->d_g, o, p->N / bk.L, p->R, nb, m0, nblocks, bk.d_slot_off, p->d_tw, p->ntab, s, bk.L));
            else if (p->N != 65536 && p->N != 262144)
                HIPCHK(fdc::launch_poly_stage2_generic(p->d_g, o, p->N / 256, p->R, nb, m0, nblocks, bk.d_slot_off, p->d_tw, p->ntab, s));
            else
                HIPCHK(fdc::launch_poly_stage2(p->d_g, o, p->N / 256, p->R, nb, m0, nblocks, p->d_tw256, p->d_tw1024, bk.d_slot_off, out_bytes, call.ncu, s));
            if (p->split) RCCHK(run_remainder(p, call, in0, o, grp, nullptr, nullptr));   // (timing: the remainder is counted with stage 2)
            RCCHK(run_post_passes(p, call, pp, grp, o, d_out));
            if (tg) {
                HIPCHK(hipEventRecord(p->events[span[3]], s));
                span[4] = kSpanTwoLaunch;
                p->ev_spans.push_back(span);
            }
            continue;
        }
        // a spectrum in memory.  (A split plan's internal spectrum holds its remainder's bins only: whoever gets here with one — a caller's
        // spectrum buffer — writes a full spectrum into THAT buffer, d_keep is not applied.)
        // the power of the 16-bin groups of the caller's spectrum (fdc_pipeline_process_device_power): summed by the block kernel while the bins are in
        // its registers; by a pass over the spectrum where another transform ran
        float *const gp = (call.gpow && d_spectrum) ? call.gpow + (size_t)(spec - call.gpow_origin) / 16 : nullptr;
        if (gp) p->gpow_src |= (p->fwd_block && !few) ? 1 : 2;
        if (p->fwd_block && !few)
            HIPCHK(fdc::launch_block_fft(p->N, in0, (size_t)p->H, spec, nb, p->d_tw256, p->d_ftwq, p->d_fcbt,
                                              p->d_fshn, p->d_fslot, p->d_fscr, call.ncu, p->block_hints, s, evp, d_spectrum ? nullptr : p->d_keep, gp));
        else {
            if (p->N == 65536 && !p->cfg_generic)
                HIPCHK(fdc::launch_fft65536(in0, (size_t)p->H, spec, p->d_tmp, nb, p->N / 2,
                                            1.0f / (float)p->N, p->d_tw256, p->d_twf, s, evp));
            else
                HIPCHK(fdc::launch_fft(in0, (size_t)p->H, spec, p->d_tmp, p->N, nb, false, 0, p->N / 2,
                                       1.0f / (float)p->N, p->d_tw, p->ntab, s, evp, p->d_twf, p->cfg_generic, d_spectrum ? ~0ull : p->keep4096));
            if (gp) HIPCHK(fdc::launch_group_power(spec, p->N, nb, gp, s));
        }
        RCCHK(run_channel_groups(p, false, spec, o, grp, s));
        RCCHK(run_post_passes(p, call, pp, grp, o, d_out));
        if (tg) {
            HIPCHK(hipEventRecord(p->events[span[3]], s));
            span[4] = p->N <= fdc::kMaxLdsFft ? kSpanSpectrumLds : kSpanSpectrum;
            p->ev_spans.push_back(span);
        }
    }
    RCCHK(run_post_tail(p, call, pp, first_block, nblocks, d_out));
    if (pp.tones) call.tones_frames = (pp.tones_fill + nblocks) / p->tones_W;      // (counts the host has: nothing is read back to learn it)
    return FDC_OK;
}

void levels_written(fdc_pipeline *p, int nblocks, hipStream_t stream, bool host)
{
    p->lev_blocks = nblocks; p->lev_stream = stream; p->lev_host = host;
}

void lag1_written(fdc_pipeline *p, int nblocks, hipStream_t stream, bool host)
{
    p->lag_blocks = nblocks; p->lag_stream = stream; p->lag_host = host;
}

void audio_written(fdc_pipeline *p, int64_t first_block, int nblocks, hipStream_t stream, bool host)
{
    p->aud_first = first_block; p->aud_blocks = nblocks; p->aud_stream = stream; p->aud_host = host;
}

void squelch_written(fdc_pipeline *p, int nblocks, hipStream_t stream, bool host)
{
    p->sq_blocks = nblocks; p->sq_stream = stream; p->sq_host = host;
}

void tones_written(fdc_pipeline *p, int nblocks, int nframes, hipStream_t stream, bool host)
{
    p->tn_blocks = nblocks; p->tn_frames = nframes; p->tn_stream = stream; p->tn_host = host;
}

void tone_squelch_written(fdc_pipeline *p, int nblocks, int nframes, hipStream_t stream, bool host)
{
    p->tsq_blocks = nblocks; p->tsq_frames = nframes; p->tsq_stream = stream; p->tsq_host = host;
}

// how the last integer-input / integer-output call was served (fdc_pipeline_describe): "<sc16|sc8>: fused", or what it was instead
std::string route(int fmt, bool fused, const char *otherwise)
{
    return std::string(fmt == FDC_IQ_SC16 ? "sc16" : "sc8") + ": " + (fused ? "fused" : otherwise);
}

// The device entries with the handle's output format: integer output needs the float staging (p->d_out, max_blocks*sum_lout samples, allocated by
// fdc_pipeline_set_output_format, never on this enqueue path) where the call's kernels do not narrow themselves
// Channel levels (p->levels_on): the call's levels go to the handle's buffer ([max_blocks][C], allocated by fdc_pipeline_set_levels), so such a call
// needs nblocks <= max_blocks too; nothing is enqueued otherwise.  The channel lag-1 correlation (p->lag1_on, d_lag1) likewise
// Channel demodulation (p->demod_mode): the call's real output comes from the float staging too, so nblocks <= max_blocks as well; the channel
// audio behind it (p->audio_decim) goes to the handle's d_audio while d_out receives the demodulated samples as ever
static int process_device_oq(fdc_pipeline *p, DeviceCall &call, const void *d_ring, int64_t first_block, int nblocks, void *d_out)
{
    const int ofmt = p->out_form;
    if (p->demod_mode && nblocks > 0 && p->C > 0) {
        if (nblocks > p->cfg.max_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel demodulation: nblocks %d above max_blocks %d", nblocks, p->cfg.max_blocks);
        if (!p->d_out && p->sum_lout > 0) return set_error(FDC_ERR_HIP, "channel demodulation: no float staging");
        call.ofmt = out_code(p); call.oscale = p->demod_gain; call.fout = p->d_out;
        call.audio = audio_rows(p, 0);          // (the audio goes to the handle's buffer, [max_blocks][A]: the check above covers it)
        call.tones = tones_rows(p, 0);          // (and the frame rows to the handle's, [(max_blocks + W - 1) div W][C][T]: likewise)
    }
    const bool lev = p->levels_on && nblocks > 0;
    if (lev) {
        if (nblocks > p->cfg.max_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel levels: nblocks %d above max_blocks %d", nblocks, p->cfg.max_blocks);
        call.levels = p->d_levels;
        call.squelch = squelch_rows(p, 0);      // (the mask goes to the handle's buffer, [max_blocks][C]: the check above covers it)
    }
    if (call.audio && call.squelch && packing_on(p)) { call.audio = p->d_audio.get(); call.pack_off = pack_rows(p, 0); call.pack_append = false; }
    if (call.tones && call.squelch) call.tone_dec = tone_dec_rows(p, 0);   // (the decisions go to the handle's buffer, a byte per frame row of the tones')
    const bool lag = p->lag1_on && nblocks > 0;
    if (lag) {
        if (nblocks > p->cfg.max_blocks) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel lag-1 correlation: nblocks %d above max_blocks %d", nblocks, p->cfg.max_blocks);
        call.lag1 = p->d_lag1;
    }
    if (ofmt && nblocks > 0) {
        call.ofmt = ofmt; call.oscale = p->out_scale; call.fout = p->d_out;
        if (!oq_fused(p, call, nblocks)) {
            if (nblocks > p->cfg.max_blocks)
                return set_error(FDC_ERR_INVALID_ARGUMENT, "integer output on this plan: nblocks %d above max_blocks %d", nblocks, p->cfg.max_blocks);
            if (!p->d_out && p->sum_lout > 0) return set_error(FDC_ERR_HIP, "integer output: no float staging");
        }
    }
    const int rc = process_device_impl(p, call, d_ring, first_block, nblocks, d_out);
    if (rc == FDC_OK && ofmt && nblocks > 0) p->oq_route = route(ofmt, call.ofused, "narrowed");
    if (rc == FDC_OK && lev) levels_written(p, nblocks, call.stream, false);
    if (rc == FDC_OK && lag) lag1_written(p, nblocks, call.stream, false);
    if (rc == FDC_OK && call.audio) audio_written(p, first_block, nblocks, call.stream, false);
    if (rc == FDC_OK && call.squelch) squelch_written(p, nblocks, call.stream, false);
    if (rc == FDC_OK && call.tones) tones_written(p, nblocks, call.tones_frames, call.stream, false);
    if (rc == FDC_OK && call.tone_dec) tone_squelch_written(p, nblocks, call.tones_frames, call.stream, false);
    return rc;
}

int check_iq_form(int32_t format, float scale)
{
    if (format != FDC_IQ_SC16 && format != FDC_IQ_SC8) return set_error(FDC_ERR_INVALID_ARGUMENT, "unknown complex integer format %d", (int)format);
    if (!std::isfinite(scale) || scale == 0.0f) return set_error(FDC_ERR_INVALID_ARGUMENT, "the scale must be finite and not zero");
    return FDC_OK;
}

} }  // namespace fdc::pipe

using namespace fdc::pipe;

extern "C" {

int fdc_pipeline_process_device(fdc_pipeline *p, const void *d_ring, int64_t first_block, int nblocks,
                                void *d_out, void *d_spectrum, void *stream)
{
    FDC_ENTRY("fdc_pipeline_process_device")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    DeviceCall call = device_call(p, stream, d_spectrum);
    return process_device_oq(p, call, d_ring, first_block, nblocks, d_out);
    FDC_ENTRY_END
}

int fdc_pipeline_process_device_iq(fdc_pipeline *p, int32_t format, float scale, const void *d_ring, int64_t first_block, int nblocks,
                                   void *d_out, void *d_spectrum, void *stream)
{
    FDC_ENTRY("fdc_pipeline_process_device_iq")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    RCCHK(check_iq_form(format, scale));
    if (reinterpret_cast<uintptr_t>(d_ring) & 3) return set_error(FDC_ERR_INVALID_ARGUMENT, "the integer ring must be 4-byte aligned");
    DeviceCall call = device_call(p, stream, d_spectrum, format, scale);
    if (nblocks > 0 && !p->d_iqw) {
        bool need = false;      // the widened launch group: allocated at the first call that has a form without integer loads
        for (int m0 = 0; m0 < nblocks && !need; m0 += p->chunk) need = !iq_fused(p, call, std::min(p->chunk, nblocks - m0) < p->block_min);
        if (need) {
            HIPCHK(hipSetDevice(p->cfg.device_id));
            HIPCHK(p->d_iqw.alloc((size_t)p->chunk * p->H + (size_t)p->ovl));
        }
    }
    call.wide = p->d_iqw;
    const int rc = process_device_oq(p, call, d_ring, first_block, nblocks, d_out);
    if (rc == FDC_OK && nblocks > 0) p->iq_route = route(format, call.all_fused, "widened");
    return rc;
    FDC_ENTRY_END
}

int fdc_pipeline_process_device_power(fdc_pipeline *p, const void *d_ring, int64_t first_block, int nblocks, void *d_out, void *d_spectrum,
                                      void *d_group_power, void *stream)
{
    FDC_ENTRY("fdc_pipeline_process_device_power")
    if (!p) return set_error(FDC_ERR_INVALID_ARGUMENT, "null handle");
    if (p->out_form) return set_error(FDC_ERR_INVALID_ARGUMENT, "fdc_pipeline_process_device_power writes complex float outputs only (the handle's output format is not FC32)");
    if (p->fine_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "fdc_pipeline_process_device_power writes the channels as they are cut: switch fine tuning off first");
    if (p->levels_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "fdc_pipeline_process_device_power gives no channel levels: switch them off first (fdc_pipeline_set_levels(p, 0))");
    if (p->lag1_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "fdc_pipeline_process_device_power gives no channel lag-1 correlation: switch it off first (fdc_pipeline_set_lag1(p, 0))");
    if (p->demod_mode) return set_error(FDC_ERR_INVALID_ARGUMENT, "fdc_pipeline_process_device_power writes complex float outputs only: switch the channel demodulation off first (fdc_pipeline_set_demod(p, FDC_DEMOD_OFF, 1))");
    if (p->gains_on) return set_error(FDC_ERR_INVALID_ARGUMENT, "fdc_pipeline_process_device_power writes the channels as they are cut: switch the channel gains off first (fdc_pipeline_set_gains(p, NULL, C))");
    if (d_group_power && (!d_spectrum || (p->N & 15))) return set_error(FDC_ERR_INVALID_ARGUMENT, "group powers go with a spectrum output of a block length that is a multiple of 16");
    DeviceCall call = device_call(p, stream, d_spectrum);
    call.gpow = static_cast<float *>(d_group_power);
    call.gpow_origin = static_cast<const float2 *>(d_spectrum);
    return process_device_impl(p, call, d_ring, first_block, nblocks, d_out);
    FDC_ENTRY_END
}

}  // extern "C"
