// The pipeline handle and what the files that work on it share (private to csrc):
//   fdc_api.hip      the library's plumbing (error text, device selection, host registration, selftests), create / destroy / preview /
//                    describe, the accessors and the settings
//   fdc_plan.hip     fdc_pipeline_create's four steps: validate -> channel records -> classify_plan -> device tables and scratch
//   fdc_enqueue.hip  the enqueue path: DeviceCall, process_device_impl, the fdc_pipeline_process_device* entries
//   fdc_work.hip     the host entries: work, work_real, work_iq, the span forms, waterfall, sinks, work_spectrum
//   fdc_faces.hip    the single-block faces (overlap_save, vector_cut, phase_window, fft_vcc)
// The handle owns its device and pinned memory (fdc_buffers.hpp): `delete p` frees it.  Streams and events are raw handles that
// fdc_pipeline_destroy synchronises and destroys first.  A buffer that is null has not been needed yet: the lazy sites test that.
#pragma once
#include "../../include/fdc_amd.h"
#include "fdc_buffers.hpp"
#include "fdc_kernels.h"
#include "fdc_window.hpp"
#include "fdc_guard.hpp"
#include "fdc_plan_cost.hpp"
#include "fdc_waterfall.hpp"
#include "fdc_iq.hpp"
#include "fdc_fine.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace fdc {
int pick_device(int device_id);                   // fdc_api.hip; set_error: fdc_guard.hpp
const char *debug_env(const char *name);
}  // namespace fdc
using fdc::pick_device;
using fdc::set_error;

#define HIPCHK(expr)                                                                                        \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return set_error(FDC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define RCCHK(expr) do { const int _rc = (expr); if (_rc != FDC_OK) return _rc; } while (0)   // a callee's status (it has set the error text)
// inside create: out of device memory is its own status
#define CHK_DEV(expr)                                                                           \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return set_error(_e == hipErrorOutOfMemory ? FDC_ERR_NOMEM : FDC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// body of an extern "C" entry: nothing thrown inside crosses the C boundary (fdc_guard.hpp)
#define FDC_ENTRY(name) return fdc::guarded(name, [&]() -> int {
#define FDC_ENTRY_END });

// launch groups below this many blocks do not go to the one-block-per-CU kernels (see fdc_pipeline_process_device)
constexpr int kBlockMinBlocks = 96;

struct fdc_pipeline {
    fdc_pipeline_cfg cfg{};
    int N = 0, R = 0, ovl = 0, H = 0, C = 0;
    int chunk = 0;
    int64_t sum_lout = 0;
    std::vector<fdc::ChanDev> chans;
    std::vector<std::pair<int, std::vector<int32_t>>> groups;   // (l, channel ids)
    std::vector<size_t> group_off;
    hipStream_t stream = nullptr;
    // device memory
    fdc::DevBuf<float2> d_tw; int ntab = 0;
    fdc::DevBuf<float2> d_wins;
    fdc::DevBuf<float2> d_tw256;   // fast path: exp(-2 pi i j/256)
    fdc::DevBuf<float2> d_tw1024;  // uniform path with 1024 slots: exp(-2 pi i j/1024)
    fdc::DevBuf<float2> d_twf;     // fast path: [k2][n1] inter-pass twiddles of the 256x256 transform
    std::vector<char> g_aligned, g_out_aligned;   // per channel group
    // ---- the plan (classify_plan): what runs without a spectrum in memory
    // A BANK is a set of channels of ONE width l on ONE grid f = l slot + r with ONE window, every slot at most once: one launch of the
    // width's block kernel per launch group (fdc_block256.hip: l = 256, any r; fdc_block512.hip / fdc_block1024.hip: r = 0 or l/2;
    // fdc_blocknarrow.hip: l = 128 / 64, r a multiple of l/4), or — a plan that is ONE on-grid bank where no block kernel applies, and
    // launch groups shorter than block_min — the two-launch form (stage 1 + stage 2 through the scratch G).  A plan may line up banks of
    // DIFFERENT widths (round 5); what fits no bank is the remainder of a split plan.
    struct Bank {
        int L = 256, r = 0;
        float passbw = 0, stopbw = 0;
        std::vector<int> chan;
        fdc::DevBuf<float2> d_cbt;            // per-column constants of the width's kernel (offset and (-1)^n1 folded in)
        fdc::DevBuf<float> d_shn;             // window shape / N (512 / 1024 at r = l/2: halves swapped)
        fdc::DevBuf<long long> d_slot_off;    // slot -> output offset of the channel, -1 = unused
        fdc::DevBuf<float2> d_tab;            // narrow kernel: its LDS image
    };
    std::vector<Bank> banks;
    bool poly_ok = false;        // banks is not empty
    bool poly_block = false;     // every bank has a block kernel: one launch per bank (path 3; with a remainder: path 4)
    std::vector<std::pair<int, int>> bank_alias;             // (channel, the earlier channel with the same slice and window): computed once, copied
    // tables the banks of one width share
    fdc::DevBuf<float2> d_tw512, d_twq512;                   // W_512^k, W_N^(16 n1 q) with 128 columns
    fdc::DevBuf<float2> d_tw1k, d_twq1k;                     // W_1024^k, W_N^(16 n1 q) with 64 columns
    fdc::DevBuf<float2> d_t2g;                               // generic two-launch form of ONE bank of another width: W_N^(t k2), tile order
    // Split plans (round 4; N = 65536): the channels that fit no bank — other widths, odd offsets, what the cost rule sends back — are the
    // REMAINDER: the banks take one block-kernel launch each, the remainder takes the spectrum path on a PARTIAL spectrum (the forward
    // kernel writes only the 64-bin groups a remainder channel reads) and channel kernels over the remainder's groups.
    bool split = false;
    std::vector<int> rem;                                        // channel ids of the remainder
    std::vector<std::pair<int, std::vector<int32_t>>> rgroups;   // the remainder by width, like `groups`
    std::vector<size_t> rgroup_off;
    std::vector<char> rg_aligned, rg_out_aligned;
    fdc::DevBuf<int32_t> d_rgroups;
    int block_hints = 1;         // FDC_BLOCK_HINTS: 1 = nt output stores, 2 = nt input loads
    int block_min = kBlockMinBlocks;   // FDC_BLOCK_MIN_BLOCKS (tests: 1 = the block kernels at any size)
    fdc::DevBuf<float2> d_g;                     // uniform path (two launches): stage-1 output G, chunk*lout*N/256 samples
    int ncu = 0;                                 // compute units of the handle's device
    int reserved_cu = 0;                         // what fdc_pipeline_reserve_compute_units stored (nothing else writes it): left out of the persistent kernels' grids
    fdc::DevBuf<float2> d_twq;                   // banks of 256-bin channels: W_N^(16 n1 q)
    // N = 65536 spectrum path: forward transform by the block kernel (fdc_block256.hip, FWD), own r = 0 tables
    bool fwd_block = false;
    // N = 4096 in one launch (fdc_fused4096.hip; fdc_pipeline_path() = 5): the spectrum of a block stays in LDS.  A workgroup takes f4_teams blocks (one
    // or two); f4_wave[w]: the rows wave w runs, up to eight (2 channel + block of the workgroup; one width per wave), f4_cls the kernel's class nibble
    // per wave; the device schedule is made in build_device_state
    bool fused = false;
    std::vector<int> f4_wave[8];
    unsigned f4_cls = 0;
    int f4_teams = 2;            // blocks per workgroup the schedule is made for
    fdc::DevBuf<fdc::F4Row> d_f4rows;
    fdc::DevBuf<float2> d_ftwq, d_fcbt;
    fdc::DevBuf<float> d_fshn;
    fdc::DevBuf<long long> d_fslot;
    fdc::DevBuf<float2> d_fscr;  // 256 KiB per compute unit: the half of T the block kernel puts aside between its two stage-2 runs
    fdc::DevBuf<fdc::ChanDev> d_chans;
    fdc::DevBuf<int32_t> d_groups;
    // plans that read part of the band only: 64-bin groups of the shifted spectrum some channel reads (the forward kernels that store
    // whole 64-bin runs per wave leave the other groups of the handle's internal spectrum unwritten)
    unsigned long long keep4096 = ~0ull;   // N = 4096
    fdc::DevBuf<unsigned> d_keep;          // N = 65536, block forward transform: [klo][k2 / 64] words, bit = register index of the slot
    fdc::DevBuf<float2> d_big;   // channels wider than 4096 bins: scratch between the two passes of their inverse transform (big_pts points)
    fdc::DevBuf<fdc::ExtractTask> d_wtasks;   // ... and their (channel, block) tasks of one piece
    size_t big_pts = 0;
    int big_l = 0;
    fdc::DevBuf<float2> d_tmp;   // two-pass intermediate, chunk*N
    fdc::DevBuf<float2> d_spec;  // spectrum, chunk*N (or max_blocks*N with keep_spectrum)
    fdc::DevBuf<float2> d_ring;  // work(): ovl + max_blocks*H
    fdc::DevBuf<float2> d_specfull; // work() with a host spectrum (debug port) and no bank to put it in: max_blocks*N, allocated at the first such call
    fdc::DevBuf<float> d_real;   // work_real(): max_blocks*H real samples
    // complex integer input (fdc_pipeline_work_iq and friends).  The input form of the work calls is latched by the first one after create / reset:
    // in_form -1 = none yet, 0 = float (work, work_real, ...), FDC_IQ_SC16 / FDC_IQ_SC8 with in_scale
    int in_form = -1;
    float in_scale = 0.f;
    fdc::DevBuf<unsigned char> d_iq;   // work_iq(): the integer ring, ovl + max_blocks*H samples of fdc::kIqRingBytes (the widest format; its first ovl
                                       // samples of the latched format: the history)
    fdc::DevBuf<float2> d_iqw;   // process_device_iq(): one launch group widened, chunk*H + ovl samples (paths without integer loads)
    std::string iq_route;        // how the last integer-input call was served (fdc_pipeline_describe)
    // complex integer output (fdc_pipeline_set_output_format): a setting, not a latch; out_form 0 = complex float, FDC_OQ_SC16 / FDC_OQ_SC8 with out_scale
    int out_form = 0;
    float out_scale = 1.f;
    fdc::DevBuf<unsigned char> d_oq; // host entries: the narrow results, max_blocks*sum_lout samples of fdc::kIqRingBytes (the widest format), allocated
                                     // at the first integer-output call
    std::string oq_route;        // how the last integer-output call was served (fdc_pipeline_describe)
    // fine tuning (fdc_pipeline_set_fine_tuning): a setting like the output format.  fine_on: some increment is not zero; the tables are allocated by the
    // first call that switches it on and rewritten by every later one: d_fine[c] = (inc_c, where channel c's lout_c step factors start in d_fstep),
    // d_f4fine the same per row of path 5's schedule (d_f4rows)
    bool fine_on = false;
    fdc::DevBuf<fdc::FineChan> d_fine, d_f4fine;
    fdc::DevBuf<float2> d_fstep;
    std::string fine_route;      // how the last call with fine tuning was served (fdc_pipeline_describe)
    // channel levels (fdc_pipeline_set_levels): a setting like the two above.  d_levels: [max_blocks][C] (power, peak) of the last call, row = block of the
    // call; pin_levels its pinned twin, which a host entry fills in front of its synchronise (lev_host) and fdc_pipeline_levels fills after a device entry,
    // behind a synchronise of the stream that one ran on (lev_stream).  Both are allocated by the first call that switches the setting on.
    bool levels_on = false;
    bool levels_separate = false;   // FDC_LEVELS_SEPARATE=1 (debug environment): rotation and levels as two passes where one merged pass would run (A/B testing)
    fdc::DevBuf<float2> d_levels;
    fdc::PinBuf<float2> pin_levels;
    int lev_blocks = -1;         // block count of the last successful work call with levels on (-1: none yet)
    bool lev_host = false;
    hipStream_t lev_stream = nullptr;
    std::string levels_route;    // how the last call with levels was served (fdc_pipeline_describe)
    // channel lag-1 correlation (fdc_pipeline_set_lag1): a setting, with the levels' state.  d_lag1: [max_blocks][C] (Re S, Im S) of the last call; pin_lag1
    // its pinned twin (lag_host, lag_stream as lev_host, lev_stream).  Both are allocated by the first call that switches the setting on.
    bool lag1_on = false;
    fdc::DevBuf<float2> d_lag1;
    fdc::PinBuf<float2> pin_lag1;
    int lag_blocks = -1;         // block count of the last successful work call with lag-1 on (-1: none yet)
    bool lag_host = false;
    hipStream_t lag_stream = nullptr;
    std::string lag1_route;      // how the last call with lag-1 was served (fdc_pipeline_describe)
    // channel gains (fdc_pipeline_set_gains): a setting like the three above.  gains_on: some gain is not exactly 1; gains: the C gains in force (empty
    // while off: all ones); d_gain their device table, allocated by the first call that switches the setting on and rewritten by every later one
    bool gains_on = false;
    std::vector<float> gains;
    fdc::DevBuf<float> d_gain;
    std::string gains_route;     // how the last call with gains was served (fdc_pipeline_describe)
    // channel demodulation (fdc_pipeline_set_demod): a setting like the ones above.  demod_mode: FDC_DEMOD_OFF / _FM / _MAG, demod_gain its factor.
    // d_carry: FM's stream state, the last complex float sample of every channel of the last demodulating call, two buffers of C: a call reads
    // d_carry[carry_cur] where it continues the stream (its first_block is demod_next; -1: the stream starts anew) and its kernel writes the other one;
    // the enqueue path swaps behind a successful enqueue.  Both, and the float staging d_out, are allocated by the first call that switches it on.
    int demod_mode = 0;
    float demod_gain = 1.f;
    fdc::DevBuf<float2> d_carry[2];
    int carry_cur = 0;
    int64_t demod_next = -1;
    std::string demod_route;     // which demodulation the last call with the setting on ran (fdc_pipeline_describe)
    // channel audio (fdc_pipeline_set_audio): a setting that needs the demodulation.  audio_decim: 0 = off; audio_taps: the K taps in force, d_ataps their
    // device copy; audio_row: A, the audio samples per block of all channels, d_aoff[c] channel c's first column.  d_ahist: the stream state, the K - 1
    // demodulated samples in front of the next call's first of every channel, two buffers of C (K - 1): a call reads d_ahist[ahist_cur] where it continues
    // the stream (its first_block is audio_next; -1: the stream starts anew) and its kernel writes the other one; the enqueue path swaps behind a
    // successful enqueue (FM's carry likewise).  d_audio: [max_blocks][A] elements of the last call (4 bytes each: the wider format), pin_audio its pinned
    // twin (aud_host, aud_stream as lev_host, lev_stream).  All of it is allocated by fdc_pipeline_set_audio, never on the enqueue path.
    int audio_decim = 0, audio_format = 0;
    float audio_scale = 1.f;
    std::vector<float> audio_taps;
    int64_t audio_row = 0;
    fdc::DevBuf<float> d_ataps, d_ahist[2];
    fdc::DevBuf<long long> d_aoff;
    int ahist_cur = 0;
    int64_t audio_next = -1;
    fdc::DevBuf<unsigned char> d_audio;
    fdc::PinBuf<unsigned char> pin_audio;
    int aud_blocks = -1;         // block count of the last successful work call with the audio on (-1: none yet)
    bool aud_host = false;
    hipStream_t aud_stream = nullptr;
    std::string audio_route;     // the last call with the setting on ran the audio pass (fdc_pipeline_describe)
    int64_t aud_first = -1;      // the absolute index of row 0 of that call's audio (fdc_pipeline_audio_first_block)
    // audio resampler (fdc_pipeline_set_audio_resampler): the other form of the channel audio, which replaces the decimating one and shares its format,
    // scale, columns (audio_row, d_aoff: W_c = ceil(lout_c up / down) per channel), histories (Kp - 1 per channel), audio_next, rows and their
    // bookkeeping.  rs_up: 0 = off; rs_taps: the prototype taps in force, rs_kp = ceil(ntaps / up) taps per phase, d_rstaps the table the kernel reads,
    // phase-major [up][Kp].  All of it is allocated by the setter, once per size.
    int rs_up = 0, rs_down = 0, rs_kp = 0;
    std::vector<float> rs_taps;
    fdc::DevBuf<float> d_rstaps;
    // channel squelch (fdc_pipeline_set_squelch): a setting that needs the levels.  sq_open / sq_close: the C thresholds in force, d_sqthr[0] / [1] their
    // device tables; sq_hang the hang count.  d_sqstate: the stream state, (open, h) of every channel behind the last call, two buffers of C int pairs: a
    // call reads d_sqstate[sqstate_cur] where it continues the stream (its first_block is squelch_next; -1: every channel starts closed) and its kernel
    // writes the other one; the enqueue path swaps behind a successful enqueue (the audio history likewise).  d_mask: [max_blocks][C] bytes of the last
    // call, pin_mask its pinned twin (sq_host, sq_stream as lev_host, lev_stream).  All of it is allocated by fdc_pipeline_set_squelch.
    bool squelch_on = false;
    std::vector<float> sq_open, sq_close;
    int sq_hang = 0;
    fdc::DevBuf<float> d_sqthr[2];
    fdc::DevBuf<int> d_sqstate[2];
    int sqstate_cur = 0;
    int64_t squelch_next = -1;
    fdc::DevBuf<unsigned char> d_mask;
    fdc::PinBuf<unsigned char> pin_mask;
    int sq_blocks = -1;          // block count of the last successful work call with the squelch on (-1: none yet)
    bool sq_host = false;
    hipStream_t sq_stream = nullptr;
    std::string squelch_route;   // the last call with the setting on ran the squelch pass (fdc_pipeline_describe)
    // packed audio (fdc_pipeline_set_audio_packing): a setting that needs the audio and the squelch.  d_packoff: the offsets of the last call's cells,
    // [max_blocks][C] words; d_packtotal: the running total of the call on the device (zeroed in front of a host call, read as the base and written
    // back by each of its sub-batches), pin_packtotal its pinned twin; pack_count: the elements of the last call's packed audio once they are known on
    // the host (aud_host).  The packed elements live in d_audio / pin_audio.  All of it is allocated by fdc_pipeline_set_audio_packing.
    bool pack_on = false;
    fdc::DevBuf<unsigned> d_packoff;
    fdc::DevBuf<long long> d_packtotal;
    fdc::PinBuf<long long> pin_packtotal;
    int64_t pack_count = 0;
    // channel tones (fdc_pipeline_set_tones): a setting that needs the demodulation.  tones_T: 0 = off, else the tones per channel; tones_S the group
    // length, tones_W the frame length in blocks; tones_inc the C T increments in force, d_tinc their device copy, d_ttab the reference table.  The stream
    // state: tones_fill, the blocks already inside the open frame, and d_tcarry, the open frame's accumulators, two buffers of C T: a call reads
    // d_tcarry[tcarry_cur] where it continues the stream (its first_block is tones_next; -1: the stream starts anew, fill 0) and its kernel writes the
    // other one; the enqueue path swaps behind a successful enqueue (the audio history likewise).  d_tones: the frame rows the last call completed,
    // [(max_blocks + W - 1) div W][C][T], pin_tones its pinned twin (tn_host, tn_stream as lev_host, lev_stream; tn_frames: how many rows).  All of it is
    // allocated by fdc_pipeline_set_tones, once per size.
    int tones_T = 0, tones_S = 0, tones_W = 0;
    std::vector<uint32_t> tones_inc;
    fdc::DevBuf<unsigned> d_tinc;
    fdc::DevBuf<float2> d_ttab, d_tcarry[2];
    int tcarry_cur = 0;
    int64_t tones_next = -1;
    int tones_fill = 0;
    fdc::DevBuf<float2> d_tones;
    fdc::PinBuf<float2> pin_tones;
    int tn_blocks = -1;          // block count of the last successful work call with the tones on (-1: none yet)
    int tn_frames = 0;           // ... and the frames it completed
    bool tn_host = false;
    hipStream_t tn_stream = nullptr;
    std::string tones_route;     // the last call with the setting on ran the tones pass (fdc_pipeline_describe)
    // tone squelch (fdc_pipeline_set_tone_squelch): a setting that needs the tones and the squelch.  tsq_tone: the C tone indices in force (-1: the channel
    // is not tone-gated), tsq_open / tsq_close / tsq_ratio the C thresholds and ratios, tsq_guard and tsq_hang (frames) for all channels; d_tsqtone and
    // d_tsqthr[0 .. 2] their device tables.  d_tsqstate: the stream state, (open, h) of every channel behind the last completed frame, two buffers of C
    // int pairs: a call reads d_tsqstate[tsqstate_cur] where it continues the TONES' stream and the state is valid (tsq_valid: a call with the setting in
    // force has written it) and its kernel writes the other one; the enqueue path swaps behind a successful enqueue.  d_tdec: the decisions of the frames
    // the last call completed, [(max_blocks + W - 1) div W][C] bytes, pin_tdec its pinned twin (tsq_host, tsq_stream as lev_host, lev_stream; tsq_frames:
    // how many rows).  All of it is allocated by fdc_pipeline_set_tone_squelch.
    bool tsq_on = false;
    std::vector<int32_t> tsq_tone;
    std::vector<float> tsq_open, tsq_close, tsq_ratio;
    int tsq_guard = 0, tsq_hang = 0;
    fdc::DevBuf<int> d_tsqtone;
    fdc::DevBuf<float> d_tsqthr[3];
    fdc::DevBuf<int> d_tsqstate[2];
    int tsqstate_cur = 0;
    bool tsq_valid = false;
    fdc::DevBuf<unsigned char> d_tdec;
    fdc::PinBuf<unsigned char> pin_tdec;
    int tsq_blocks = -1;         // block count of the last successful work call with the tone squelch on (-1: none yet)
    int tsq_frames = 0;          // ... and the frames it decided
    bool tsq_host = false;
    hipStream_t tsq_stream = nullptr;
    std::string tsq_route;       // the last call with the setting on ran the tone squelch (fdc_pipeline_describe)
    fdc::DevBuf<float2> d_out;   // work(): max_blocks*sum_lout (out_staging)
    int64_t blockcount = 0;      // work(): blocks consumed so far
    // work(): transfers and kernels of consecutive sub-batches overlap (H2D on s_in, kernels on stream, D2H on s_out)
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    fdc::PinBuf<float2> pin_out[2];                                              // staging for unregistered output buffers
    fdc::MappedBuf<fdc::ScatterEnt> pin_tab;                                     // registered outputs: scatter table, pinned and device-mapped ...
    fdc::ScatterEnt *d_tab = nullptr;                                            // ... and its device-side address (an alias: pin_tab owns the memory)
    int sub = 0;                 // blocks per sub-batch
    // fdc_pipeline_work_sinks on a look-ahead bank (the pipelined hier block): the batch of the last call sits transformed in the bank's
    // next-batch buffer and is submitted by the NEXT call, beside that call's input copy and forward transform
    int hier_filled = 0;         // its block count (0 = none)
    fdc_sinks *hier_bank = nullptr;
    hipEvent_t ev_hier = nullptr;   // on the bank's fill stream behind the last call's transform and history copy: the ring may be overwritten
    bool hier_ring_busy = false;
    bool hier_broken = false;    // a pipelined call failed after it had advanced the stream state: the pair of handles cannot go on (see work_sinks_pipelined)
    bool reserve_user = false;   // fdc_pipeline_reserve_compute_units was called with n > 0: the pipelined entry takes that reservation, not its own
    std::string wf_route;        // the route of the last waterfall call (fdc_pipeline_describe)
    int gpow_src = 0;            // who summed the 16-bin group powers of the last waterfall call: bit 0 the block kernel's epilogue, bit 1 k_group_power
    bool cfg_generic = false;    // FDC_FORCE_GENERIC=1: bypass the size-specialised kernels (A/B testing)
    // timing
    bool timing = false;
    int timing_stride = 1;       // events on every stride-th launch group (fdc_pipeline_enable_timing(p, stride))
    long long timing_seq = 0;
    std::vector<hipEvent_t> events;
    size_t ev_used = 0;
    std::vector<std::array<size_t, 5>> ev_spans;   // events: start, mid, end-of-fft, end-of-channels; [4]: which form the span ran (kSpan*)
};

namespace fdc { namespace pipe {

// One launch group of a call: blocks [m0, m0 + nb) of the call's nblocks; first_block: the stream's index of the call's block 0.  The kernels place
// the group's samples in the CALL's output by m0 and nblocks.
struct Span { int nb, m0, nblocks; int64_t first_block; };

// What one call brings to the enqueue path: the entry fills it (device_call), everything below process_device_impl reads it, and the two results come
// back in it.  Nothing per call is parked on the handle, so no call can leave anything behind for the next.  Plain members: making one allocates nothing.
struct DeviceCall {
    // input form.  fmt: 0 = float2 ring; FDC_IQ_SC16 / FDC_IQ_SC8: a ring of complex integers (scale: their factor), and `wide` the float2 buffer of
    // chunk*H + ovl samples a launch group is widened into where the kernels take float input
    int fmt = 0; float scale = 1.0f; float2 *wide = nullptr;
    // output form.  ofmt: 0 = complex float into d_out; FDC_OQ_SC16 / FDC_OQ_SC8 (times oscale): narrow samples into d_out (same offsets).  Kernels that do not
    // narrow themselves (oq_fused) write float into fout (nblocks*sum_lout samples); k_complex_to_iq narrows it into d_out unless narrow is false (the caller does)
    // Channel demodulation (fdc_pipeline_set_demod) rides ofmt as two private codes of 4 bytes per sample, kOqDemod + FDC_DEMOD_FM / _MAG, with its gain in
    // oscale: never fused (the kernels write float into fout) and never left to the caller (narrow stays true): k_chan_demod is the call's tail
    int ofmt = 0; float oscale = 1.0f; float2 *fout = nullptr; bool narrow = true;
    hipStream_t stream = nullptr;        // every launch of the call
    void *spectrum = nullptr;            // the caller's spectrum buffer for the blocks of this invocation, or none
    bool own_spectrum = false;           // `spectrum` is the entry's own staging (waterfall): allowed without keep_spectrum
    // group powers (fdc_pipeline_process_device_power): the 16-bin group sums of the block whose spectrum starts at gpow_origin + k N go to gpow + k N / 16
    float *gpow = nullptr; const float2 *gpow_origin = nullptr;
    // waterfall rows (path 5: the fused kernel's epilogue): the row sums of the stream's block b go to rows + (b - rows_first) * 1024
    float *rows = nullptr; int64_t rows_first = 0;
    // channel levels (fdc_pipeline_set_levels): where (power, peak) of the call's block 0, channel 0 go, [block][C]; null = none.  With them the kernels
    // write float whatever the output format (the order of the passes: fdc_enqueue.hip, float_passes)
    float2 *levels = nullptr;
    // channel lag-1 correlation (fdc_pipeline_set_lag1): where (Re S, Im S) of the call's block 0, channel 0 go, [block][C]; null = none.  As with levels
    // the kernels write float whatever the output format
    float2 *lag1 = nullptr;
    // channel gains (fdc_pipeline_set_gains): the handle's device table of C gains, null = off (device_call).  With them the kernels write float whatever
    // the output format, as with levels
    const float *gain = nullptr;
    // channel audio (fdc_pipeline_set_audio): where row 0 of the call's audio goes, [block][A] elements of the setting's format; null = none.  It
    // goes with a demodulating output code only
    void *audio = nullptr;
    // channel squelch (fdc_pipeline_set_squelch): where the mask byte of the call's block 0, channel 0 goes, [block][C]; null = none.  It goes with levels
    unsigned char *squelch = nullptr;
    // packed audio (fdc_pipeline_set_audio_packing): where the offsets of the call's block 0 go, [block][C] words; null = none.  It goes with audio and
    // squelch; `audio` is then element 0 of the packed buffer whichever block the call starts at, the offsets start at the handle's running total where
    // pack_append says so (a sub-batch behind the first of a host call) and at 0 otherwise, and the total goes to the handle's device word
    unsigned *pack_off = nullptr;
    bool pack_append = false;
    // channel tones (fdc_pipeline_set_tones): where the first frame row the call completes goes, [frame][C][T]; null = none.  It goes with a demodulating
    // output code only.  A sub-batch of a host call hands in the row behind the frames the host call has completed so far (tones_frames, below)
    float2 *tones = nullptr;
    // tone squelch (fdc_pipeline_set_tone_squelch): where the decisions of the first frame the call completes go, [frame][C] bytes; null = none.  It goes
    // with tones and squelch; a sub-batch of a host call hands in the row behind the frames the host call has completed so far, as for the tones
    unsigned char *tone_dec = nullptr;
    int ncu = 0;                       // compute units the call's persistent kernels may use
    // results: no launch group had to be widened (each read the integer input in its own loads); the call's kernels narrowed in their own stores;
    // the frame rows the tones pass of the call completed
    bool all_fused = true, ofused = false;
    int tones_frames = 0;
};

// which form a timed launch group ran (ev_spans[.][4]): how the three intervals between its four events map to ms[0..2]
enum { kSpanBanks = 0 /* banks | remainder forward | remainder channels */, kSpanTwoLaunch = 1 /* stage 1 | - | stage 2 (+ remainder) */,
       kSpanSpectrumLds = 2 /* forward transform = a + b | channels */, kSpanSpectrum = 3 /* pass A / block forward | pass B | channels */ };

// the private output codes of channel demodulation (DeviceCall::ofmt), and the bytes per sample of any output code
constexpr int kOqDemod = 16;
inline bool oq_demod(int ofmt) { return ofmt > kOqDemod; }
inline size_t oq_bytes(int ofmt) { return oq_demod(ofmt) ? sizeof(float) : fdc::iq_bytes(ofmt); }
// the output code of the handle's next call: demodulation while it is on (it excludes integer output; a plan without channels has nothing to
// demodulate), else the output format
inline int out_code(const fdc_pipeline *p) { return p->demod_mode && p->C > 0 ? kOqDemod + p->demod_mode : p->out_form; }

// channel audio: whether the handle's next call runs the pass, and the bytes of one audio element
inline bool audio_set(const fdc_pipeline *p) { return p->audio_decim > 0 || p->rs_up > 0; }     // either form of the audio is switched on
inline bool audio_on(const fdc_pipeline *p) { return audio_set(p) && p->demod_mode && p->C > 0; }
inline size_t audio_bytes(const fdc_pipeline *p) { return p->audio_format == FDC_AUDIO_S16 ? sizeof(int16_t) : sizeof(float); }
// ... and where the rows from block b0 of a host call on go in the handle's buffer
inline void *audio_rows(const fdc_pipeline *p, size_t b0) { return audio_on(p) ? p->d_audio.get() + audio_bytes(p) * b0 * (size_t)p->audio_row : nullptr; }

// channel squelch: where the mask rows from block b0 of a host call on go in the handle's buffer (null: the call runs no squelch pass)
inline unsigned char *squelch_rows(const fdc_pipeline *p, size_t b0)
{
    return p->squelch_on && p->levels_on && p->C > 0 ? p->d_mask.get() + b0 * (size_t)p->C : nullptr;
}

// packed audio: whether the handle's next call packs its audio, and where the offsets rows from block b0 of a host call on go (null: it does not)
inline bool packing_on(const fdc_pipeline *p) { return p->pack_on && audio_on(p) && squelch_rows(p, 0); }
inline unsigned *pack_rows(const fdc_pipeline *p, size_t b0) { return packing_on(p) ? p->d_packoff.get() + b0 * (size_t)p->C : nullptr; }

// channel tones: whether the handle's next call runs the pass, the elements of one frame row, and where the row behind `done` completed frames of a
// host call goes in the handle's buffer (null: the call runs no tones pass)
inline bool tones_on(const fdc_pipeline *p) { return p->tones_T > 0 && p->demod_mode && p->C > 0; }
inline size_t tones_row(const fdc_pipeline *p) { return (size_t)p->C * (size_t)p->tones_T; }
inline float2 *tones_rows(const fdc_pipeline *p, size_t done) { return tones_on(p) ? p->d_tones.get() + done * tones_row(p) : nullptr; }

// tone squelch: where the decisions behind `done` completed frames of a host call go in the handle's buffer (null: the call runs no tone squelch)
inline unsigned char *tone_dec_rows(const fdc_pipeline *p, size_t done)
{
    return p->tsq_on && tones_on(p) && squelch_rows(p, 0) ? p->d_tdec.get() + done * (size_t)p->C : nullptr;
}

inline bool ispow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

inline float2 unit(double turns)              // exp(-2 pi i turns), designed in double, rounded once
{
    const double a = -2.0 * M_PI * turns;
    return make_float2(float(std::cos(a)), float(std::sin(a)));
}

// the two-launch form (stage 1 + stage 2 through the scratch G) exists for a plan that is ONE bank on its grid, no copied channels
inline bool two_launch_possible(const fdc_pipeline *p)
{
    return p->poly_ok && p->banks.size() == 1 && p->banks[0].r == 0 && p->bank_alias.empty();
}

// ---- fdc_api.hip
std::vector<float2> make_twiddles(int n);     // exp(-2 pi i k / n) designed in double, rounded once
bool host_registered(const void *ptr, size_t bytes, void **devptr = nullptr);   // inside a range pinned with fdc_host_register (devptr: its device address)
int out_staging(fdc_pipeline *p);             // d_out, max_blocks*sum_lout samples, at the first call that needs it (the handle's device is current)

// ---- fdc_plan.hip: the steps of fdc_pipeline_create (1 - 3 are fdc_pipeline_plan_preview's too: host code only)
int validate_cfg(const fdc_pipeline_cfg *cfg);
int effective_flags(int flags);
void build_channel_records(fdc_pipeline *p, const fdc_pipeline_cfg *cfg, std::vector<std::complex<float>> &pool);
void group_by_width(const fdc_pipeline *p, const std::vector<int> *ids, std::vector<std::pair<int, std::vector<int32_t>>> &groups,
                    std::vector<size_t> &off, std::vector<char> &al, std::vector<char> &oal, std::vector<int32_t> &flat);
void classify_plan(fdc_pipeline *p, const fdc_pipeline_cfg *cfg, int flags);
int build_device_state(fdc_pipeline *p, const fdc_pipeline_cfg *cfg, const std::vector<std::complex<float>> &pool,
                       const std::vector<int32_t> &flat, const std::vector<int32_t> &rflat);

// ---- fdc_enqueue.hip
DeviceCall device_call(const fdc_pipeline *p, void *stream, void *d_spectrum, int fmt = 0, float scale = 1.0f);
int process_device_impl(fdc_pipeline *p, DeviceCall &call, const void *d_ring, int64_t first_block, int nblocks, void *d_out);
int channels_wide(fdc_pipeline *p, const float2 *spec, float2 *d_out, const int32_t *d_gids, int ngroup, int l, const Span &span, hipStream_t s);
int check_iq_form(int32_t format, float scale);
void levels_written(fdc_pipeline *p, int nblocks, hipStream_t stream, bool host);   // a call with levels on succeeded: what fdc_pipeline_levels hands out
void lag1_written(fdc_pipeline *p, int nblocks, hipStream_t stream, bool host);     // the same of the lag-1 correlation (fdc_pipeline_lag1)
void audio_written(fdc_pipeline *p, int64_t first_block, int nblocks, hipStream_t stream, bool host);    // ... and of the channel audio (fdc_pipeline_audio)
void squelch_written(fdc_pipeline *p, int nblocks, hipStream_t stream, bool host);  // ... and of the channel squelch (fdc_pipeline_squelch)
void tones_written(fdc_pipeline *p, int nblocks, int nframes, hipStream_t stream, bool host);   // ... and of the channel tones (fdc_pipeline_tones)
void tone_squelch_written(fdc_pipeline *p, int nblocks, int nframes, hipStream_t stream, bool host);   // ... and of the tone squelch (fdc_pipeline_tone_squelch)
std::string route(int fmt, bool fused, const char *otherwise);   // "<sc16|sc8>: fused", or what the call was instead (fdc_pipeline_describe)

} }  // namespace fdc::pipe
