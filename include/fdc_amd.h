/* fdc_amd.h — C-ABI of the MI355X (gfx950) frequency-domain channelizer.
 *
 * Drop-in boundary for the ONE hot path of gereonsuch/gr-FDC: overlap-save -> large forward FFT ->
 * per-channel vector cut / phase-shifting window -> per-channel inverse FFT -> overlap discard.
 * Plain pointers and sizes only; no C++ types, no exceptions, no torch types.  Every entry point names
 * the reference interface it replaces (paths relative to the reference tree).  How the reference's
 * blocks bind to these functions (C++ sync_block::work() bodies, ctypes stub) is in INTEGRATION.md.
 *
 * Conventions
 *  - samples are complex float32, interleaved (re, im): GNU Radio's gr_complex;
 *  - every function returns FDC_OK (0) or a negative fdc_status; fdc_last_error() gives the text;
 *  - a handle is used by one thread at a time (GNU Radio calls work() of one block instance from
 *    one thread); distinct handles may be used concurrently;
 *  - host pointers passed to *_work() are not retained after the call returns
 *    (the runtime owns them only for the duration of work(): lib/overlap_save_impl.cc:62-81).
 */
#ifndef FDC_AMD_H
#define FDC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FDC_OK = 0,
    FDC_ERR_INVALID_ARGUMENT = -1, /* the predicates on which the reference ctors throw std::invalid_argument */
    FDC_ERR_HIP = -2,              /* a HIP runtime call failed */
    FDC_ERR_NO_DEVICE = -3,        /* no gfx950 device visible: the product path never falls back to the CPU */
    FDC_ERR_UNSUPPORTED = -4,
    FDC_ERR_NOMEM = -5
} fdc_status;

/* window shapes: lib/windows.h:28-32 */
enum { FDC_WIN_RECTANGULAR = 0, FDC_WIN_HANN = 1, FDC_WIN_RAMP = 2 };

const char *fdc_last_error(void);            /* thread-local text of the last failure */
/* No C++ exception leaves the library: every entry that can allocate on the host (std::vector, std::thread, new) runs behind one
 * barrier that turns std::bad_alloc / std::system_error into FDC_ERR_NOMEM and anything else into FDC_ERR_HIP (csrc/fdc_guard.hpp).
 * This entry throws each kind through that same barrier and returns FDC_OK when every one came back as the status it should
 * (needs no device; tests/test_abi_cpu.py). */
int fdc_selftest_exception_barrier(void);
const char *fdc_version(void);
int fdc_device_count(void);                  /* number of visible HIP devices (0 if none) */
/* Runs the headline geometry (65536-point blocks, R = 2, 256 channels of 256 bins, 96 blocks: the one-kernel path) through
 * fdc_pipeline_work() on EVERY visible device and compares a checksum of all output samples with device 0's (same kernels,
 * same input: the bytes must be identical), then once more through ONE multi-device handle over all visible devices
 * (fdc_pipeline_group below; with one device: two virtual members on it), the call cut in two so that the group's history is
 * used: again device 0's bytes.  Returns the number of devices verified, or a negative fdc_status with the device and the
 * mismatch in fdc_last_error().  A multi-GPU launcher calls it once before sharding block spans over the devices (the kernel
 * attributes are set per device: this is what exercises device_id > 0, and the group's worker threads on real peers). */
int fdc_selftest_devices(void);

/* ------------------------------------------------------------------------------------------------
 * Fused throughput pipeline = the chain python/FrequencyDomainChannelizer.py:200-231 wires:
 *   stream_to_vector -> overlap_save (lib/overlap_save_impl.cc:62-81) -> fft_vcc(N, fwd, shift) (:206)
 *   -> multiply_const_cc(1/N) (:214-216) -> per channel { vector_cut_vxx (lib/vector_cut_vxx_impl.cc:59-72)
 *   -> phase_shifting_windowing_vcc (lib/phase_shifting_windowing_vcc_impl.cc:72-86) -> fft_vcc(l, inv, shift)
 *   (:228) -> vector_cut_vxx(l, l-lout, lout) (:229) -> vector_to_stream (:230) -> multiply_const_cc(l) (:231) }.
 * The spectrum stays in HBM; only input samples and channel outputs cross the boundary.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fdc_pipeline fdc_pipeline;

typedef struct {
    int32_t f;        /* first bin of the slice in the fftshifted spectrum (vector_cut_vxx offset) */
    int32_t l;        /* slice / inverse-FFT length, power of two (vector_cut_vxx blocklen)          */
    float passbw;     /* phase_shifting_windowing_vcc::make passbw                                   */
    float stopbw;     /* phase_shifting_windowing_vcc::make stopbw                                   */
} fdc_channel;

typedef struct {
    int32_t device_id;      /* HIP device ordinal */
    int32_t blocklen;       /* N, power of two (hier block "blocksize", py:138)                      */
    int32_t relinvovl;      /* R, power of two >= 2 (py:139); overlap = N/R                           */
    int32_t windowtype;     /* FDC_WIN_* (hier block "windowtype", py:227)                            */
    int32_t nchannels;
    const fdc_channel *channels;
    int32_t max_blocks;     /* largest nblocks a single work()/process call will carry; max_blocks x (sum of the channels' kept
                               samples per block) x 8 bytes must stay below 4 GiB (32-bit output offsets inside one call):
                               FDC_ERR_INVALID_ARGUMENT otherwise                                    */
    int32_t chunk_blocks;   /* blocks per internal launch group (0 = as many as a 2 GiB scratch budget
                               allows: long launches measured faster than cache-sized ones)          */
    int32_t keep_spectrum;  /* != 0: keep the whole normalised spectrum of a call (debug port, py:314) */
    int32_t flags;          /* FDC_PIPE_* bits, 0 = the library picks the fastest kernels for the plan            */
    int32_t min_block_launch; /* launch groups of fewer blocks than this do not take the one-block-per-compute-unit
                               kernels (0 = default 96: such a kernel gives a whole block to ONE compute unit, so a short
                               call would leave most of the device idle; 1 = always take them)                  */
    int32_t host_sub_blocks;  /* fdc_pipeline_work(): blocks per sub-batch whose transfers and kernels overlap (0 = about
                               8 MiB of input)                                                                */
} fdc_pipeline_cfg;
/* fdc_pipeline_cfg.flags: restrict the choice of kernels (A/B measurements, tests of the slower forms; results are the same
 * to rounding).  The library reads NO environment variable unless FDC_DEBUG_ENV=1 is set, and then only as a debugging
 * override of these fields (FDC_FORCE_GENERIC, FDC_NO_POLY, FDC_NO_BLOCK, FDC_BLOCK_HINTS, FDC_BLOCK_MIN_BLOCKS,
 * FDC_HOST_SUB, FDC_SINKS_THREADS, FDC_SINKS_TRACE, and the tile knobs of the two-launch kernels). */
enum {
    FDC_PIPE_FORCE_GENERIC = 1,   /* generic LDS Stockham kernels only                                              */
    FDC_PIPE_NO_POLY = 2,         /* no uniform-plan commutation: forward transform to a spectrum in memory + channel kernels */
    FDC_PIPE_NO_BLOCK = 4,        /* no one-block-per-compute-unit kernels (two-launch uniform path / two-pass transform)   */
    FDC_PIPE_PLAIN_STORES = 8,    /* block kernels: ordinary instead of streamed (nt) output stores                 */
    FDC_PIPE_NT_LOADS = 16,       /* block kernels: streamed (nt) input loads (not the 512- / 1024-bin kernels, which stage their loads) */
    FDC_PIPE_FULL_SPECTRUM = 32,  /* the handle's internal spectrum is written in full (default: only the 64-bin groups some channel reads) */
    FDC_PIPE_NO_FUSED = 128,      /* N = 4096: not the one-launch kernel that keeps the spectrum in LDS (A/B, tests); also off under FDC_PIPE_NO_POLY */
    FDC_PIPE_WIDE_UNIFORM = 64    /* uniform banks of ANY channel width (every channel l = L on the L-bin grid, one window) take the form without
                                     a spectrum: the width's block kernel where there is one (N = 16384 / 32768 / 65536: l = 64, 128, 256, 512, 1024), else two
                                     launches on generic kernels; default: only where that measured faster than the spectrum path (the block
                                     kernels; what the cost rule of csrc/fdc_plan_cost.hpp sends there: l = 1024 from 3 channels up) */
};

int fdc_pipeline_create(const fdc_pipeline_cfg *cfg, fdc_pipeline **out);
void fdc_pipeline_destroy(fdc_pipeline *p);

/* sizes derived from the configuration */
int64_t fdc_pipeline_input_samples(const fdc_pipeline *p, int nblocks);   /* nblocks*(N-N/R)            */
int64_t fdc_pipeline_output_samples(const fdc_pipeline *p, int nblocks);  /* nblocks*sum_c lout_c       */
int64_t fdc_pipeline_channel_offset(const fdc_pipeline *p, int channel, int nblocks); /* in d_out, samples */
int32_t fdc_pipeline_channel_lout(const fdc_pipeline *p, int channel);

/* work()-shaped entry: host buffers, stateful like the block chain (overlap history + window counters
 * persist across calls; lib/overlap_save_impl.h:33, lib/phase_shifting_windowing_vcc_impl.h:47).
 *   in          nblocks*(N-N/R) new samples (what stream_to_vector hands overlap_save)
 *   outs[c]     nblocks*lout_c samples for channel c (hier output port c), in the handle's output format (fdc_pipeline_set_output_format below:
 *               complex float unless it was set to sc16 / sc8; the same for every work, span, real, iq and device entry that names it)
 *   spectrum    NULL, or nblocks*N samples of the normalised spectrum (needs keep_spectrum)
 * Returns nblocks (items consumed, sync 1:1) or a negative fdc_status. */
int fdc_pipeline_work(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum);
/* The same for a REAL input stream (float32 items, the hier block's "Float" input type: stream_to_vector(4, ...),
 * overlap_save(4, ...) and the fft_vfc the reference meant to put at python/FrequencyDomainChannelizer.py:207-208 — the branch
 * is unreachable there, :205-210): in = nblocks*(N-N/R) float32 samples, taken as the real part of the block; everything
 * behind the load is the complex path unchanged (fftshift, 1/N, channels).  History and block counter are shared with
 * fdc_pipeline_work; do not mix the two on one handle. */
int fdc_pipeline_work_real(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum);

/* One contiguous SPAN of a longer stream, handed over by a dispatcher that cuts a work() call over several handles (the
 * members of an fdc_pipeline_group below; a user-written scheduler may call it directly).  Same as fdc_pipeline_work() except
 * that the two pieces of stream state come from the caller instead of from the handle:
 *   halo         the N/R samples in front of the span (the tail of the previous span; lib/overlap_save_impl.cc:62-81), or NULL
 *                for zeros (stream start, :52)
 *   first_block  global index of the span's first block (window phase = first_block*shift mod R,
 *                lib/phase_shifting_windowing_vcc_impl.cc:82)
 * Afterwards the handle's own state is that of a stream that ended with this span (a following fdc_pipeline_work() continues it).
 * _real: float32 samples, halo included (see fdc_pipeline_work_real). */
int fdc_pipeline_work_span(fdc_pipeline *p, const void *halo, const void *in, int64_t first_block, int nblocks, void *const *outs,
                           void *spectrum);
int fdc_pipeline_work_span_real(fdc_pipeline *p, const void *halo, const void *in, int64_t first_block, int nblocks, void *const *outs,
                                void *spectrum);

/* Complex INTEGER input, as radio front ends deliver it (UHD sc16 / sc8, RFSoC and ADC capture cards: interleaved int16 or int8 I/Q).
 * Sample k is (float(I_k) * scale, float(Q_k) * scale): the conversion is exact, the product rounded once in float32 (numpy's
 * np.float32(I) * np.float32(scale)), and everything behind it is the complex path, so the outputs are bit-identical to
 * fdc_pipeline_work / _span / process_device on the converted complex64 input, for any finite scale.  UHD sc16 -> fc32 is scale = 1/32768;
 * GNU Radio's interleaved_short_to_complex has scale 1.
 *   format   FDC_IQ_SC16 (4 bytes per sample) or FDC_IQ_SC8 (2 bytes per sample); anything else, or a scale that is zero or not finite:
 *            FDC_ERR_INVALID_ARGUMENT
 *   in, halo the same sample counts as the float entries, in the format (halo: N/R samples); a registered `in` is DMA'd in place
 * Input form: the first work call after create / fdc_pipeline_reset latches the handle to (format, scale), or to float input (fdc_pipeline_work,
 * _span, _real, ...).  A call in another form returns FDC_ERR_INVALID_ARGUMENT and changes nothing; the next call in the right form continues
 * the stream.  The overlap history of integer calls is kept in the integer format.  Path 5 (N = 4096 in one launch) and the banks of 256-bin
 * channels at N = 16384 / 32768 / 65536 read the integers in their own loads; every other plan widens them on the device first
 * (fdc_pipeline_describe names which: "input sc16: fused" / "input sc16: widened").  The integer ring (and any staging) is allocated at the
 * first integer call; nothing is allocated in the steady state.  Out of scope: the sink and waterfall entries take float input only. */
enum { FDC_IQ_SC16 = 1,   /* int16 I, int16 Q interleaved: 4 bytes per sample */
       FDC_IQ_SC8  = 2 }; /* int8  I, int8  Q interleaved: 2 bytes per sample */
int fdc_pipeline_work_iq(fdc_pipeline *p, int32_t format, float scale, const void *in, int nblocks, void *const *outs, void *spectrum);
int fdc_pipeline_work_span_iq(fdc_pipeline *p, int32_t format, float scale, const void *halo, const void *in, int64_t first_block, int nblocks,
                              void *const *outs, void *spectrum);

/* Complex INTEGER output (the other half of the integer I/O: recorders, network sinks and fixed-point demodulators behind an SDR front end want the
 * channel streams back as sc16 / sc8).  A SETTING of the handle, not a latch: it may be changed between any two calls and applies from the next one; it
 * does not touch the history, the block counter or the input-form latch, and survives fdc_pipeline_reset.
 *   format   FDC_OQ_FC32 (default: complex float32, 8 bytes per sample), FDC_OQ_SC16 (int16 I, int16 Q interleaved: 4 bytes) or FDC_OQ_SC8 (int8: 2 bytes)
 *   scale    float32; zero or not finite: FDC_ERR_INVALID_ARGUMENT (negative is allowed).  UHD's sc16 convention is scale = 32768.
 * Each component of a channel sample y (exactly what the float entries write) becomes saturate(round_half_even(float32(y * scale))), the product rounded
 * once and kept out of FMA contraction; NaN -> 0, +Inf -> the maximum, -Inf -> the minimum; saturation to [-32768, 32767] / [-128, 127].
 * While it is set, outs[c] (host) or d_out (device) of fdc_pipeline_work, _work_real, _work_span, _work_span_real, _work_iq, _work_span_iq,
 * _process_device, _process_device_iq and the group's work entries hold nblocks*lout_c samples OF THAT FORMAT (sample counts, offsets and lout are
 * unchanged; the max_blocks rule stays computed at 8 bytes).  The debug spectrum stays complex float.  The entries that write complex float only —
 * fdc_pipeline_work_sinks, _flush_sinks, _work_spectrum, _process_device_power, fdc_pipeline_work_waterfall — return FDC_ERR_INVALID_ARGUMENT and change
 * nothing while it is not FC32.  Refused (FDC_ERR_INVALID_ARGUMENT) while a pipelined sinks batch is inside the handle (flush it first).
 * Path 5 and the banks of 256-bin channels at N = 16384 / 32768 / 65536 (streamed stores) narrow in their kernels' own stores; every other plan narrows
 * the complex float results on the device (fdc_pipeline_describe: "output sc16: fused" / "output sc16: narrowed").  The float staging of the narrowed
 * route (max_blocks*sum_lout samples) is allocated by the first call that sets sc16 / sc8, the host entries' narrow staging at their first integer-output
 * call; nothing in the steady state, nothing inside a device entry.  A device call that is narrowed needs nblocks <= max_blocks. */
enum { FDC_OQ_FC32 = 0,   /* complex float32 (the default) */
       FDC_OQ_SC16 = 1,   /* = FDC_IQ_SC16 */
       FDC_OQ_SC8  = 2 }; /* = FDC_IQ_SC8 */
int fdc_pipeline_set_output_format(fdc_pipeline *p, int32_t format, float scale);

/* FINE TUNING: centre each channel on its requested frequency.  A channel's slice is cut at whole bins, so its stream carries the signal at a residual
 * offset of up to half a bin of N (more for slices wrapped or clamped at a band edge).  With a fine-tuning frequency nu_c for channel c, in cycles per
 * OUTPUT sample of that channel, |nu_c| < 0.5, sample t of the channel's stream becomes
 *     y'_c[t] = y_c[t] * exp(-2 pi i phi_c(t)),   phi_c(t) = ((inc_c * t) mod 2^64) / 2^64,   inc_c = round_half_even(nu_c * 2^64) mod 2^64
 * where y_c[t] is exactly what the entry writes without it and t = (global block index) * lout_c + j is the stream's own sample index (the block index:
 * the handle's block counter, or first_block of the span and device entries).  The phase is an INTEGER function of t (a 64-bit wrapping product): no
 * drift, no accumulated rounding, no dependence on how the stream is cut into calls, launch groups or spans.
 *   fdc_fine_tuning_increment   inc for one nu (host only, no device); NaN and |nu| >= 0.5: FDC_ERR_INVALID_ARGUMENT
 *   fdc_pipeline_set_fine_tuning   nu[n], n = the channel count (else FDC_ERR_INVALID_ARGUMENT; so is any nu the function above refuses: nothing changes);
 *                               nu = NULL or all zeros switches it off
 * A SETTING like fdc_pipeline_set_output_format: it may change between any two calls and applies from the next one; it does not touch the history, the
 * block counter or the input-form latch, and survives fdc_pipeline_reset; refused while a pipelined sinks batch is inside the handle.  Every table it
 * needs is allocated (once) and written here, nothing in a work call; the call waits for the handle's own stream first (device entries on another
 * stream: the caller orders them).  While it is on, the channel outputs of fdc_pipeline_work, _work_span, _work_real, _work_span_real, _work_iq,
 * _work_span_iq, _process_device, _process_device_iq and the group's work entries are y'; with integer output the turn comes BEFORE the narrowing:
 * oq(y' * scale).  The debug spectrum is unchanged.  fdc_pipeline_work_sinks, _work_spectrum, _process_device_power and fdc_pipeline_work_waterfall return
 * FDC_ERR_INVALID_ARGUMENT and change nothing while it is on.  Per sample the device multiplies y * base * step in float32, in this order and without
 * FMA contraction: base = the phasor of phi_c(block * lout_c), computed once per (block, channel), step = a per-channel table of lout_c phasors designed
 * in double; |y' - y w| <= 11 * 2^-24 |y| against the exact phasor w.  Path 5 turns the samples in its kernel's own stores
 * (fdc_pipeline_describe: "fine tuning: fused"), every other plan in one pass over the launch group's results ("fine tuning: rotated"). */
int fdc_fine_tuning_increment(double nu, uint64_t *inc);
int fdc_pipeline_set_fine_tuning(fdc_pipeline *p, const double *nu, int n);

/* CHANNEL LEVELS: per-block power and peak of every channel, summed on the device (meters, squelch, occupancy, an AGC that sets the next call's channel
 * gains, CHANNEL GAINS below — without pulling the float streams over the link).  With levels on, every (block m of the call, channel c) gets two float32 values from the
 * lout_c samples the call produces for it:
 *     power[m][c] = sum_j (re_j^2 + im_j^2)        peak[m][c] = max_j max(|re_j|, |im_j|)   (fmax: a NaN component is passed over)
 * of the complex float32 samples y' the entry writes, or would write before narrowing: AFTER fine tuning, BEFORE the sc16 / sc8 narrowing.  So
 * peak * |scale| >= 32767.5 (sc16) or >= 127.5 (sc8) means some component of that row saturated in the narrowing.  Layout: levels[m][c] = (power, peak),
 * float[nblocks][C][2], c the plan's channel index (a channel that is a copy of another channel's slice has its own entry).  Rows with samples that are
 * not finite give what IEEE arithmetic and fmax give; nothing traps and no other row is disturbed.  The bits of power[m][c] depend on lout_c and the
 * row's sample values only (one lane assignment and one summation tree per lout, no FMA contraction, no atomics): not on the row's address, not on how
 * the stream is cut into calls, sub-batches, launch groups or spans, not on which kernel summed it.  |power - P| <= (lout_c + 8) 2^-24 P against the exact
 * sum of squares P of the float32 samples; peak is exact.
 *   fdc_pipeline_set_levels      on != 0 / 0.  A SETTING like fdc_pipeline_set_output_format and fdc_pipeline_set_fine_tuning: it may change between any
 *                                two calls and applies from the next one; it does not touch the history, the block counter or the input-form latch, and
 *                                survives fdc_pipeline_reset; refused while a pipelined sinks batch is inside the handle; it waits for the handle's own
 *                                stream first.  The first call that switches it on allocates everything the feature needs, once (max_blocks*C pairs on
 *                                the device and pinned on the host); nothing in a work call, nothing inside a device entry.  With C = 0, on is accepted
 *                                and every result is empty.
 *   fdc_pipeline_levels          the levels of the last successful work call (host or device entry; a device entry's are read after a synchronise of
 *                                the stream it ran on): dst receives nblocks*C*2 floats.  nblocks must be that call's block count, otherwise
 *                                FDC_ERR_INVALID_ARGUMENT; the same while levels are off and before any call.  A call of 0 blocks leaves the previous
 *                                result in place.
 *   fdc_pipeline_levels_device   the device buffer ([block of the call][C] float2), NULL while off: for callers of fdc_pipeline_process_device /
 *                                _process_device_iq, who read it ordered on their own stream.  While levels are on, a device call needs
 *                                nblocks <= max_blocks (the rule of a narrowed device call): above it FDC_ERR_INVALID_ARGUMENT, nothing enqueued.
 * While levels are on, fdc_pipeline_work_sinks, _work_spectrum, _process_device_power and fdc_pipeline_work_waterfall return FDC_ERR_INVALID_ARGUMENT and
 * change nothing (fdc_pipeline_flush_sinks still flushes a batch that is inside), and every plan writes complex float first: with integer output the
 * samples are narrowed behind the levels ("output sc16: narrowed"; "fused" again once levels are off).  One pass over the launch group's results reads
 * them once (fdc_pipeline_describe: "levels: pass"); with fine tuning on, off path 5, the rotation's pass reduces the turned samples it holds and no
 * second trip is made ("levels: with the rotation"). */
int fdc_pipeline_set_levels(fdc_pipeline *p, int32_t on);
int fdc_pipeline_levels(fdc_pipeline *p, float *dst, int nblocks);
void *fdc_pipeline_levels_device(fdc_pipeline *p);

/* CHANNEL GAINS: a per-channel output gain, applied on the device.  fdc_pipeline_set_output_format has ONE scale for every channel of the plan; the
 * channels of a real band differ by tens of dB, so with one scale the strong ones clip or the weak ones keep two or three bits of an sc8 / sc16 sample.
 * With a gain g_c (float32) for channel c, every sample of that channel's stream becomes
 *     y''_c[t] = ( f32(re(y'_c[t]) * g_c), f32(im(y'_c[t]) * g_c) )
 * where y' is exactly what the entry writes with gains off (after fine tuning when that is on).  Each product is rounded once in float32 and kept out of
 * FMA contraction with whatever produced y' (the rule of the integer input's scale and of fine tuning); float32 subnormals are kept, so the statement
 * holds for every finite value: in numpy, (y.view(np.float32) * np.float32(g)).view(np.complex64), bit for bit on every route.
 * Order of the settings, fixed: cut -> fine tuning -> GAIN -> levels -> sc16 / sc8 narrowing.  The levels are those of y'' (a caller who wants the
 * pre-gain power divides by g^2), so the clip rule peak * |scale| >= 32767.5 / 127.5 stays true; integer output is oq(y'' * scale): two roundings, the
 * gain's and then the narrowing's, which is observably not oq(y' * (g * scale)).  The debug spectrum is unchanged.
 *   fdc_pipeline_set_gains   gain[n], n = the channel count (else FDC_ERR_INVALID_ARGUMENT; n = 0 with no channels is accepted).  Any finite float32: zero
 *                            mutes, negative inverts.  NaN or +-Inf in any entry: FDC_ERR_INVALID_ARGUMENT, nothing changes.  gain = NULL, or every
 *                            entry exactly 1.0f, switches the setting off.
 *   fdc_pipeline_gains       copies the n = C gains in force to dst: C ones while off.
 * A SETTING like fdc_pipeline_set_output_format, _set_fine_tuning and _set_levels: it may change between any two calls and applies from the next one; it
 * does not touch the history, the block counter or the input-form latch, and survives fdc_pipeline_reset; refused while a pipelined sinks batch is inside
 * the handle; it waits for the handle's own stream before the device table is rewritten (device entries on another stream: the caller orders them).  The
 * first call that switches gains on allocates a device table of C floats, once; later calls — an AGC that sets new gains before every work call —
 * allocate nothing and copy C floats; nothing is allocated in a work call or a device entry.  A device call needs nblocks <= max_blocks only where it
 * already does (levels on, or a narrowed integer route): gains add no rule of their own.
 * While gains are on, fdc_pipeline_work_sinks, _work_spectrum, _process_device_power and fdc_pipeline_work_waterfall return FDC_ERR_INVALID_ARGUMENT and
 * change nothing (fdc_pipeline_flush_sinks still flushes), and every plan writes complex float first: with integer output the samples are narrowed behind
 * the gain ("output sc16: narrowed"; "fused" again once gains are off).  fdc_pipeline_describe names the route of the last call: where the rotation's
 * pass runs (fine tuning on, off path 5 or with a spectrum output) it multiplies the turned sample it holds ("gains: with the rotation"); otherwise one
 * pass over the launch group's float results multiplies them in place ("gains: pass") or, where the call narrows an integer output on the device
 * itself (the device entries, staged host outputs), reads them once and stores the narrow samples ("gains: with the narrowing").  With levels on the
 * same pass sums them ("levels: with the rotation" / "levels: with the gains"): no further trip over the output. */
int fdc_pipeline_set_gains(fdc_pipeline *p, const float *gain, int n);
int fdc_pipeline_gains(const fdc_pipeline *p, float *dst, int n);

/* CHANNEL LAG-1 CORRELATION: a per-block frequency estimate of every channel, summed on the device — the measurement of an AFC, as the levels are the
 * measurement of an AGC: fine tuning takes nu_c in cycles per output sample, and this says what nu_c should be.  With the setting on, every (block m of
 * the call, channel c) gets one complex float32 value from the lout_c samples the call produces for it:
 *     S[m][c] = sum_{j = 1 .. lout_c - 1}  y[j] conj(y[j - 1])
 * of the complex float32 samples y the entry writes, or would write before narrowing: AFTER fine tuning and the channel gain, BEFORE the sc16 / sc8
 * narrowing (cut -> fine tuning -> gain -> levels, lag-1 -> narrowing), so a loop sees the residual left by the fine tuning in force.  arg(S) / (2 pi)
 * is the row's mean frequency in cycles per output sample, the unit of fdc_pipeline_set_fine_tuning: added to the nu in force it cancels the residual;
 * |S| against the row's power (CHANNEL LEVELS) says how far to trust it.  Only the row's own samples: the product across the block boundary is not
 * taken, so the value needs no state and no sample of another call, span or launch group, and every cut of a stream gives the same values.
 * Layout: lag1[m][c] = (Re S, Im S), float[nblocks][C][2], c the plan's channel index (a channel that is a copy of another channel's slice has its
 * own entry); lout_c = 1 gives (+0, +0).  Rows with samples that are not finite give what IEEE arithmetic gives; no other row is disturbed.  The bits
 * of S[m][c] depend on lout_c and the row's sample values only (the levels' lane assignment and summation tree, each product and sum rounded on its
 * own, no atomics).  Each component is within (lout_c + 8) 2^-24 M of the exact sum over the float32 samples, M = sum_j |y[j]| |y[j - 1]| (relative
 * to M, not to |S|: the terms may cancel).
 *   fdc_pipeline_set_lag1        on != 0 / 0.  A SETTING with the semantics of fdc_pipeline_set_levels, word for word: it may change between any two
 *                                calls and applies from the next one; it does not touch the history, the block counter or the input-form latch, and
 *                                survives fdc_pipeline_reset; refused while a pipelined sinks batch is inside the handle; it waits for the handle's own
 *                                stream first.  The first call that switches it on allocates max_blocks*C float2 on the device and pinned on the
 *                                host, once; nothing in a work call, nothing inside a device entry.  With C = 0, on is accepted and every result
 *                                is empty.
 *   fdc_pipeline_lag1            the values of the last successful work call (host or device entry; a device entry's are read after a synchronise of
 *                                the stream it ran on): dst receives nblocks*C*2 floats.  nblocks must be that call's block count, otherwise
 *                                FDC_ERR_INVALID_ARGUMENT; the same while the setting is off and before any call.  A call of 0 blocks leaves the
 *                                previous result in place.
 *   fdc_pipeline_lag1_device     the device buffer ([block of the call][C] float2), NULL while off.  While the setting is on, a device call needs
 *                                nblocks <= max_blocks: above it FDC_ERR_INVALID_ARGUMENT, nothing enqueued.
 * While the setting is on, fdc_pipeline_work_sinks, _work_spectrum, _process_device_power and fdc_pipeline_work_waterfall return
 * FDC_ERR_INVALID_ARGUMENT and change nothing (fdc_pipeline_flush_sinks still flushes), and every plan writes complex float first: with integer output
 * the samples are narrowed behind the pass ("output sc16: narrowed"; "fused" again once it is off).  It is always one pass of its own over the launch
 * group's final float results, which reads them once (fdc_pipeline_describe: "lag1: pass"). */
int fdc_pipeline_set_lag1(fdc_pipeline *p, int32_t on);
int fdc_pipeline_lag1(fdc_pipeline *p, float *dst, int nblocks);
void *fdc_pipeline_lag1_device(fdc_pipeline *p);

/* CHANNEL DEMODULATION: the FM discriminator (GNU Radio's quadrature_demod_cf) or the envelope (complex_to_mag) of every channel, on the device, as the
 * last pass over the float results: cut -> fine tuning -> gain -> levels, lag-1 -> demodulation, in the place the sc16 / sc8 narrowing has.  While the
 * setting is on, every channel's output stream is REAL float32, 4 bytes per sample: the same number of samples in the same channel-major layout
 * (device entries: channel c's nblocks*lout_c elements start at ELEMENT offset nblocks*out_off_c of d_out; host entries: outs[c] is
 * float[nblocks*lout_c]).  With y[t] the complex float32 sample the entry would write with the setting off (after fine tuning and the channel gain;
 * levels and lag-1 stay those of y):
 *   FDC_DEMOD_FM    P = y[t] conj(y[t-1]) = (a.x b.x + a.y b.y, a.y b.x - a.x b.y) with a = y[t], b = y[t-1], every product and sum rounded on its own
 *                   (lag-1's term); d[t] = float32(gain * atan2f(Im P, Re P)).  Where both components of P compare equal to zero d[t] = +0.0f: a silent
 *                   channel and a stream start give zeros, not +-pi from signed zeros.  NaN propagates.  gain = 1 / (2 pi) gives cycles per output
 *                   sample, the unit of fdc_pipeline_set_fine_tuning and of arg(S) / (2 pi) of the lag-1 correlation.
 *                   |d[t] - gain theta| <= |gain| (5 + 13 |theta|) 2^-24 modulo 2 pi |gain|, theta the exact angle of the exact product of the float32
 *                   samples, where |y[t]| |y[t-1]| >= 2^-60.
 *   FDC_DEMOD_MAG   d[t] = float32(gain * sqrt(float32(float32(re re) + float32(im im)))), the square root correctly rounded: numpy states it bit
 *                   for bit in float32.  It needs no state and uses none.
 * THE SAMPLE IN FRONT (FM): inside a call y[t-1] is the element before y[t] in the channel's run (a channel's stream is contiguous across the blocks of
 * a call).  In front of a call's first sample stands the handle's CARRY, the last y of each channel of the previous call, held on the device: it is used
 * when the call CONTINUES the stream, that is when its first_block is the block after the last block of the previous successful demodulating call;
 * for fdc_pipeline_work and its kin that is always so between resets, and the sub-batches a host entry cuts its call into are linked the same way.
 * Otherwise the stream starts anew, y[-1] = 0 and d[0] = +0: a device or span entry elsewhere in the stream, the first call after create or
 * fdc_pipeline_reset, after switching from OFF, after a change of mode, after a call that failed once it had begun to enqueue (a call that is REFUSED
 * for its arguments or the handle's settings enqueues nothing and leaves the carry as it was: the next call may still continue the stream).  A change of gain alone keeps the carry.  The bits of d
 * depend on the stream's samples and the setting only: not on how the stream is cut into calls, sub-batches, launch groups or chunks, nor on the route.
 *   fdc_pipeline_set_demod   mode FDC_DEMOD_OFF / _FM / _MAG; gain finite and not zero (ignored with OFF); anything else FDC_ERR_INVALID_ARGUMENT and
 *                            the previous setting stays in force.  A SETTING like the ones above: it applies from the next call, does not touch the
 *                            history, the block counter or the input-form latch, and survives fdc_pipeline_reset (the carry does not); refused while a
 *                            pipelined sinks batch is inside the handle; it waits for the handle's own stream first.  The first call that switches it
 *                            on allocates two carry buffers of C float2 and the float staging of integer output (max_blocks*sum_lout samples), once;
 *                            the host entries' 4-byte staging is allocated at their first such call; nothing in the steady state, nothing inside a
 *                            device entry.  While it is on a device call needs nblocks <= max_blocks.
 *   fdc_pipeline_demod       the setting in force (either pointer may be NULL).
 * EXCLUSIVE with integer output: set_demod(FM / MAG) is refused while the output format is not FDC_OQ_FC32, and fdc_pipeline_set_output_format(sc16 /
 * sc8) while the demodulation is on.  While it is on, fdc_pipeline_work_sinks, _work_spectrum, _process_device_power and fdc_pipeline_work_waterfall
 * return FDC_ERR_INVALID_ARGUMENT and change nothing, and so do the group's work entries when a member has it on (there is no group setter: 4-byte
 * samples would misplace the spans, and a span's first sample has no predecessor on its device).  fdc_pipeline_describe: "demod: fm" / "demod: mag"
 * after a call that ran it. */
enum { FDC_DEMOD_OFF = 0, FDC_DEMOD_FM = 1, FDC_DEMOD_MAG = 2 };
int fdc_pipeline_set_demod(fdc_pipeline *p, int32_t mode, float gain);
int fdc_pipeline_demod(const fdc_pipeline *p, int32_t *mode, float *gain);
/* The demodulating pass alone, for complex channel streams that are on the device already (and the entry the footprint tests reach the kernel by):
 * d_in holds one call's complex float32 results in the layout fdc_pipeline_process_device writes (nblocks blocks, channel c at element offset
 * nblocks*out_off_c), d_out receives the real float32 samples at the same element offsets.  FM: d_carry_in (C float2, NULL: nothing stands in front,
 * the stream starts anew) is read, d_carry_out (C float2, another buffer, not NULL) receives the last complex sample of every channel; MAG ignores
 * both.  Exactly 4*nblocks*sum_lout bytes of d_out and, in FM, C float2 of d_carry_out are written, enqueued on `stream` (NULL: the handle's).  The
 * handle gives its channel table only: its setting, its own carry and its stream position are neither read nor changed, whatever its setting is.
 * mode other than FM / MAG, a gain that is zero or not finite, nblocks < 0, a NULL buffer: FDC_ERR_INVALID_ARGUMENT, nothing enqueued. */
int fdc_pipeline_demod_device(const fdc_pipeline *p, int32_t mode, float gain, const void *d_in, void *d_out, const void *d_carry_in, void *d_carry_out,
                              int nblocks, void *stream);

/* CHANNEL AUDIO: a decimating FIR (GNU Radio's fir_filter_fff with decimation D) behind the channel demodulation, on the device, so that the ports
 * leave the card at the audio rate.  With d_c[t] the real float32 stream the demodulation gives for channel c, D the decimation and h[0 .. K-1] the
 * float32 taps:
 *     a_c[n] = sum over k = 0 .. K-1 of h[k] d_c[n D - k]
 * in float32, k ascending from acc = +0, every product and every sum rounded on its own (no fused multiply-add); NaN and +-Inf follow IEEE.
 * FDC_AUDIO_S16: q = saturate(round_half_even(float32(a scale))), NaN -> 0, +-Inf -> the limits (the rule of sc16 output).
 * THE HISTORY: in front of a call's first sample stand K - 1 values of d, held per channel on the device.  They are used when the call CONTINUES
 * the stream, that is when its first_block is the block after the last one of the previous successful call with the audio on (the handle keeps this
 * position for the audio, in both demodulation modes); otherwise zeros stand there: after create or fdc_pipeline_reset, after switching the audio
 * on or changing the decimation or the taps, after a change of demodulation mode, after a call that failed once it had begun to enqueue, at a device
 * or span call elsewhere in the stream.  A new format, audio scale or demodulation gain alone keeps the history, and a call that is REFUSED leaves it
 * as it was.  After a call the history is the tail of (what stood in front, the call's d): calls of fewer than K - 1 samples are covered.  The
 * bits of the audio depend on the stream's samples and the settings only, not on how the stream is cut.
 * THE LAYOUT: D divides every lout_c, so every block gives lout_c / D audio samples of channel c however the stream is cut.  The audio of a call is a
 * BLOCK-MAJOR matrix [nblocks][A] of float32 or int16, A = sum over c of lout_c / D; in a row channel c owns the lout_c / D columns from
 * aoff_c = sum over i < c of lout_i / D on (the audio's own prefix sums in channel order); row m belongs to block first_block + m.  Channel c's
 * stream is column block c of all rows, row after row.
 * THE AUDIO IS A RESULT HELD BY THE HANDLE, like the levels: it is never written to a buffer whose size only the caller knows.
 *   fdc_pipeline_set_audio      decim 0 switches it off (the other arguments are ignored).  Otherwise decim 1 .. 64, ntaps 1 .. 256 finite taps, format
 *                               FDC_AUDIO_F32 / _S16, scale finite and not zero (ignored for F32).  FDC_ERR_INVALID_ARGUMENT, the previous setting staying
 *                               in force: any of these out of range; while the demodulation is off; where decim does not divide some lout_c (the message
 *                               names the channel); while a pipelined sinks batch is inside the handle.  fdc_pipeline_set_demod(FDC_DEMOD_OFF) is
 *                               refused while the audio is on.  A SETTING: it applies from the next call and survives fdc_pipeline_reset (the history
 *                               does not); it waits for the handle's own stream first.  It allocates everything the feature needs, once per size: the taps
 *                               on the device, two history buffers of C (K - 1) floats, the rows of max_blocks blocks and their pinned twin; nothing in
 *                               the steady state of any entry.  A plan without channels accepts it.
 *   fdc_pipeline_audio_setting  the setting in force (decim 0: off); any pointer may be NULL; taps receives ntaps floats (room for 256).
 *   fdc_pipeline_audio_row      A, 0 while off.
 *   fdc_pipeline_audio          the first nblocks rows of the last call, nblocks being that call's block count (as fdc_pipeline_levels), to dst:
 *                               nblocks * A elements.  capacity_bytes below that: FDC_ERR_INVALID_ARGUMENT, nothing written.  After a host entry it
 *                               is a memcpy; after a device entry it waits for the stream that one ran on.
 *   fdc_pipeline_audio_device   the device buffer ([block of the last call][A]), NULL while off.
 * WHILE IT IS ON, the host stream entries (fdc_pipeline_work, _work_real, _work_iq and the span forms) run the demodulation and the audio pass and
 * hand the host the audio alone: they write NOTHING to outs, which may be NULL, and copy no port.  The device entries write the demodulated float
 * ports to d_out as ever (4 * nblocks * sum_lout bytes) and the audio to the handle's buffer.  fdc_pipeline_describe: "audio: pass" after a call
 * that ran it. */
enum { FDC_AUDIO_F32 = 0, FDC_AUDIO_S16 = 1 };
int fdc_pipeline_set_audio(fdc_pipeline *p, int32_t decim, const float *taps, int32_t ntaps, int32_t format, float scale);
int fdc_pipeline_audio_setting(const fdc_pipeline *p, int32_t *decim, int32_t *ntaps, int32_t *format, float *scale, float *taps);
int64_t fdc_pipeline_audio_row(const fdc_pipeline *p);
int fdc_pipeline_audio(fdc_pipeline *p, void *dst, size_t capacity_bytes, int nblocks);
void *fdc_pipeline_audio_device(fdc_pipeline *p);
/* The audio pass alone, on device buffers of the caller (and the entry the footprint tests reach the kernel by), with the handle's channel table and
 * audio setting (which must be on) and nothing of its stream state: d_in real float32 in fdc_pipeline_process_device's layout (channel c at element
 * offset nblocks*out_off_c), d_out exactly nblocks * A elements, d_hist_in C (K - 1) floats or NULL (zeros), d_hist_out another buffer that receives
 * exactly C (K - 1) floats (NULL only where K = 1).  Enqueued on `stream` (NULL: the handle's). */
/* While the channel squelch is on (below) this entry does read one thing of the handle's: it runs the GATED form over the mask of the last successful
 * work call (fdc_pipeline_squelch_device), and is refused unless nblocks is that call's block count; the bytes written are the same. */
int fdc_pipeline_audio_pass_device(const fdc_pipeline *p, const void *d_in, void *d_out, const void *d_hist_in, void *d_hist_out, int nblocks,
                                   void *stream);

/* AUDIO RESAMPLER: the second form of the channel audio, a polyphase FIR with interpolation L = up and decimation M = down behind the demodulator,
 * which takes the channel rate fs l / N to a chosen audio rate (25 kHz to 8 kHz: 8 / 25; to 48 kHz: 48 / 25).  The two forms replace each other.
 * tests/resample_model.py is the definition.  With d_c[t] the float32 stream the demodulation gives for channel c, t the ABSOLUTE sample index (sample 0
 * is the first of block 0, block m holds samples m lout_c .. (m + 1) lout_c - 1), h[0 .. ntaps-1] the prototype taps, Kp = ceil(ntaps / L) and h
 * padded with +0 to L Kp entries, output n of the stream (n = 0, 1, ...; it stands at input time n M / L) is
 *
 *     a_c[n] = sum over k = 0 .. Kp-1 of h[k L + (n M mod L)] d_c[floor(n M / L) - k]
 *
 * in float32, k ascending from acc = +0, every product and every sum rounded on its own (fdc_pipeline_set_audio's rule; the padded zero taps are part
 * of the sum): upsample by L, filter with h, keep every M-th sample, started at sample 0.  With L = 1 it is fdc_pipeline_set_audio's sum with D = M.
 * FDC_AUDIO_S16 narrows as there.
 * THE LAYOUT: output n belongs to block floor(floor(n M / L) / lout_c).  Block m owns the outputs ceil(m lout_c L / M) .. ceil((m + 1) lout_c L / M) - 1:
 * cnt_c(m) of them, which is W_c or W_c - 1 with W_c = ceil(lout_c L / M) and depends on the ABSOLUTE block index alone (fdc_audio_resampler_counts).
 * The audio of a call is the block-major matrix [nblocks][A] with A = sum of the W_c; channel c owns the W_c columns from aoff_c = sum over i < c of
 * W_i on; cell (m, c) holds its cnt_c outputs in order, and where cnt_c = W_c - 1 one pad element of zero bits follows.  The pass writes every element.
 * THE HISTORY is fdc_pipeline_set_audio's with K = Kp: Kp - 1 values of d per channel stand in front of a call that continues the stream, zeros
 * otherwise; phase and counts come from the absolute index of the call's first block either way, so the calls of a continuing stream concatenate to
 * the stream's bits however it is cut.  THE GATE is the decimating form's: with the channel squelch on (with or without the tone squelch) every element
 * of a closed (block, channel) cell is zero bits and the history runs on over the ungated stream.
 *   fdc_pipeline_set_audio_resampler  up 0 switches it off.  Otherwise up 1 .. 64, down 1 .. 128, gcd(up, down) = 1 (a ratio that is not reduced
 *                               would leave tap phases unused), ntaps >= 1 finite taps with ceil(ntaps / up) <= 256; format and scale as
 *                               fdc_pipeline_set_audio.  FDC_ERR_INVALID_ARGUMENT, the previous setting staying in force: those, while the
 *                               demodulation is off, while a pipelined sinks batch is inside the handle, while the audio packing is on, and where
 *                               lout_c up reaches 2^31.  A successful call switches the decimating form off, and a successful
 *                               fdc_pipeline_set_audio(decim > 0) switches this one off; fdc_pipeline_set_audio(decim 0) switches off whichever is
 *                               on.  While it is on fdc_pipeline_set_audio_packing(1), fdc_pipeline_set_demod(OFF) and
 *                               fdc_pipeline_audio_pass_device are refused and fdc_pipeline_audio_setting reports decim 0.  A SETTING: it survives
 *                               fdc_pipeline_reset, allocates everything once per size and nothing on any entry.  A new ratio or other taps restart
 *                               the stream; a new format or scale alone keeps the history; a new ratio or format leaves no rows to fetch.
 *                               All offsets into the matrix are 64-bit: max_blocks A is bounded by memory only.
 *   fdc_pipeline_audio_resampler_setting  the setting in force (up 0: off); any pointer may be NULL; taps receives ntaps floats only where
 *                               taps_capacity >= ntaps.
 *   fdc_pipeline_audio_first_block  the absolute index of row 0 of the audio the handle holds (either form), -1 where there is none.
 *   fdc_audio_resampler_counts  cnt(first_block + i) for i = 0 .. nblocks-1, of a channel of lout samples per block: a pure host function.
 * fdc_pipeline_audio_row (A), fdc_pipeline_audio and fdc_pipeline_audio_device serve the matrix above.  fdc_pipeline_describe: "audio: resampled"
 * or "audio: resampled, gated" after a call that ran it.  With the setting off every entry launches exactly what it launched before. */
int fdc_pipeline_set_audio_resampler(fdc_pipeline *p, int32_t up, int32_t down, const float *taps, int32_t ntaps, int32_t format, float scale);
int fdc_pipeline_audio_resampler_setting(const fdc_pipeline *p, int32_t *up, int32_t *down, int32_t *ntaps, int32_t *format, float *scale, float *taps,
                                         int32_t taps_capacity);
int64_t fdc_pipeline_audio_first_block(const fdc_pipeline *p);
int fdc_audio_resampler_counts(int32_t lout, int32_t up, int32_t down, int64_t first_block, int32_t nblocks, int32_t *counts);
/* The resampling pass alone, on device buffers of the caller, with the handle's channel table and resampler setting (which must be on) and nothing
 * of its stream state: d_in as fdc_pipeline_audio_pass_device's, d_out exactly nblocks * A elements, the histories exactly C (Kp - 1) floats
 * (d_hist_in NULL: zeros; d_hist_out NULL only where Kp = 1), first_block the absolute index of the call's first block, d_mask NULL or [nblocks][C]
 * bytes of the caller's (the gated form).  Enqueued on `stream` (NULL: the handle's). */
int fdc_pipeline_audio_resampler_pass_device(const fdc_pipeline *p, const void *d_in, void *d_out, const void *d_hist_in, void *d_hist_out,
                                             int64_t first_block, int nblocks, const void *d_mask, void *stream);

/* CHANNEL SQUELCH: per channel a carrier-operated squelch on the block powers the levels give, decided on the device, with hysteresis and a hang time;
 * with the channel audio on it gates the audio.  The setting: per-channel float32 thresholds open_c >= close_c >= 0, finite, and one hang count of
 * blocks, 0 .. 65535.  The state of a channel is (open in {0, 1}, h in [0, hang]) and starts as (0, 0).  For block m of the stream, in order:
 *     p  = the float32 power the levels hold for (m, c) (after fine tuning and the gain)
 *     g2 = float32(g_c g_c), g_c the channel gain in force (1 while the gains are off);  To = float32(g2 open_c), Tc = float32(g2 close_c)
 *     if p >= To: open = 1, h = hang;   else if open and p >= Tc: h = hang;   else if open: h > 0 ? h -= 1 : open = 0
 *     mask[m][c] = open
 * Every comparison is an IEEE float32 >=, so a NaN power or a NaN threshold product is below.  The thresholds therefore refer to the power IN FRONT of
 * the gain: an AGC that levels every channel does not defeat them.  Their unit is the levels' own: the sum over the row of re^2 + im^2, which is the
 * mean power times lout_c.  tests/squelch_model.py states the rule in numpy, and the mask is that model's byte for byte.
 * A GAIN OF 0 makes both products +0, which every power that is not NaN reaches (the gained samples are zeros, their power +0): a channel muted
 * with gain 0 has mask = 1, whatever its thresholds.  Mute with the squelch's thresholds, not with the gain, where the mask matters.
 * THE STATE lives on the device, one int32 pair per channel.  It is used when a call CONTINUES the stream, that is when its first_block is the block
 * after the last one of the previous successful call with the squelch on (the handle keeps this position for the squelch); otherwise every channel
 * starts at (0, 0): after create or fdc_pipeline_reset, after switching the squelch on, after a call that failed once it had begun to enqueue, at a
 * device or span call elsewhere in the stream.  New thresholds or a new hang count while it is on keep `open`; h is read as min(h, the hang count
 * in force), and is 0 while the channel is closed.  A call that is REFUSED leaves everything as it was.  The bits of the mask depend on the
 * stream's powers and the settings only, not on how the stream is cut into calls, sub-batches or launch groups, nor on the plan's route.
 *   fdc_pipeline_set_squelch          open_thr NULL switches it off.  FDC_ERR_INVALID_ARGUMENT, the previous setting staying in force: n != C; a threshold
 *                                     that is not finite or negative; close > open; hang out of range; while the levels are off; while a pipelined sinks
 *                                     batch is inside the handle.  fdc_pipeline_set_levels(p, 0) is refused while the squelch is on.  A SETTING: it
 *                                     applies from the next call and survives fdc_pipeline_reset (the state does not); it waits for the handle's own
 *                                     stream first.  It allocates everything the feature needs, once: two threshold tables, two state buffers, max_blocks
 *                                     C mask bytes and their pinned twin; nothing in the steady state of any entry.  A plan without channels accepts it.
 *   fdc_pipeline_squelch_setting      the setting in force; any pointer may be NULL; the thresholds receive C floats each, hang -1 while it is off.
 *   fdc_pipeline_squelch              mask[nblocks][C] of the last call, one byte (0 / 1) per block and channel, nblocks being that call's block count
 *                                     (as fdc_pipeline_levels).  capacity_bytes below nblocks C: FDC_ERR_INVALID_ARGUMENT, nothing written.  After a
 *                                     host entry it is a memcpy from the pinned twin, copied home with the levels; after a device entry it waits
 *                                     for the stream that one ran on.
 *   fdc_pipeline_squelch_device       the device mask ([block of the last call][C] bytes), NULL while off.
 * WITH THE CHANNEL AUDIO ON (fdc_pipeline_set_audio) the audio pass is GATED: an audio sample of a closed (block, channel) is stored as +0.0f
 * (FDC_AUDIO_F32) or 0 (FDC_AUDIO_S16), the filter's history runs on over the ungated demodulated stream, so a channel that opens has the bits it
 * would have had without a squelch, and the pass writes exactly the bytes of the ungated pass; closed tiles are not filtered.  The demodulated ports
 * themselves are NOT gated: the device entries write d_out as without the squelch, and with the audio off the squelch gives the mask only.
 * While it is on the entries that refuse under the levels refuse as they do; there is no group setter.  fdc_pipeline_describe: "squelch: pass" after a
 * call that ran it, and "audio: pass, gated". */
int fdc_pipeline_set_squelch(fdc_pipeline *p, const float *open_thr, const float *close_thr, int n, int32_t hang);
int fdc_pipeline_squelch_setting(const fdc_pipeline *p, float *open_thr, float *close_thr, int32_t *hang);
int fdc_pipeline_squelch(fdc_pipeline *p, uint8_t *dst, size_t capacity_bytes, int nblocks);
void *fdc_pipeline_squelch_device(fdc_pipeline *p);
/* The decision alone, on device buffers of the caller (and the entry the tests reach the kernel by with hand-made powers), with the handle's setting
 * (which must be on), gains and channel count and nothing of its stream state: d_levels [nblocks][C] float32 pairs (power, peak) as
 * fdc_pipeline_levels_device holds them, d_mask exactly nblocks C bytes, d_state_in C int32 pairs (open, h) or NULL ((0, 0)), d_state_out another
 * buffer that receives exactly C int32 pairs.  Enqueued on `stream` (NULL: the handle's). */
int fdc_pipeline_squelch_pass_device(const fdc_pipeline *p, const void *d_levels, void *d_mask, const void *d_state_in, void *d_state_out, int nblocks,
                                     void *stream);

/* PACKED AUDIO: with the channel audio and the channel squelch on, only the audio of open (block, channel) cells leaves the device, one cell behind
 * the other, instead of the [nblocks][A] matrix with its zeros.  With D the audio's decimation and npb_c = lout_c / D:
 *     a CELL is (m, c), block m of the call and channel c, of weight w(m, c) = mask[m][c] npb_c;  cells are ordered ROW-MAJOR, m outer, c inner;
 *     off(m, c) = the sum of w over all cells in front of (m, c) (for a closed cell: where it would go);  count = the sum of w over all cells;
 *     packed[off(m, c) + i] = audio[m][aoff_c + i]  for every OPEN cell and 0 <= i < npb_c,
 * audio being the matrix the audio pass gives without packing (gated or not: the same bits on open cells), in the audio setting's own format.  The
 * filter's history runs on over the ungated stream as ever.  The offsets start at 0 in EVERY call: the packing has no stream state.  Two consequences:
 * with every cell open the packed bytes are the matrix's bytes; and the packed buffers of the calls of a stream, concatenated, are the packed buffer
 * of the stream in one call, however it is cut (which is why the order is block-major).  tests/audio_pack_model.py states this in numpy, and the
 * packed bytes, the count and the mask are that model's byte for byte.  NOT BUILT: a channel-major order; packing of the demodulated ports.
 *   fdc_pipeline_set_audio_packing  on != 0 switches it on.  FDC_ERR_INVALID_ARGUMENT, the previous setting staying in force: unless both the channel audio
 *                                   and the squelch are on; where max_blocks * A >= 2^32 (the offsets are 32-bit words); while a pipelined sinks batch
 *                                   is inside the handle.  While it is on, fdc_pipeline_set_audio(decim 0) and fdc_pipeline_set_squelch(NULL ...) are
 *                                   refused (switch the packing off first), and so is a new decimation that breaks the 2^32 bound; a new audio format,
 *                                   decimation or taps is allowed otherwise and, as a switch of the packing itself, leaves nothing to fetch until the
 *                                   next call.  A SETTING: it applies from the next call and survives fdc_pipeline_reset; it waits for the handle's own
 *                                   stream first.  It allocates everything the feature needs, once: the offsets uint32[max_blocks][C], one int64
 *                                   running total on the device and its pinned twin; nothing in the steady state of any entry.  The packed elements
 *                                   live in the audio's own buffers (count <= nblocks * A).  A plan without channels accepts it.
 *   fdc_pipeline_audio_packing      1 while on, 0 while off, -1 for a NULL handle.
 *   fdc_pipeline_audio_packed       the packed audio of the last call, nblocks being that call's block count (as fdc_pipeline_audio).  *count receives
 *                                   the number of ELEMENTS whenever the call is valid (right handle state, right nblocks, count not NULL).  dst NULL: a
 *                                   query for the count.  capacity_bytes below count elements: FDC_ERR_INVALID_ARGUMENT, nothing written to dst, *count
 *                                   set all the same, so the caller can size its buffer.  After a host entry it is a memcpy from the pinned twin; after
 *                                   a device entry it waits for the stream that one ran on, fetches the count and then count elements.
 * WHILE IT IS ON: fdc_pipeline_audio (the matrix) is refused.  fdc_pipeline_audio_device is the packed buffer, of which only the first count elements
 * are specified.  The host stream entries bring the mask and the 8-byte count home with the levels, and after the call's synchronise copy exactly count
 * elements and synchronise once more (neither where count is 0): no entry copies more than count audio elements over the link.  AT FULL OCCUPANCY that
 * second synchronise is pure cost: leave the packing off on a band whose channels are mostly open.  The sub-batches of a long host call append to one
 * packed buffer through the running total on the device.  The device entries write the demodulated ports to d_out as ever, the packed audio to
 * the handle's buffer and the count to the device word.  fdc_pipeline_audio_pass_device runs the PACKED form over the handle's mask and offsets of the
 * last successful call (refused unless nblocks is that call's block count) and writes exactly count elements at the front of d_out, plus the history
 * as before.  fdc_pipeline_describe: "audio: pass, gated, packed" after a call that ran it.  With the setting off every entry launches exactly the
 * kernels it launches without this feature. */
int fdc_pipeline_set_audio_packing(fdc_pipeline *p, int on);
int fdc_pipeline_audio_packing(const fdc_pipeline *p);
int fdc_pipeline_audio_packed(fdc_pipeline *p, void *dst, size_t capacity_bytes, int nblocks, int64_t *count);
/* The offsets alone, on device buffers of the caller (and the entry the tests reach the kernels by with hand-made masks), with the handle's channel
 * table and the audio's decimation (the audio must be on) and nothing of its state: d_mask [nblocks][C] bytes, d_base_in one int64 added to every
 * offset and to the total (NULL: 0), d_off exactly nblocks C uint32 words (an offset is kept modulo 2^32), d_total_out one int64, which may be d_base_in's
 * word.  Three launches, none of which waits on another workgroup.  Enqueued on `stream` (NULL: the handle's). */
int fdc_pipeline_audio_pack_offsets_device(const fdc_pipeline *p, const void *d_mask, const void *d_base_in, void *d_off, void *d_total_out, int nblocks,
                                           void *stream);

/* CHANNEL TONES: per channel a bank of T narrow correlators (a tone squelch's measurement: CTCSS, pilot and paging tones) over the demodulated samples,
 * integrated over frames of W blocks, on the device.  The setting: T tones per channel, 1 .. 64; a table inc[C][T] of uint32 phase increments; a group
 * length S >= 1 that divides every lout_c; a frame length W of 1 .. 4096 blocks.  With d the real float32 stream k_chan_demod writes for channel c (the
 * demodulation gain included), G = lout_c / S and b the stream's block index:
 *     u(b, q)  = d[b lout_c + q S + i] summed over i = 0 .. S - 1, ascending, in float32 from +0, every sum rounded on its own       (a boxcar by S)
 *     g        = b G + q (64 bits);  k = ((inc[c][t] g) mod 2^32) >> 22;  (cs, sn) = table[k]
 *     re = re + float32(u cs);  im = im - float32(u sn)       per group, g ascending, every product and sum rounded on its own, from (+0, +0)
 * table: 1024 float32 pairs (cos, sin)(2 pi k / 1024), designed in double and rounded once, entries 0 / 256 / 512 / 768 exactly (1, 0), (0, 1), (-1, 0),
 * (0, -1) (fdc_tone_table writes them; host only, no handle).  The accumulator of (c, t) runs on over the W blocks of a frame; at the frame's last group
 * it is the frame's row Z[f][c][t] (re, im) and starts again at (+0, +0).  The phase is an integer function of the stream's own group index: no drift,
 * and nothing depends on how the stream is cut.  tests/tones_model.py states this in numpy, and the rows are that model's byte for byte.
 * For a tone of amplitude a at frequency f in d, at channel rate r: |Z| ~ a (W lout_c / 2) droop(f), droop(f) = sin(pi f S / r) / (S sin(pi f / r)); an
 * increment is round(2^32 f S / r).  The tones are NOT gated by the squelch; the decision on top of them is the host's, or the device's (TONE SQUELCH).
 * THE STATE: the handle keeps a block position for the tones, the blocks already inside the open frame (fill, a host integer) and the open frame's
 * accumulators, float2[C][T], on the device.  A call CONTINUES the stream when its first_block is the block after the last one of the previous
 * successful call with the tones on; otherwise fill = 0 and the accumulators are zero: after create or fdc_pipeline_reset, after switching the tones on
 * or changing any part of the setting, after a change of demodulation mode, after a call that failed once it had begun to enqueue, at a device or span
 * call elsewhere in the stream.  A new demodulation gain alone keeps the state.  A call that is REFUSED leaves everything as it was.  A call of nb
 * blocks completes nf = (fill + nb) div W frames and leaves fill = (fill + nb) mod W: frames are counted from the tone stream's start (the phase uses
 * the stream's block index all the same), and nf may be 0.  The rows of the calls of a stream, one behind the other, are the rows of the stream in
 * one call, byte for byte, however it is cut into calls, sub-batches or launch groups.
 *   fdc_pipeline_set_tones          inc NULL switches it off.  FDC_ERR_INVALID_ARGUMENT, the previous setting staying in force: nchan != C; ntones not in
 *                                   1 .. 64, group < 1, frame_blocks not in 1 .. 4096; group does not divide some lout_c (the message names the channel);
 *                                   while the demodulation is off; while a pipelined sinks batch is inside the handle; where the rows of the longest
 *                                   call would exceed 2^31 bytes.  fdc_pipeline_set_demod(FDC_DEMOD_OFF) is refused while the tones are on.  A SETTING:
 *                                   it applies from the next call and survives fdc_pipeline_reset (the state does not); it waits for the handle's own
 *                                   stream first.  It allocates everything the feature needs, once per size: the table, the increments, two carry
 *                                   buffers of C T, ((max_blocks + W - 1) div W) C T rows and their pinned twin; nothing in the steady state of any
 *                                   entry.  A plan without channels accepts it.
 *   fdc_pipeline_tones_setting      the setting in force; any pointer may be NULL; ntones is 0 while off; inc receives C T words.
 *   fdc_pipeline_tones              the rows the last call completed, [nf][C][T] float32 pairs, nblocks being that call's block count (as
 *                                   fdc_pipeline_levels); *nframes receives nf.  capacity_bytes below nf C T 8: FDC_ERR_INVALID_ARGUMENT, nothing
 *                                   written.  After a host entry it is a memcpy from the pinned twin, copied home with the levels (no copy where
 *                                   nf = 0); after a device entry it waits for the stream that one ran on.
 *   fdc_pipeline_tones_device       the device rows, NULL while off.
 * Whether the ports themselves go to the host is unchanged: with the channel audio off the host entries write the demodulated ports to outs, with it
 * on they do not; the device entries write d_out as ever.  The tones pass is one more launch behind k_chan_demod, independent of the audio, the squelch
 * and the packing.  fdc_pipeline_describe: "tones: pass" after a call that ran it.  With the setting off every entry launches exactly the kernels it
 * launches without this feature.  There is no group setter. */
int fdc_pipeline_set_tones(fdc_pipeline *p, const uint32_t *inc, int nchan, int ntones, int32_t group, int32_t frame_blocks);
int fdc_pipeline_tones_setting(const fdc_pipeline *p, int32_t *ntones, int32_t *group, int32_t *frame_blocks, uint32_t *inc);
int fdc_pipeline_tones(fdc_pipeline *p, void *dst, size_t capacity_bytes, int nblocks, int32_t *nframes);
void *fdc_pipeline_tones_device(fdc_pipeline *p);
/* The pass alone, on device buffers of the caller (and the entry the tests reach the kernel by with hand-made samples), with the handle's channel table
 * and the tones' setting (which must be on) and nothing of its stream state: d_in real float32 in fdc_pipeline_process_device's layout (channel c at
 * element offset nblocks*out_off_c), blocks [first_block, first_block + nblocks) of a stream with `fill` blocks (0 .. W - 1) already in the open frame;
 * d_carry_in C T float32 pairs or NULL (zeros; read only where fill > 0), d_carry_out another buffer that receives exactly C T pairs (zeros where the
 * call leaves no frame open), d_frames exactly ((fill + nblocks) div W) C T pairs (NULL where that is 0).  Enqueued on `stream` (NULL: the handle's). */
int fdc_pipeline_tones_pass_device(const fdc_pipeline *p, const void *d_in, void *d_frames, const void *d_carry_in, void *d_carry_out, int64_t first_block,
                                   int32_t fill, int nblocks, void *stream);
/* The 1024 (cos, sin) pairs of the tones' reference, 2048 floats.  Host only, no handle. */
int fdc_tone_table(float *dst);

/* TONE SQUELCH: thresholds on the frame rows of the channel tones decide, per channel and frame, whether the selected tone is there, and the decision
 * gates the carrier squelch's mask, all on the device: the audio and the packed audio of a channel whose carrier is up but whose tone is another
 * user's never leave the card.  It needs the channel tones (T, S, W) and the channel squelch.  The setting: per channel a tone index tone_c (-1: the
 * channel is not tone-gated, else 0 .. T - 1), float32 thresholds open_c >= close_c >= 0 and a float32 ratio_c >= 0, all finite; for all channels a
 * guard of 0 .. 63 tones and a hang count of 0 .. 65535 FRAMES.  Of the row Z[f][c][0 .. T - 1] of a completed frame, with sel = tone_c:
 *     e_t = float32(float32(re re) + float32(im im));   e = e_sel
 *     o   = the largest e_t over the t with |t - sel| > guard, from +0 by "e_t > o ? e_t : o" (a NaN is never taken; +0 where no such t is left)
 *     R   = float32(ratio_c o);   strong = e >= open_c and e >= R;   hold = e >= close_c and e >= R;   low = neither
 * every comparison an IEEE float32 >=, so a NaN is below.  Over the frames runs the channel squelch's own state machine with frames in the place of
 * blocks, from (open, h) = (0, 0): strong -> (1, hang); open and not low -> h = hang; open and low -> h - 1, closing at 0; dec[f][c] = open behind
 * frame f.  The unit of the thresholds is |Z|^2 (fdc_pipeline_set_tones gives |Z| for a tone of a given amplitude).
 * THE GATE IS CAUSAL.  Block m of a call stands in frame j = (fill + m) div W counted from the call's first frame, fill being the tones' own.  The
 * decision in force for it is the carried state's `open` for j = 0 and dec[j - 1][c] otherwise, and mask[m][c] = carrier mask[m][c] AND in force.  The
 * latency is one frame by construction, which is what makes the bytes independent of how the stream is cut; a caller who wants less picks a smaller W
 * and a hang.  A channel with tone -1 keeps its carrier mask, has dec = 1, and its state is written as (0, 0).  tests/tone_squelch_model.py states all
 * of this in numpy, and dec and the mask are that model's byte for byte.
 * THE STATE lives on the device, one int32 pair per channel.  The tone squelch continues exactly where the tones continue their stream (see CHANNEL
 * TONES); otherwise it restarts at (0, 0) with fill 0, so the first frame of a fresh stream is closed.  A new tone-squelch setting restarts the state
 * only, not the tones' frames.  A call that is REFUSED leaves everything as it was.
 *   fdc_pipeline_set_tone_squelch     tone NULL switches it off.  FDC_ERR_INVALID_ARGUMENT, the previous setting staying in force: n != C; a tone outside
 *                                     -1 .. T - 1; a threshold or ratio that is not finite or negative; close > open; guard or hang out of range; while
 *                                     the tones or the channel squelch are off; while a pipelined sinks batch is inside the handle.  While it is on,
 *                                     fdc_pipeline_set_tones is refused where it would switch the tones off or change T, S or W (new increments alone
 *                                     are allowed and restart both streams), and so is fdc_pipeline_set_squelch(NULL ...).  A SETTING: it applies from
 *                                     the next call and survives fdc_pipeline_reset (the state does not); it waits for the handle's own stream first.
 *                                     It allocates everything the feature needs, once: four tables of C, two state buffers, ((W - 1 + max_blocks) div W)
 *                                     C decision bytes and their pinned twin; nothing in the steady state of any entry.  A plan without channels accepts it.
 *   fdc_pipeline_tone_squelch_setting the setting in force; any pointer may be NULL; the arrays receive C elements each, guard and hang -1 while it is off.
 *   fdc_pipeline_tone_squelch         dec[nf][C] of the frames the last call completed, one byte (0 / 1) each, nblocks being that call's block count
 *                                     (as fdc_pipeline_tones); *nframes receives nf.  capacity_bytes below nf C: FDC_ERR_INVALID_ARGUMENT, nothing written.
 *                                     After a host entry it is a memcpy from the pinned twin, copied home with the levels (no copy where nf = 0); after
 *                                     a device entry it waits for the stream that one ran on.
 *   fdc_pipeline_tone_squelch_device  the device decisions, NULL while off.
 * WHILE IT IS ON fdc_pipeline_squelch and fdc_pipeline_squelch_device give the COMBINED mask (carrier AND tone), which is the mask that gates the audio
 * and feeds the pack offsets; the carrier squelch's own state is untouched by the gate.  A call's tail then runs k_chan_squelch, k_chan_demod,
 * k_chan_tones, k_tone_decide, k_tone_gate, the pack offsets and k_chan_audio in this order; the sub-batches of a long host call append their decisions
 * as the tones append their rows.  fdc_pipeline_describe: "tone squelch: pass" after a call that ran it.  With the setting off every entry launches
 * exactly the kernels it launches without this feature, in the same order.  There is no group setter. */
int fdc_pipeline_set_tone_squelch(fdc_pipeline *p, const int32_t *tone, const float *open_thr, const float *close_thr, const float *ratio, int n,
                                  int32_t guard, int32_t hang_frames);
int fdc_pipeline_tone_squelch_setting(const fdc_pipeline *p, int32_t *tone, float *open_thr, float *close_thr, float *ratio, int32_t *guard,
                                      int32_t *hang_frames);
int fdc_pipeline_tone_squelch(fdc_pipeline *p, uint8_t *dst, size_t capacity_bytes, int nblocks, int32_t *nframes);
void *fdc_pipeline_tone_squelch_device(fdc_pipeline *p);
/* The decision and the gate alone, on device buffers of the caller (and the entry the tests reach the kernels by with hand-made rows), with the handle's
 * setting (which must be on), the tones' T and W and the channel count, and nothing of its stream state: d_frames ((fill + nblocks) div W) C T float32
 * pairs, d_dec exactly that many times C bytes (both may be NULL where that is 0), d_state_in C int32 pairs (open, h) or NULL ((0, 0)), d_state_out
 * another buffer that receives exactly C int32 pairs (the state as read where the call completes no frame), d_mask exactly nblocks C bytes, ANDed in
 * place, or NULL: the decision alone.  fill: 0 .. W - 1.  Enqueued on `stream` (NULL: the handle's). */
int fdc_pipeline_tone_squelch_pass_device(const fdc_pipeline *p, const void *d_frames, void *d_dec, const void *d_state_in, void *d_state_out, void *d_mask,
                                          int32_t fill, int nblocks, void *stream);

/* Optional: pin a host range that will be handed to fdc_pipeline_work() again and again (GNU Radio's circular buffers
 * live as long as the flowgraph: register them in start(), unregister in stop()).  A call whose `in` lies in a
 * registered range is DMA'd from it in place, and when every outs[c] does, the results are stored straight into
 * them; other buffers are staged through pinned memory inside the handle.  Results are identical either way.
 * The range must stay mapped until fdc_host_unregister(ptr) (same ptr as registered). */
int fdc_host_register(void *ptr, size_t bytes);
int fdc_host_unregister(void *ptr);
void fdc_pipeline_reset(fdc_pipeline *p);    /* history <- zeros, block counter <- 0, input form unlatched (fresh ctor state)  */

/* Device-resident entry (stateless; the form bench.py and a device-side flowgraph use).
 *   d_ring      device pointer: N/R halo samples preceding the span, then nblocks*(N-N/R) new samples
 *   first_block global index of the span's first block (window phase = first_block*shift mod R)
 *   d_out       device pointer, fdc_pipeline_output_samples() samples of the handle's output format: channel c's stream of
 *               nblocks*lout_c samples starts at fdc_pipeline_channel_offset(p, c, nblocks)
 *   d_spectrum  NULL or device pointer for nblocks*N samples (needs keep_spectrum)
 *   stream      hipStream_t (NULL = the handle's own stream).  Asynchronous: returns after enqueue. */
int fdc_pipeline_process_device(fdc_pipeline *p, const void *d_ring, int64_t first_block, int nblocks,
                                void *d_out, void *d_spectrum, void *stream);
/* The same on a device ring of complex integers (format / scale as fdc_pipeline_work_iq; d_ring 4-byte aligned, the same sample counts).
 * Stateless, like fdc_pipeline_process_device: it neither checks nor latches the handle's input form. */
int fdc_pipeline_process_device_iq(fdc_pipeline *p, int32_t format, float scale, const void *d_ring, int64_t first_block, int nblocks,
                                   void *d_out, void *d_spectrum, void *stream);
/* The same, and beside the spectrum the POWER OF ITS 16-BIN GROUPS (round 6): d_group_power receives nblocks x N/16 float32, entry [m][g] = the sum
 * of |S|^2 over bins 16 g .. 16 g + 15 of block m's normalised, shifted spectrum.  At N = 16384 / 32768 / 65536 the forward kernel sums them in its
 * epilogue, while the bins are in its registers; elsewhere (other block lengths, launch groups too short for the block kernel) a pass over the
 * spectrum does.  What a sink bank's power cells are summed from (fdc_sinks_group_power / fdc_sinks_prepare_from_groups below) instead of reading the
 * spectrum back: lib/PowerActivationChannel_impl.cc:286-306, lib/activity_detection_channelizer_vcm_impl.cc:630-650 sum |X|^2 over a bin range per
 * block.  Needs d_spectrum and N a multiple of 16; d_group_power = NULL is fdc_pipeline_process_device. */
int fdc_pipeline_process_device_power(fdc_pipeline *p, const void *d_ring, int64_t first_block, int nblocks, void *d_out, void *d_spectrum,
                                      void *d_group_power, void *stream);
int fdc_pipeline_synchronize(fdc_pipeline *p);
void *fdc_pipeline_stream(fdc_pipeline *p);  /* the handle's hipStream_t */
/* The one-block-per-compute-unit kernels are persistent: one workgroup per unit, all of its LDS.  A consumer that wants to run other
 * kernels BESIDE them (the sinks' look-ahead form, fdc_sinks_spectrum_ahead) asks for n units to be left out: the block kernels then
 * launch on (units - n) workgroups.  Returns that number — launch groups should hold a multiple of it in blocks, or the last round of
 * the persistent loop runs part of the machine — or a negative fdc_status.  n = 0 restores the default. */
int fdc_pipeline_reserve_compute_units(fdc_pipeline *p, int32_t n);
int32_t fdc_pipeline_chunk_blocks(const fdc_pipeline *p);   /* blocks per internal launch group */
/* Which kernels a process call without spectrum output runs: 0 = generic LDS Stockham kernels (any size),
 * 1 = spectrum in memory at N = 16384 / 32768 / 65536 (forward transform by the block kernel in one launch, ms[0]; channel kernels
 * ms[2]), 2 = uniform-plan path (all channels
 * l = 256 on the 256-bin grid: stage 1 = column FFT + window + IFFT, stage 2 = FFT across slots; timing
 * slots ms[0], ms[1] then hold stage 1 and stage 2 and ms[2] = 0), 3 = the uniform plan at N = 65536, R = 2 as ONE
 * kernel (one block per compute unit, nothing between the input rows and the output samples touches memory;
 * ms[0] = that kernel, ms[1] = ms[2] = 0).  Path 3 is every plan that is a line-up of up to FOUR BANKS, one block-kernel launch each: a bank is a
 * set of channels of one width l in {64, 128, 256, 512, 1024} on one grid f = l*slot + r with one window (l = 256: any r; 512 / 1024: r = 0 or l/2; 128 /
 * 64: r a multiple of l/4), banks of different widths may stand side by side (round 5), at N = 16384 / 32768 / 65536 (2 / 4 / 8 passes of the same kernels),
 * R = 2 or 4.  4 = a SPLIT plan at any of those three block lengths: the banks take path 3 (ms[0]), the rest — widths without a block kernel, odd offsets,
 * a fifth bank, banks the cost rule sends back — take the spectrum path on a partial spectrum that holds only what they read (forward transform ms[1], channel
 * kernels ms[2]).  Which it is, the cost rule decides (csrc/fdc_plan_cost.hpp: measured constants per launch and per band read; a plan goes to path 1 whole
 * when the sum says so); fdc_pipeline_describe / fdc_pipeline_plan_preview say what was chosen.
 * 5 (round 6) = N = 4096 — the block length of the reference's example flowgraph — in ONE launch (csrc/fdc_fused4096.hip; ms[0]): forward transform, channel
 * slices, windows and inverse transforms with the spectrum in LDS, nothing but the new input samples and the output samples crosses the memory interface.
 * Every plan of channels 16 ... 1024 bins wide (any offsets, windows, overlaps between them) of at least 512 and — about — at most 4096 bins in total
 * (exactly: the rows of a pair of blocks fit eight waves — two rows of 1024 bins, four of 512, eight of 256 or less per wave — and the two spectrum tiles);
 * a call that asks for the spectrum runs path 0 on the same handle.  FDC_PIPE_NO_FUSED / FDC_PIPE_NO_POLY: paths 0 / 2 as before (FDC_PIPE_WIDE_UNIFORM: path 5 for
 * plans under 512 bins too, which the two launches run a few per cent faster).  plan_preview: every channel -1.  The kernel takes one block per workgroup
 * where no channel is wider than 256 bins and a pair of blocks where one is (fdc_pipeline_describe says which). */
int32_t fdc_pipeline_path(const fdc_pipeline *p);
/* The same in words, for logs: which kernels the handle's plan was given ("N = 65536, R = 2, 512 channels; path 3: k_blknar, l = 128, bank of 511 half a
 * channel off the grid + bank of 1 on the grid (two launches)").  Writes at most n bytes including the terminator; returns the untruncated length, -1 for
 * bad arguments.  (No counterpart in the reference, which has one implementation.) */
int32_t fdc_pipeline_describe(const fdc_pipeline *p, char *buf, int32_t n);
/* What fdc_pipeline_create WOULD choose for cfg, without a device (round 5: the plan selector — csrc/fdc_api.hip classify_plan, the measured constants of
 * csrc/fdc_plan_cost.hpp — is host code): returns the path number (as fdc_pipeline_path; the block kernels are those of an MI355X), writes the description
 * (as fdc_pipeline_describe) into buf if given, and into assignment[c], if given (nchannels entries), where channel c goes: k >= 0 = bank k (one block-kernel
 * launch each, in launch order; path 2: the one bank of the two-launch form), -1 = the spectrum path (a split plan's remainder, or the whole plan),
 * -2 - c0 = a copy of channel c0's output (same slice, same window).  Negative return: the status fdc_pipeline_create would give for the arguments. */
int fdc_pipeline_plan_preview(const fdc_pipeline_cfg *cfg, char *buf, int32_t n, int32_t *assignment);

/* Timing of the kernels with HIP events recorded on the stream they are launched on (bench.py's
 * roofline leg).  While enabled, every process_device call brackets its launches with events; the readout
 * synchronises on them, sums all launch groups since enable / the previous readout and clears them:
 * ms[0] forward FFT pass A, ms[1] forward FFT pass B (or the single-pass kernel), ms[2] fused channel
 * kernel(s), ms[3] = number of launch groups summed (each group = one chunk of fdc_pipeline_chunk_blocks
 * blocks, the last of a call possibly shorter).  Needs n >= 4; returns the number of entries written. */
/* enable: 0 = off, 1 = every launch group, k > 1 = every k-th launch group (a sample: the event packets between the
 * kernels cost 7-17 us per group on MI355X, enough to show in the throughput of the region they time) */
int fdc_pipeline_enable_timing(fdc_pipeline *p, int enable);
int fdc_pipeline_last_kernel_ms(fdc_pipeline *p, float *ms, int n);

/* ------------------------------------------------------------------------------------------------
 * Multi-device handle: the same chain behind ONE work() — what the FrequencyDomainChannelizer hier block is to the scheduler
 * (python/FrequencyDomainChannelizer.py:283-315: one block, one work() thread) — spread over several GPUs of the node.  A call
 * of nblocks items is cut into contiguous spans, one per member device; every member copies its span's samples over its own
 * PCIe link (the halo of a span is the N/R samples in front of it in the caller's buffer; the first span's halo is the history
 * the group keeps), runs the kernels with the span's global first-block index and writes its results into the caller's
 * per-channel buffers at the span's block offset, all members concurrently.  No collective and no device-to-device traffic:
 * spans are independent given halo and block index.  Results are those of one handle fed the same stream
 * (bit for bit when the members run the kernels one handle would run: tests/test_group_gpu.py).
 * The reference's own parallelism inside one work(): 4 FFTW threads (python/...:206), one std::thread per segment / per
 * detected channel (lib/activity_detection_channelizer_vcm_impl.cc:293-304, :339-371).
 *   cfg              as for fdc_pipeline_create; device_id is ignored, max_blocks is the largest nblocks of a GROUP call
 *   devices[n]       HIP device ordinal of each member; an ordinal may appear more than once (virtual members on one GPU)
 *   min_span_blocks  a member is not given fewer blocks than this, so short calls use fewer members (0 = default 8)
 * One thread at a time per group, like every handle.  A call that fails on some member leaves the group unusable until
 * fdc_pipeline_group_reset() (the other members' spans of that call were written).
 * ---------------------------------------------------------------------------------------------- */
typedef struct fdc_pipeline_group fdc_pipeline_group;
int fdc_pipeline_group_create(const fdc_pipeline_cfg *cfg, const int32_t *devices, int ndevices, int min_span_blocks,
                              fdc_pipeline_group **out);
void fdc_pipeline_group_destroy(fdc_pipeline_group *g);
/* work()-shaped, same arguments and state semantics as fdc_pipeline_work() / fdc_pipeline_work_real(); outs[c] in the group's output format */
int fdc_pipeline_group_work(fdc_pipeline_group *g, const void *in, int nblocks, void *const *outs, void *spectrum);
int fdc_pipeline_group_work_real(fdc_pipeline_group *g, const void *in, int nblocks, void *const *outs, void *spectrum);
/* complex integer input: the arguments, the bytes and the input-form latch of fdc_pipeline_work_iq (the group latches, as its members do) */
int fdc_pipeline_group_work_iq(fdc_pipeline_group *g, int32_t format, float scale, const void *in, int nblocks, void *const *outs, void *spectrum);
void fdc_pipeline_group_reset(fdc_pipeline_group *g);           /* history <- zeros, block counter <- 0, input form unlatched, error state cleared */
/* complex integer output for every member (fdc_pipeline_set_output_format: the same arguments, refusals and setting semantics).  A group call takes
 * the members' own setting and refuses (FDC_ERR_INVALID_ARGUMENT) when members set one by one through fdc_pipeline_group_member disagree. */
int fdc_pipeline_group_set_output_format(fdc_pipeline_group *g, int32_t format, float scale);
/* fine tuning for every member (fdc_pipeline_set_fine_tuning: the same arguments, refusals and setting semantics); the spans carry their global block
 * index, so a group's output is one handle's */
int fdc_pipeline_group_set_fine_tuning(fdc_pipeline_group *g, const double *nu, int n);
/* channel levels for every member (fdc_pipeline_set_levels: the same argument, refusals and setting semantics), and the levels of the last group call:
 * the members' spans (fdc_pipeline_group_last_spans) put together in block order, nblocks*C*2 floats with the bits one handle gives for the same call;
 * nblocks must be that call's block count (FDC_ERR_INVALID_ARGUMENT otherwise, while levels are off and before any call) */
int fdc_pipeline_group_set_levels(fdc_pipeline_group *g, int32_t on);
int fdc_pipeline_group_levels(fdc_pipeline_group *g, float *dst, int nblocks);
/* the channel lag-1 correlation for every member (fdc_pipeline_set_lag1), and that of the last group call, put together as the levels are */
int fdc_pipeline_group_set_lag1(fdc_pipeline_group *g, int32_t on);
int fdc_pipeline_group_lag1(fdc_pipeline_group *g, float *dst, int nblocks);
/* channel gains for every member (fdc_pipeline_set_gains: the same arguments, refusals and setting semantics) */
int fdc_pipeline_group_set_gains(fdc_pipeline_group *g, const float *gain, int n);
int32_t fdc_pipeline_group_size(const fdc_pipeline_group *g);
fdc_pipeline *fdc_pipeline_group_member(fdc_pipeline_group *g, int i);   /* owned by the group (fdc_pipeline_path, sizes, timing) */
int32_t fdc_pipeline_group_device(const fdc_pipeline_group *g, int i);
int32_t fdc_pipeline_group_member_max_blocks(const fdc_pipeline_group *g);   /* the longest span a member can be given */
/* Host placement (round 6).  A group's worker thread for member i — the thread that copies the member's span over its PCIe link — pins itself
 * to the CPUs of the NUMA node its device hangs off (/sys/bus/pci/devices/<bdf>/numa_node, /sys/devices/system/node/node<k>/cpulist,
 * intersected with the process's own mask; member 0 runs on the calling thread, which is never touched: pin the scheduler thread of the
 * block yourself if you want it placed).  Pinned staging comes from the host pool closest to the member's device whatever thread asks
 * (hipHostMalloc without hipHostMallocNumaUser).  Best effort: unknown node (-1: single-node machines, most containers) = left alone.
 *   fdc_device_numa_node(d)                 the node of HIP device d, -1 if unknown or no such device
 *   fdc_selftest_worker_placement(node,..)  starts a worker exactly as a group would for a member on `node` and checks the mask it runs
 *                                           under: 1 = pinned inside the node's CPUs, 0 = left alone under the process's mask (node unknown
 *                                           or none of its CPUs usable), negative = failure; the two counts are the node's usable CPUs and the
 *                                           worker's.  Needs no device (tests/test_abi_cpu.py). */
int fdc_device_numa_node(int device_id);
int fdc_selftest_worker_placement(int node, int32_t *cpus_of_node, int32_t *cpus_of_worker);
/* the spans of the last call: first_block[i] (global index) and nblocks[i] (0 = member idle) for i < min(size, cap); returns size */
int fdc_pipeline_group_last_spans(const fdc_pipeline_group *g, int64_t *first_block, int32_t *nblocks, int cap);

/* ------------------------------------------------------------------------------------------------
 * Stateful sinks fed with the normalised spectrum (what the hier block connects to normalize_input,
 * python/FrequencyDomainChannelizer.py:301-312): a bank of
 *   gr::FDC::PowerActivationChannel::make(blocklen, cfreq, bw, relinvovl, thresh, maxblocks, deactivation_delay,
 *        msg, fileoutput, path, verbose, ID)                       — include/FDC/PowerActivationChannel.h:49
 * instances and the segments of one
 *   gr::FDC::activity_detection_channelizer_vcm::make(blocklen, segments, thresh, relinvovl, maxblocks, message,
 *        fileoutput, path, threads, minchandist, channel_deactivation_delay, window_flank_puffer, verbose)
 *                                                                  — include/FDC/activity_detection_channelizer_vcm.h:49
 * sharing ONE device-resident spectrum.  Power sums and extractions (window, half swap, inverse FFT, overlap discard)
 * run on the GPU for a whole batch; the per-block decisions run on the host (lib/PowerActivationChannel_impl.cc:137-306,
 * lib/activity_detection_channelizer_vcm_impl.cc:542-841).  What the reference publishes as pmt PDUs
 * (dict + c32vector, …vcm_impl.cc:415-430, PowerActivationChannel_impl.cc:222-233) comes back as POD records that the
 * C++ face turns into pmt; `msg`, `fileoutput`, `path`, `verbose` and `threads` stay with that face.
 * create() fails with FDC_ERR_INVALID_ARGUMENT exactly where the reference constructors throw.
 * Failure: the blocks are stateful and a batch advances that state on the device as it goes (block counter, channel state
 * machines, buffered blocks, the two-deep submission).  A work / submit / flush call that fails after it has started to do so
 * (a HIP error, out of memory while growing a landing buffer) cannot be rolled back or repeated: the handle is DEAD from then
 * on — every later work / submit / flush returns FDC_ERR_HIP naming the first failure, PDUs of the failed call are not handed
 * out (none twice, none with a wrong payload) — and must be destroyed.  Argument errors (a count out of range, a null buffer,
 * work_device while a batch is in flight) are refused before anything moves and leave the handle usable.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fdc_sinks fdc_sinks;
typedef struct { float cfreq, bw; int32_t id; } fdc_pac_cfg;           /* INTERNAL frequency units, [0,1) */
typedef struct { float start, stop; } fdc_segment_cfg;                 /* INTERNAL frequency units        */
typedef struct {
    int32_t device_id, blocklen, relinvovl;
    int32_t npac; const fdc_pac_cfg *pac;
    float pac_thresh_db; int32_t pac_maxblocks, pac_deactivation_delay;
    int32_t nseg; const fdc_segment_cfg *seg;
    float det_thresh_db; int32_t det_maxblocks; float minchandist; int32_t det_deactivation_delay;
    double window_flank_puffer;
    int32_t max_blocks;                                                /* largest batch of one work call  */
    int32_t det_variant;   /* 0 = activity_detection_channelizer_vcm (all segments in one block); 1 = one
                              gr::FDC::SegmentDetection::make(ID, blocklen, relinvovl, seg_start, seg_stop, thresh,
                              minchandist, window_flank_puffer, maxblocks_to_emit, channel_deactivation_delay, …)
                              (include/FDC/SegmentDetection.h:49) per segment, ID = segment index — the twin the hier
                              block instantiates (python/FrequencyDomainChannelizer.py:261-278): its own segment geometry,
                              raw power sums, block counter from 0, partial emission after all channels */
    int32_t verbose;       /* the blocks' `verbose` argument (lib/PowerActivationChannel_impl.h:46-50): 0 = no log, 1 = to
                              stdout, 2 = to the reference's log files in the working directory — gr-FDC.PowActChan.<ID>.log
                              (PowerActivationChannel_impl.cc:54), gr-FDC.ActDetChan.log (…vcm_impl.cc:94),
                              gr-FDC.ActDetChan.ID_<n>.log (SegmentDetection_impl.cc:51); same lines: the derived geometry at
                              construction, one line per emitted PDU */
    int32_t det_id;        /* det_variant 1 with ONE segment: SegmentDetection's ID argument (names the log file and the
                              segment in the message IDs); < 0 = the segment index */
    int32_t flags;         /* FDC_SINKS_* bits, 0 = defaults */
    int32_t threads;       /* host engine only: worker threads of the decision phase (0 = chosen from the bank's size) */
    int32_t seg_id_base;   /* segment i of this bank is segment seg_id_base + i of the block it belongs to (the number in the message
                              IDs, fdc_pdu.source and the log lines): a bank that holds part of a block's segments — a member of an
                              fdc_sinks_group — still names them as the reference does; 0 for a whole block */
} fdc_sinks_cfg;
/* fdc_sinks_cfg.flags.  A bank runs on one of two engines.  DEVICE (default): the work() loops of the blocks
 * (lib/PowerActivationChannel_impl.cc:146-170, lib/activity_detection_channelizer_vcm_impl.cc:551-568) are device kernels —
 * per-channel state machines, edge detection and matching, the layout of the emitted payloads — so a batch is enqueued without a
 * host round trip and only finished PDUs cross PCIe.  HOST: the same decisions on host threads between two GPU phases (round 1/2
 * form); taken for verbose != 0 (the log lines are written while the decisions are made), for detection segments of more than
 * 1024 power cells, and on request.  Both engines emit the same PDUs in the same order (tests/test_sinks_gpu.py). */
enum {
    FDC_SINKS_HOST_DECISIONS = 1,   /* use the host engine */
    FDC_SINKS_DEVICE_PAYLOAD = 2,   /* device engine: fdc_pdu.samples are DEVICE pointers (no payload copy to the host); valid like
                                       the host pointers, until the next-but-one batch is submitted */
    FDC_SINKS_LOOKAHEAD = 4         /* a second spectrum buffer and a fill stream: the producer writes batch n + 1 while the bank decides
                                       batch n (fdc_sinks_spectrum_ahead / fdc_sinks_fill_stream / fdc_sinks_prepare, below) */
};
typedef struct {
    int32_t kind;        /* 0 = PowerActivationChannel, 1 = detected channel of a segment                       */
    int32_t source;      /* PAC: its ID argument; detection: segment index, or det_id where a SegmentDetection bank was given one                                    */
    int32_t chan_id;     /* the running number inside the ID string: PAC finished_channels at activation
                            (…PowActChan.<ID>.<n>), detection: channel counter of the segment (…DETECTED.<seg>.<n>) */
    int32_t finalized, part, has_part;   /* has_part: whether the dict carries "part" (…vcm_impl.cc:419-420)   */
    double rel_bw, rel_cfreq;
    int64_t blockstart, blockend, vectorstart, vectorend;   /* vectorstart/end are in the dict for detection only */
    int64_t nsamples;
    const void *samples; /* nsamples items of the bank's payload format (fdc_sinks_set_payload_format: complex float32 by default,
                            sc16 or sc8), owned by the handle until its next work call; a device pointer under FDC_SINKS_DEVICE_PAYLOAD */
    char id[72];         /* the message ID the reference builds when the channel is ACTIVATED:
                            "<YYYY-mm-dd-HH-MM-SS>.PowActChan.<ID>.<n>" (PowerActivationChannel_impl.cc:308-312; the dict and
                            the file name append ".fin" / ".part" / ".parted.<k>", :224, :237) and
                            "<YYYY-mm-dd-HH-MM-SS>.DETECTED.<seg>.<n>" (…vcm_impl.cc:526-530); local time, all PDUs of one
                            activation carry the same string */
} fdc_pdu;

/* Log lines of the sinks (verbose != 0) additionally go to this callback when one is set (process-wide; NULL = off). */
typedef void (*fdc_log_fn)(const char *line, void *user);
void fdc_set_log_callback(fdc_log_fn fn, void *user);

/* Same, for a hier block fed with items that are ALREADY transformed (inpveclen = blocksize: the front end is skipped,
 * python/FrequencyDomainChannelizer.py:201, :284-290): nblocks unnormalised, fftshifted spectrum items in; the 1/N of
 * multiply_const_cc (:213-216), the channel branches and, if given, the sinks run on the device.  sinks may be NULL. */
int fdc_pipeline_work_spectrum(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum,
                               fdc_sinks *sinks);
int fdc_sinks_create(const fdc_sinks_cfg *cfg, fdc_sinks **out);
/* The whole hier block in one call: fdc_pipeline_work() whose spectrum lands directly in the sinks' device buffer,
 * followed by the sinks' work on it (python/FrequencyDomainChannelizer.py:283-312).  The pipeline needs keep_spectrum,
 * the same blocklen/device as the sinks and nblocks <= the sinks' max_blocks.
 * Two forms, chosen by the BANK:
 *  - a bank without FDC_SINKS_LOOKAHEAD (default): front end, then the sinks, inside the call; fdc_sinks_pdu*() afterwards give the PDUs
 *    the reference's blocks would have published for exactly these items (the reference's item-by-item behaviour, whatever the batch);
 *  - a bank created with FDC_SINKS_LOOKAHEAD: PIPELINED (round 6).  In the reference the front end and every sink are blocks of one
 *    flowgraph that GNU Radio's thread-per-block scheduler runs side by side (python/FrequencyDomainChannelizer.py:237-278); here one call
 *    copies and transforms ITS items into the bank's next-batch buffer on the bank's fill stream (power cells behind them), submits the
 *    batch the call BEFORE left there (fdc_sinks_submit_device: decision chains beside this call's copy and transform, then extractions)
 *    and hands out the PDUs of the batch before that one, whose payload copy ran meanwhile.  The call returns when its input has left the
 *    caller's buffer (and its stream outputs / debug spectrum, if any, have arrived): with pinned input and no stream outputs it costs what
 *    its input copy costs.  fdc_sinks_pdu*() after call n give the PDUs of the items of call n - fdc_pipeline_sinks_latency() (2 on the
 *    device engine, 1 on the host engine; none for the first calls) — same PDUs, same order, same bits as the serial form, later.
 *    fdc_pipeline_flush_sinks() hands out what is still inside: call it until it returns 0 when the stream ends (the block's stop()).
 *    The persistent forward kernel leaves ncu/8 compute units to the bank's chains when a call is long enough to take it through two
 *    rounds (fdc_pipeline_reserve_compute_units overrides).  Between the first pipelined call and the last flush the bank belongs to the
 *    pipeline: no fdc_sinks_work*() / submit / prepare on it from elsewhere; flush before destroying either handle
 *    (fdc_pipeline_reset resets the front end only — history and block counter; a batch already transformed into the bank stays there and its PDUs
 *    come out with the next call or a flush: the sink blocks keep their own state, as separate blocks do).  A pipelined call that fails after it has
 *    advanced the stream state (history, block counter, the bank's buffers: a HIP error, a dead bank) cannot be repeated or skipped: every later
 *    fdc_pipeline_work_sinks / fdc_pipeline_flush_sinks on that pipeline returns FDC_ERR_HIP — destroy both handles (as for a dead bank, below). */
int fdc_pipeline_work_sinks(fdc_pipeline *p, const void *in, int nblocks, void *const *outs, void *spectrum,
                            fdc_sinks *sinks);
/* Pipelined form: submits / finishes the oldest batch still inside and makes its PDUs the bank's current ones; returns its block count,
 * 0 when nothing is left (serial form: always 0), or a negative fdc_status. */
int fdc_pipeline_flush_sinks(fdc_pipeline *p, fdc_sinks *sinks);
/* How many calls later the PDUs of a call's items are handed out: 0 (serial form), 1 or 2 (pipelined; see above); -1 for a null handle. */
int32_t fdc_pipeline_sinks_latency(const fdc_pipeline *p, const fdc_sinks *sinks);
void fdc_sinks_destroy(fdc_sinks *s);
/* work()-shaped: nitems normalised-spectrum items of blocklen samples each on the host; returns nitems */
int fdc_sinks_work(fdc_sinks *s, const void *spectrum, int nitems);
/* the same when only the bins [bin_lo, bin_hi) of every item are needed by this bank's channels and segments: only those columns
 * cross PCIe (one strided copy), the rest of the device-side items keeps whatever it held.  The caller answers for the band covering
 * every bin the bank reads (fdc_sinks_read_band gives it); what an fdc_sinks_group member is fed with. */
int fdc_sinks_work_band(fdc_sinks *s, const void *spectrum, int nitems, int32_t bin_lo, int32_t bin_hi);
/* [lo, hi): every bin this bank can ever read — the measure and extract ranges of its PowerActivationChannels, its segments widened by
 * the widest extraction a detected channel can get (lib/activity_detection_channelizer_vcm_impl.cc:575-607: the next power of two above
 * width * (1 + 2 * window_flank_puffer), centred on the channel, clamped to the block) */
int fdc_sinks_read_band(const fdc_sinks *s, int32_t *lo, int32_t *hi);
/* device-resident: the producer (fdc_pipeline_process_device with d_spectrum = fdc_sinks_spectrum(s)) has written
 * nblocks spectra there on a stream it has synchronised; no PCIe traffic for the spectrum */
void *fdc_sinks_spectrum(fdc_sinks *s);
void *fdc_sinks_stream(fdc_sinks *s);
int32_t fdc_sinks_blocklen(const fdc_sinks *s);     /* N the bank was created for                                  */
int32_t fdc_sinks_max_blocks(const fdc_sinks *s);   /* capacity of its device-resident spectrum buffer, in blocks   */
int fdc_sinks_work_device(fdc_sinks *s, int nblocks);
/* Two-deep form of fdc_sinks_work_device for a producer that keeps the device busy: submit() enqueues the batch that sits in
 * the spectrum buffer and, if an earlier batch is still in flight, finishes that one first (waits for its payload copy, builds its
 * PDUs) while the device works on the new one.  Returns the number of blocks of the batch whose PDUs are readable now through
 * fdc_sinks_pdu*() (0 = none yet), or a negative fdc_status.  flush() finishes the batch in flight (returns its block count, 0 if
 * there was none).  The spectrum buffer may be overwritten by work enqueued on fdc_sinks_stream() as soon as submit() returns.
 * fdc_sinks_work_device(s, n) == submit(s, n) + flush(s); it refuses to run while a submitted batch is in flight.
 * PDUs (and their payload pointers) stay valid until the next submit / flush / work call on the handle. */
int fdc_sinks_submit_device(fdc_sinks *s, int nblocks);
int fdc_sinks_flush(fdc_sinks *s);
int32_t fdc_sinks_engine(const fdc_sinks *s);       /* 0 = host decisions, 1 = device decisions */
/* PAYLOAD FORMAT: fdc_pdu.samples as sc16 / sc8, narrowed on the device before they leave it (the payload copy over PCIe is what bounds a bank
 * whose PDUs land in host memory: sc16 halves its bytes, sc8 quarters them).  A setting of the bank like fdc_pipeline_set_output_format, and its rule:
 *   format   FDC_OQ_FC32 (default), FDC_OQ_SC16 (int16 I, int16 Q interleaved: 4 bytes per sample) or FDC_OQ_SC8 (int8: 2 bytes)
 *   scale    float32; zero or not finite: FDC_ERR_INVALID_ARGUMENT (negative is allowed)
 * Each component of each payload sample y (exactly what the bank emits in FC32) becomes saturate(round_half_even(float32(y * scale))), the product
 * rounded once and kept out of FMA contraction; NaN -> 0, +-Inf -> the limits.  fdc_pdu keeps its layout: nsamples stays a sample count, samples
 * points at nsamples items of the format (host memory, or device memory under FDC_SINKS_DEVICE_PAYLOAD).
 * The setting does not touch the channel state machines, the buffered blocks or the block counter: blocks buffered in live channels across batches
 * stay complex float on the device and are narrowed when their PDU goes out, so a PDU collected over several batches (and over a change of the
 * format) has the bits of the narrowed float PDU.
 * Refused with FDC_ERR_INVALID_ARGUMENT, nothing changed: a null handle, an unknown format, a bad scale; a batch submitted, prepared (ahead) or in
 * flight (fdc_sinks_flush first); a pipelined fdc_pipeline_work_sinks that still holds batches of the bank (fdc_pipeline_flush_sinks first).
 * Refused with FDC_ERR_UNSUPPORTED: any format but FC32 on a bank that runs the HOST engine (FDC_SINKS_HOST_DECISIONS, verbose != 0, segments of more
 * than 1024 cells): it assembles payloads on the host from float landing runs; narrowing there is out of scope.
 * A successful call drops the bank's current PDUs (fdc_sinks_pdu_count == 0): every PDU a caller can see is in the format the bank reports.
 * Two routes, chosen per batch (fdc_sinks_payload_route: of the last finished batch; 0 = float, 1 = narrowed, 2 = fused):
 *   fused      every extraction of the batch is of the 256-bin class (a bank of 256-bin PowerActivationChannels): the extraction kernel and the move of
 *              the buffered blocks store the emitted runs narrow themselves; the float landing buffer holds the buffered rests only
 *              (a batch without extractions: fused on a bank that holds nothing but 256-bin PowerActivationChannels, narrowed on any other)
 *   narrowed   any mix of width classes: the batch runs as in FC32, then one pass narrows the emitted runs in front of the payload copy
 * The narrow landing buffers (device, and pinned host unless FDC_SINKS_DEVICE_PAYLOAD) grow by the rule of the float ones; nothing else is allocated. */
int fdc_sinks_set_payload_format(fdc_sinks *s, int32_t format, float scale);
int fdc_sinks_payload_format(const fdc_sinks *s, int32_t *format, float *scale);   /* both out-pointers are required */
int32_t fdc_sinks_payload_route(const fdc_sinks *s);                               /* -1 for a null handle */
/* Look-ahead (banks created with FDC_SINKS_LOOKAHEAD; round 5).  The decision kernels of a batch are chains — one wave per
 * PowerActivationChannel, one workgroup per detection segment (lib/activity_detection_channelizer_vcm_impl.cc:741-841 is sequential over
 * blocks and channels) — that leave the device idle, and the host has to see their summary before it can size the extraction launches.
 * With two spectrum buffers the producer fills batch n + 1 beside them:
 *     fill(fdc_sinks_spectrum(s)) on fdc_sinks_fill_stream(s)                                 batch 0   (a look-ahead bank is filled on the fill stream only)
 *     loop:  fill(fdc_sinks_spectrum_ahead(s)) on fdc_sinks_fill_stream(s)                    batch n + 1   (never on fdc_sinks_stream)
 *            fdc_sinks_prepare(s, nblocks, 1)                          its power cells behind the fill, and the mark "batch n + 1 complete"
 *            fdc_sinks_submit_device(s, nblocks)                       batch n; afterwards fdc_sinks_spectrum(s) names batch n + 1's buffer
 * fdc_sinks_spectrum(s) is always the buffer the NEXT submit / work call reads; it alternates between the two, so ask again for every
 * batch.  The bank orders the streams itself: a submit waits for the mark fdc_sinks_prepare left behind ITS batch on the fill stream (not for
 * what the producer has enqueued there since: that is what runs beside the decisions) — without a prepare of the same block count, for
 * everything enqueued on the fill stream so far, which is correct and overlaps nothing; work enqueued on the fill stream after a submit
 * has returned waits until the batch before that submit's has been read for the last time.  The producer should
 * leave a few compute units free for the chains (fdc_pipeline_reserve_compute_units): the block kernels are persistent and fill every
 * unit's LDS.  Without the flag: spectrum_ahead and fill_stream return null, prepare refuses.
 * fdc_sinks_prepare(s, n, ahead): power cells of the n blocks in fdc_sinks_spectrum_ahead (ahead = 1) or fdc_sinks_spectrum (0) on the
 * fill stream; the submit of that batch then skips them if its block count is n.
 * Round 6: a batch prepared AHEAD is committed.  The submit in front of it, once it has placed its own tasks, enqueues the prepared batch's decision
 * chain at once (device engine) instead of when the caller returns with the next submit — the chain is the long pole of a detector's step and used
 * to start a host lap late — so the next submit / work_device call must be for exactly that batch (another block count: FDC_ERR_INVALID_ARGUMENT and the
 * handle is dead); fdc_sinks_work / work_band / a second prepare of the current buffer are refused until it has been submitted.  The extraction
 * streams run at the device's highest stream priority (own hardware queues: at equal priority they shared one with the fill stream and sat behind the
 * next batch's forward kernel). */
void *fdc_sinks_spectrum_ahead(fdc_sinks *s);
void *fdc_sinks_fill_stream(fdc_sinks *s);
int fdc_sinks_prepare(fdc_sinks *s, int nblocks, int ahead);
/* Power cells WITHOUT a pass over the spectrum (round 6).  fdc_sinks_group_power(s) / fdc_sinks_group_power_ahead(s): device buffers of max_blocks x N/16
 * float32 that go with fdc_sinks_spectrum(s) / fdc_sinks_spectrum_ahead(s) (they swap together; NULL for a bank without cells or N < 16): the producer
 * hands them to fdc_pipeline_process_device_power as d_group_power.  fdc_sinks_prepare_from_groups(s, n, ahead) then sums every cell from the groups
 * inside it plus the bins of the (at most two) groups it cuts, and marks the batch like fdc_sinks_prepare: the submit / work call of n blocks that follows
 * skips its own power pass.  ahead = 0 also on banks without FDC_SINKS_LOOKAHEAD (on the bank's stream).  The cells' float sums are formed in another
 * order than k_cell_power forms them (last bits); the PDUs' payloads do not depend on them.  fdc_pipeline_work_sinks does all of this itself. */
void *fdc_sinks_group_power(fdc_sinks *s);
void *fdc_sinks_group_power_ahead(fdc_sinks *s);
int fdc_sinks_prepare_from_groups(fdc_sinks *s, int nblocks, int ahead);
/* PDUs emitted by the last work call, in emission order */
int fdc_sinks_pdu_count(const fdc_sinks *s);
int fdc_sinks_pdu(const fdc_sinks *s, int i, fdc_pdu *out);
/* all of them at once: fills out[0 .. min(count, cap)) and returns the count.  Every payload is one contiguous run of a pinned
 * buffer of the handle (device engine: always; host engine: when all blocks of the PDU come from the last call). */
int fdc_sinks_pdus(const fdc_sinks *s, fdc_pdu *out, int cap);
/* for every PDU of the last call, the index (inside that call) of the item at which the block emitted it: what orders the PDUs of
 * several banks that saw the same items (fdc_sinks_group) the way one bank orders its own; returns the PDU count */
int fdc_sinks_pdu_emit_items(const fdc_sinks *s, int32_t *item, int cap);
/* the same, and for every PowerActivationChannel PDU the index of its channel in THIS bank's cfg->pac[] (-1 for a detection): a group that hands
 * its members the bank's channels in frequency order puts their PDUs back into the bank's own order with it (either array may be NULL) */
int fdc_sinks_pdu_emit_order(const fdc_sinks *s, int32_t *item, int32_t *pac, int cap);
/* derived geometry (for logs and tests): v[8] = extract_start, extract_stop, extract_width, measure_start,
 * measure_stop, output_len, output_ovl_offset, deltaphase;  v[5] = start, stop, width, decimation, power cells */
int fdc_sinks_pac_params(const fdc_sinks *s, int i, int32_t *v8);
int fdc_sinks_segment_params(const fdc_sinks *s, int i, int32_t *v5);

/* ------------------------------------------------------------------------------------------------
 * The sink blocks over several devices ("shard by channel / by segment").  A sink block's input is the
 * stream of normalised spectrum items (512 KiB each at N = 65536): fed from host memory, ONE device is bound by its PCIe link
 * long before its kernels matter (1024 items: 9.6 ms of copy, 0.5 ms of kernels).  The group cuts the bank BY FREQUENCY: the
 * PowerActivationChannels sorted by centre frequency (round 5: whatever order cfg->pac[] lists them in; the PDUs come back in the
 * bank's own order) and the segments as listed (their numbers in the message IDs are their places in cfg->seg[]: list them by
 * frequency), in runs of equal counts, one run per member device.  Every
 * member copies only the band of bins its run reads (fdc_sinks_work_band) over its own link and runs its state machines and
 * extractions on it, all members concurrently; their PDUs are merged into the order ONE bank emits them in (item by item:
 * PowerActivationChannels in bank order, then the segments in order).  Every channel / segment lives on exactly one member, so
 * no state is shared and nothing is exchanged between devices.  Same PDUs as one bank on one device, payload bits included
 * (tests/test_group_gpu.py).  The reference's counterpart: one std::thread per segment and per detected channel
 * (lib/activity_detection_channelizer_vcm_impl.cc:293-304, :339-371), one scheduler thread per PowerActivationChannel block.
 *   cfg       as for fdc_sinks_create; device_id is ignored; max_blocks = items per call, for every member
 *   devices   HIP ordinals, repeats allowed (virtual members)
 * One thread at a time per group.  PDUs (and payload pointers) stay valid until the next work call on the group. */
typedef struct fdc_sinks_group fdc_sinks_group;
int fdc_sinks_group_create(const fdc_sinks_cfg *cfg, const int32_t *devices, int ndevices, fdc_sinks_group **out);
void fdc_sinks_group_destroy(fdc_sinks_group *g);
int fdc_sinks_group_work(fdc_sinks_group *g, const void *spectrum, int nitems);      /* like fdc_sinks_work */
int fdc_sinks_group_pdu_count(const fdc_sinks_group *g);
int fdc_sinks_group_pdus(const fdc_sinks_group *g, fdc_pdu *out, int cap);           /* like fdc_sinks_pdus */
int32_t fdc_sinks_group_size(const fdc_sinks_group *g);
fdc_sinks *fdc_sinks_group_member(fdc_sinks_group *g, int i);                        /* owned by the group; NULL for a member without work */
/* member i: its device, the band [lo, hi) of bins it copies, how many PowerActivationChannels and segments it holds */
int fdc_sinks_group_member_info(const fdc_sinks_group *g, int i, int32_t *device, int32_t *lo, int32_t *hi, int32_t *npac, int32_t *nseg);
/* fdc_sinks_set_payload_format on every member (all or none: a member on the host engine refuses sc16 / sc8 for the whole group); drops the group's PDUs */
int fdc_sinks_group_set_payload_format(fdc_sinks_group *g, int32_t format, float scale);

/* ------------------------------------------------------------------------------------------------
 * Single-block faces (same arithmetic as the fused pipeline, one reference block each).
 * ---------------------------------------------------------------------------------------------- */
/* gr::FDC::overlap_save::make(itemsize, outputlen, overlaplen) — include/FDC/overlap_save.h:49,
 * lib/overlap_save_impl.cc:41-81.  Type-agnostic byte copies on the device. */
typedef struct fdc_overlap_save fdc_overlap_save;
int fdc_overlap_save_create(int device_id, int itemsize, int outputlen, int overlaplen, fdc_overlap_save **out);
int fdc_overlap_save_work(fdc_overlap_save *b, const void *in, int nitems, void *out);
void fdc_overlap_save_destroy(fdc_overlap_save *b);

/* gr::FDC::vector_cut_vxx::make(itemsize, veclen, offset, blocklen) — include/FDC/vector_cut_vxx.h:49,
 * lib/vector_cut_vxx_impl.cc:41-72. */
typedef struct fdc_vector_cut fdc_vector_cut;
int fdc_vector_cut_create(int device_id, int itemsize, int veclen, int offset, int blocklen, fdc_vector_cut **out);
int fdc_vector_cut_work(fdc_vector_cut *b, const void *in, int nitems, void *out);
void fdc_vector_cut_destroy(fdc_vector_cut *b);

/* gr::FDC::phase_shifting_windowing_vcc::make(blocklen, numphasestates, shifts, passbw, stopbw, windowtype)
 * — include/FDC/phase_shifting_windowing_vcc.h:49, lib/phase_shifting_windowing_vcc_impl.cc:41-86.
 * create fails with FDC_ERR_INVALID_ARGUMENT on the ctor's predicates (:46-53). */
typedef struct fdc_phase_window fdc_phase_window;
int fdc_phase_window_create(int device_id, int blocklen, int numphasestates, int shifts, float passbw,
                            float stopbw, int windowtype, fdc_phase_window **out);
int fdc_phase_window_work(fdc_phase_window *b, const void *in, int nitems, void *out);
void fdc_phase_window_destroy(fdc_phase_window *b);

/* Window table generator used by the faces above (lib/windows.h:41-78 cr_win): w receives
 * [numphasestates][blocklen] complex float32.  Host-side, no device needed. */
int fdc_window_table(int windowtype, int blocklen, float passbw, float stopbw, int numphasestates,
                     int step, int normalize, float *w);

/* Stand-alone batched FFT with the semantics of gr-fft fft_vcc(n, forward, rectangular, shift, *)
 * (python/FrequencyDomainChannelizer.py:206,228) on host buffers: nitems transforms of length n. */
int fdc_fft_vcc(int device_id, int n, int forward, int shift, const void *in, int nitems, void *out);

/* ---------------------------------------------------------------------------------------------
 * Waterfall rows: the data path of FDC.WaterfallMsgTagging (python/WaterfallMsgTagging.py), the sink the reference's example
 * flowgraph ends in (examples/FDC_example.grc: complex_to_mag_squared(blocklen) -> WaterfallMsgTagging).  Per block the N-bin power
 * vector becomes 1024 pixels (:251-254: the mean of N/1024 consecutive bins for N >= 1024, each bin repeated 1024/N times below),
 * blockdecimation consecutive rows are averaged, aligned to the first block of the stream, the unfinished group carried to the next
 * call (:153-164 pxupdate, puffer_blocks), and every pixel gets a colour index = numpy.digitize(x, edges, right=False) against 1023
 * edges linspace(minvaldb, maxvaldb, 1023), 10**(edge/10) when loginput = 0 (:261-262, :284-287), compared in FP64, and optionally
 * the RGB888 colour of one of four schemes (:276-312).  The Qt widget and the PDU rectangles are not here (host code, the Python
 * WaterfallImage draws them).  Row values are deterministic: the same input gives the same bytes, however the calls split it.
 *   rows   NULL or cap_rows x 1024 float32: mean power per pixel of every row finished in the call
 *   index  NULL or cap_rows x 1024 uint16: colour index 0 .. 1023
 *   rgb    NULL or cap_rows x 1024 x 3 bytes
 *   nrows  receives the number of rows finished; more than cap_rows is FDC_ERR_INVALID_ARGUMENT before anything is consumed.
 * Row r covers blocks [r D, (r + 1) D) of the handle's stream (D = blockdecimation); fdc_waterfall_reset starts a new stream
 * (fdc_pipeline_reset does NOT reset a waterfall used with the pipeline: call both).
 * ---------------------------------------------------------------------------------------------- */
typedef struct fdc_waterfall fdc_waterfall;
typedef struct {
    int32_t blocklen;         /* N: a multiple of 1024 or a divisor of 1024 (the reference's reshape fails elsewhere) */
    int32_t blockdecimation;  /* D; <= 0 is 1 (:37) */
    int32_t loginput;         /* != 0: the input is already in dB, the edges are linspace itself */
    double minvaldb, maxvaldb;  /* the reference's levels are Python floats: the edges are made from these doubles */
    int32_t colorscheme;      /* 0 black-blue-cyan-white, 1 black-rainbow, 2 black-red-yellow, 3 black-white; others are 0 (:306) */
} fdc_waterfall_cfg;
/* Host only: the configuration create would use (D <= 0 -> 1) or FDC_ERR_INVALID_ARGUMENT. */
int fdc_waterfall_check(const fdc_waterfall_cfg *cfg, fdc_waterfall_cfg *normalized);
/* max_items: the most blocks one fdc_pipeline_work_waterfall call carries, and the blocks per internal pass of fdc_waterfall_work */
int fdc_waterfall_create(int device_id, const fdc_waterfall_cfg *cfg, int32_t max_items, fdc_waterfall **out);
void fdc_waterfall_destroy(fdc_waterfall *w);
void fdc_waterfall_reset(fdc_waterfall *w);                                   /* carried rows and row counter <- 0 */
int fdc_waterfall_set_levels(fdc_waterfall *w, double minvaldb, double maxvaldb);   /* set_minvaldb / set_maxvaldb (:264-270) */
int fdc_waterfall_set_colorscheme(fdc_waterfall *w, int32_t scheme);            /* set_colorscheme (:272-274) */
int64_t fdc_waterfall_rows_done(const fdc_waterfall *w);                      /* rows finished since create / reset */
/* Host only: the 1024 x 3 colour table and the frame colour of a scheme (cr_colorscheme, numpy.linspace(..., dtype = uint8) truncation) */
int fdc_waterfall_color_table(int32_t scheme, uint8_t *rgb, uint8_t *frame);
/* Host only: the 1023 FP64 edges the colour index is counted against */
int fdc_waterfall_edges(int32_t loginput, double minvaldb, double maxvaldb, double *edges);
/* The reference block: nitems float32 power vectors of blocklen (host buffers, as fdc_pipeline_work) */
int fdc_waterfall_work(fdc_waterfall *w, const float *power, int nitems, float *rows, uint16_t *index, uint8_t *rgb, int cap_rows,
                       int32_t *nrows);
/* The hier block with the waterfall on its spectrum: the channels of fdc_pipeline_work and the rows of this call as above (no spectrum to the host,
 * no keep_spectrum needed).  Needs the same device and blocklen, nblocks <= the waterfall's max_items.  Routes:
 *  - path 5 (N = 4096 in one launch) stays path 5: its kernel sums the rows' pixels from the spectrum in LDS, and the channel outputs are
 *    bit-identical to fdc_pipeline_work's;
 *  - every other plan runs the spectrum path, as a call that asks for the spectrum does (the channel outputs are those of fdc_pipeline_work
 *    with a debug spectrum, equal to fdc_pipeline_work's to rounding): the rows are summed from the spectrum's 16-bin group powers (N a multiple
 *    of 16384) or from its bins.
 * fdc_pipeline_describe names the route of the last such call. */
int fdc_pipeline_work_waterfall(fdc_pipeline *p, fdc_waterfall *w, const void *in, int nblocks, void *const *outs, float *rows,
                                uint16_t *index, uint8_t *rgb, int cap_rows, int32_t *nrows);

#ifdef __cplusplus
}
#endif
#endif /* FDC_AMD_H */
