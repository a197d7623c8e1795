// Internal launcher interface between the host side of the library (the C-ABI entries, fdc_plan.hip, fdc_enqueue.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fdc {

constexpr int kThreads = 256;        // 4 wave64 per workgroup
constexpr int kMaxLdsFft = 8192;     // longest transform one workgroup does in LDS

// Per-channel record in device memory.
struct ChanDev {
    int32_t f;          // first bin in the shifted spectrum
    int32_t l;          // slice / IFFT length
    int32_t lout;       // l - l/R
    int32_t shift;      // ((f mod R)+R) mod R   (lib/phase_shifting_windowing_vcc_impl.cc:58)
    int64_t out_off;    // sum of lout over preceding channels (samples per block)
    int32_t win_off;    // offset of this channel's [R][l] table in the window pool (complex elements)
    int32_t pad;
};

// Sinks (PowerActivationChannel / activity_detection_channelizer_vcm): power cells and extraction tasks.
struct PowerCell { int32_t start, len; float scale; int32_t pad; };
struct ExtractTask {
    int32_t slot;       // spectrum block slot (0 = history block of the previous call, 1.. = blocks of this call)
    int32_t start;      // first bin of the slice
    int32_t win_off;    // offset of the (phase-resolved) window in the pool, complex elements
    int32_t pad;
    int64_t out_off;    // where the w - skip output samples go, complex elements
};

// Geometry of an LDS "column" FFT tile: TC independent transforms of length L, element (i, t) at i*ld + t.
struct TileGeom {
    int L, log2L, TC, log2TC, ld, NB;   // NB: 4096-point units per tile (2 only for L = 8192)
    size_t lds_bytes() const { return (size_t)L * ld * sizeof(float2); }
};
TileGeom tile_geom(int L);

// Two-pass split N = N1*N2 used above kMaxLdsFft.
struct BigGeom { int N, N1, N2; TileGeom a /* length N2 */, b /* length N1 */; };
BigGeom big_geom(int N);

hipError_t init_kernels();   // raises the dynamic-LDS limits once per process

// Forward/inverse batched FFT of `nitems` transforms of length N (any power of two >= 2).
//   in : item m starts at in + m*in_stride (complex elements); element n is read at (n + in_rot) mod N
//   out: item m at out + m*N; result bin k is stored at (k + out_rot) mod N, multiplied by scale
//   tw : exp(-2 pi i k / ntab), k in [0, ntab), ntab >= N, ntab % N == 0
//   tmp: nitems*N complex scratch (two-pass sizes only)
hipError_t launch_fft(const float2 *in, size_t in_stride, float2 *out, float2 *tmp, int N, int nitems,
                      bool inverse, int in_rot, int out_rot, float scale, const float2 *tw, int ntab,
                      hipStream_t s, hipEvent_t *ev /* null or 3 events: start, after pass A, end */,
                      const float2 *twf = nullptr /* two-pass sizes: [k2][n1] = exp(-2 pi i n1*k2/N), N entries, optional */,
                      bool generic_only = false /* no size-specific register kernels (FDC_FORCE_GENERIC handles) */,
                      unsigned long long keep4096 = ~0ull /* N = 4096: 64-bin groups of the output that are wanted (others may stay unwritten) */);

// Fused slice + phase + window + ifftshift + IFFT(l) + overlap discard + *l for one group of channels of
// equal l (<= kMaxLdsFft).  spec holds nb_chunk spectra; block m of the chunk is block mbase+m of the call.
hipError_t launch_channels(const float2 *spec, float2 *out, const ChanDev *chans, const int32_t *group,
                           int ngroup, int l, int N, int R, int nb_chunk, int mbase, int nb_call,
                           int64_t first_block, const float2 *wins, const float2 *tw, int ntab, hipStream_t s);

// ---- fast path (fdc_fast256.hip): N = 65536 forward transform, l = 256 channels ------------------------
//   tw256: exp(-2 pi i j/256), j in [0,256);  twf: [k2][n1] = exp(-2 pi i n1*k2/65536)
hipError_t init_fast_kernels();
hipError_t launch_fft65536(const float2 *in, size_t in_stride, float2 *out, float2 *tmp, int nitems, int out_rot,
                           float scale, const float2 *tw256, const float2 *twf, hipStream_t s, hipEvent_t *ev);
// needs an even discard length 256/R; aligned = all f even; out_aligned = all out_off and lout even
hipError_t launch_channels256(const float2 *spec, float2 *out, const ChanDev *chans, const int32_t *group,
                              int ngroup, bool aligned, bool out_aligned, int N, int R, int nb_chunk, int mbase,
                              int nb_call, int64_t first_block, const float2 *wins, const float2 *tw256,
                              hipStream_t s);

// the same for l = 512 and l = 1024 (fdc_chanwide.hip: 32 points per lane, DFT-32 layers); needs an even discard length l/R
hipError_t init_wide_kernels();
hipError_t launch_channels_wide(const float2 *spec, float2 *out, const ChanDev *chans, const int32_t *group, int ngroup, int l,
                                int N, int R, int nb_chunk, int mbase, int nb_call, int64_t first_block, const float2 *wins,
                                const float2 *tw, int ntab, hipStream_t s);

// 4096-point transforms in registers (fdc_chanwide.hip), same meaning of the arguments as launch_fft
hipError_t launch_fft4096(const float2 *in, size_t in_stride, float2 *out, int nitems, bool inverse, int in_rot, int out_rot,
                          float scale, const float2 *tw, int ntab, hipStream_t s,
                          unsigned long long keep = ~0ull /* 64-bin groups of the output some reader wants */);

// N = 4096 in one launch (fdc_fused4096.hip): forward transform + every channel's slice / window / inverse transform, the spectrum stays in LDS.
// A 512-thread workgroup takes a pair of blocks.  The schedule is the host's (fdc_plan.hip plan_fused4096): rows[8 waves][8 slots], four bits per
// wave in wcls (0 = no rows, 1 = l = 256 slots 0..3, 2 = l = 256 slots 0..7, 3 = l = 512 slots 0..3, 4 = l = 1024 slots 0..1, 5 / 6 / 7 / 8 = l = 128 / 64 / 32 / 16
// slots 0..7); valid = 0: no row,
// 1 + k: a row of the pair's block k; xch = the row's exchange area in the two tiles (points), rows disjoint, all inside 2 fused4096_tile_points().
// Unused slots: everything 0 except lout.
struct F4Row { int32_t f, win_off, shift, xch, lout, valid; long long out_off; };
hipError_t init_fused4096_kernels();
int fused4096_tile_points();
// One launch over a launch group.  Which form of the kernel it takes (fdc_fused4096.hip, for_f4_forms) follows from the formats, wf, fine_rows, teams and
// wcls; hipErrorInvalidValue where there is none: an unknown format, wf together with integer samples or fine tuning, teams other than 1 or 2
struct FineChan;
struct F4Launch {
    const void *in;              // first sample of the launch group's first block; item m at in + m * in_stride samples
    int ifmt; float iscale;      // kIqFloat (fdc_iq.hpp): in holds float2; kIqSc16 / kIqSc8: integer samples, widened times iscale in the kernel's loads
    size_t in_stride;
    void *out;                   // float2, or with ofmt = kIqSc16 / kIqSc8 the same sample offsets in narrow elements, narrowed times oscale in the stores (oq_bits)
    int ofmt; float oscale;
    int nb_chunk, R, mbase, nb_call;   // blocks of this launch, overlap, index of its first block in the call, blocks of the call
    int64_t first_block;         // the stream's index of the call's block 0
    const float2 *tw; int ntab;  // exp(-2 pi i k / ntab), ntab a multiple of 4096
    const float2 *wins;
    const F4Row *rows; unsigned wcls; int teams;   // the schedule; teams = blocks per workgroup: 1 (rows[4][8], no wide rows) or 2 (rows[8][8])
    float *wf;                   // null, or nb_chunk x 1024 waterfall row sums (fdc_waterfall.hip): the ROWS form
    const FineChan *fine_rows;   // null, or fine tuning in the stores (fdc_fine.hpp): [8 waves][8 slots] the increment and step-table start of each schedule
    const float2 *fine_step;     //   row's channel, and the step table: the FINE forms
    hipStream_t s;
};
hipError_t launch_fused4096(const F4Launch &a);

// uniform plan (all channels l = 256, f = 256*slot, N = 256*N1): stage 1 + stage 2, no spectrum in memory.
//   twq[n1][q] = W_N^(16*n1*q), cbt[n1][b] = (-1)^n1 W_N^(n1*b)  (16 entries per n1 each), shn[k2] = shape[k2]/N;
//   slot_off[c] = per-block sample offset of the channel sitting in slot c, or -1;  g: nb_chunk*lout*N1 scratch
// one entry per channel: where the caller's (pinned, device-mapped) buffer of that channel is
struct ScatterEnt { float2 *dst; long long out_off; int lout; int pad; };
// dst[c][row0*lout_c + i] = src[nb*out_off_c + i], i < nb*lout_c: the [channel][nb*lout] result of one sub-batch is
// stored straight into the caller's per-channel host buffers (PCIe writes, 512 B per wave)
hipError_t launch_scatter_out(const float2 *src, const ScatterEnt *tab, int nchan, int nb, long long row0, hipStream_t s);
// the same with integer output (ofmt: kIqSc16 / kIqSc8; dst holds narrow samples): src_fmt kIqFloat = src is float2, narrowed times scale on the way
// (oq_bits); src_fmt = ofmt = src holds the narrow samples already (a copy)
hipError_t launch_scatter_oq(int src_fmt, const void *src, int ofmt, float scale, const ScatterEnt *tab, int nchan, int nb, long long row0, hipStream_t s);

hipError_t launch_poly_stage1(const float2 *in, size_t in_stride, float2 *g, int N1, int R, int nb_chunk,
                              const float2 *tw256, const float2 *twq, const float2 *cbt, const float *shn,
                              int ncu /* compute units of the device */, hipStream_t s);
hipError_t launch_poly_stage2(const float2 *g, float2 *out, int N1 /* 256 or 1024 slots */, int R, int nb_chunk, int mbase,
                              int nb_call, const float2 *tw256, const float2 *tw1024 /* N1 = 1024 only */,
                              const long long *slot_off, unsigned out_bytes /* whole d_out, < 4 GiB */,
                              int ncu, hipStream_t s);

// stage 2 for any other slot count N1 = N/256 in [16, 4096] (generic LDS core, fdc_kernels.hip)
hipError_t launch_poly_stage2_generic(const float2 *g, float2 *out, int N1, int R, int nb_chunk, int mbase, int nb_call,
                                      const long long *slot_off, const float2 *tw, int ntab, hipStream_t s,
                                      int L = 256 /* channel width; other than 256: G in rows of N1 columns (launch_poly_stage1_generic) */);
// uniform plans of any power-of-two width L on the L-bin grid: stage 1 on the generic LDS core; g: nb_chunk * (L - L/R) * N/L points,
// shn[k2] = shape[k2] / N (L entries), tw = exp(-2 pi i k / ntab) with ntab = N
// t2[k2][t] = W_N^(t k2), t < poly_stage1_generic_tile_columns(N, L): the tile-local factor of the inter-pass twiddle
hipError_t launch_poly_stage1_generic(const float2 *in, size_t in_stride, float2 *g, int N, int L, int R, int nb_chunk, const float *shn,
                                      const float2 *tw, int ntab, const float2 *t2, hipStream_t s);
int poly_stage1_generic_tile_columns(int N, int L);

// ---- uniform plans, N = 16384 / 32768 / 65536, R = 2 or 4: the whole path in one kernel, one block per CU, G kept in registers
// (fdc_block256.hip, fdc_block512.hip, fdc_block1024.hip, fdc_blocknarrow.hip; their shared core: fdc_blockcommon.hpp).
// One launch of a bank's block kernel over a launch group: what every launcher below takes.
struct BlockLaunch {
    // the samples: complex float (kIqFloat, fdc_iq.hpp), or for L = 256 complex integers (kIqSc16 / kIqSc8) that the kernel widens times iscale in its loads
    // and narrows times oscale in its stores (out_bytes: the narrow extent; streamed stores only, hints bit 0).  The other widths take float only
    const void *in;              // first sample of the launch group's first block
    int ifmt; float iscale;
    size_t in_stride;            // samples from one block to the next
    void *out;
    int ofmt; float oscale;
    int nb_chunk, mbase, nb_call;   // blocks of this launch, index of its first block in the call, blocks of the call
    const long long *slot_off;   // [N / L]: where each channel slot's samples go (negative: unused)
    unsigned out_bytes;          // whole output, < 4 GiB
    int ncu;                     // compute units of the device (grid size)
    int hints;                   // 1 = nt output stores, 2 = nt input loads
    hipStream_t s;
    hipEvent_t ev_start, ev_stop;   // timing: stamped by the dispatch itself (may be null)
    int N, R;                    // block length; overlap 2 or 4
    float2 *scratch;             // R = 4: ncu x 32768 points
    int L, r;                    // channel width; common offset f mod L of the bank's channels (the tables hold it)
    long long first_block;       // global index of block 0 of this launch (window phase of odd r, L = 256)
    const float2 *cbt;           // L >= 256: [n1][L / 16] (-1)^n1 W_N^(n1 (b + r + 256 i)); narrow: [V][16] W_N^(S V (b + r))
    const float *shn;            // [L] shape / N (L >= 256)
    const float2 *tw256, *twq;   // W_256^k; [n1][16] W_N^(16 n1 q) (L >= 256)
    const float2 *twl;           // L = 512: W_512^k, k < 256; L = 1024: W_1024^k, k < 1024
    const float2 *tab;           // L = 128 / 64: the table image of poly_block_narrow_tables()

    const float2 *fin() const { return static_cast<const float2 *>(in); }   // float samples, as the kernels without integer forms take them
    float2 *fout() const { return static_cast<float2 *>(out); }
    bool half() const { return r == L / 2; }                 // the bank half a channel off the grid: the on-grid kernels with their tables moved
    int grid(int per_cu = 1) const                           // one 512-thread workgroup per CU (or per_cu), never more than there are blocks
    {
        const int g = (ncu > 0 ? ncu : 256) * per_cu;
        return g > nb_chunk ? nb_chunk : g;
    }
};

// L = 256 (fdc_block256.hip): any offset r; cbt must hold (-1)^n1 W_N^(n1 (b + r)).  Which form of the kernel a launch takes: for_blk256_forms there;
// hipErrorInvalidValue where there is none
hipError_t init_block_kernels();
hipError_t launch_poly_block(const BlockLaunch &b);
bool poly_block_supports(int N);

// L = 512 on the 512-bin grid or half a channel off it (fdc_block512.hip): the two parities of a column's 512 rows run the 256-point machinery side by
// side in the lanes of a quad.
//   twl[k] = W_512^k (k < 256); twq[n1][q] = W_N^(16 n1 q) (N/512 x 16); cbt[n1][b + 16 h] = (-1)^n1 W_N^(n1 (b + 256 h)) (N/512 x 32);
//   shn[k2] = shape[k2] / N (512); half: shn and cbt with their halves swapped, W_N^(256 n1) in cbt
hipError_t init_block512_kernels();
hipError_t launch_poly_block512(const BlockLaunch &b);
bool poly_block512_supports(int N, int R);

// L = 1024 on the 1024-bin grid or half a channel off it (fdc_block1024.hip): the four phases of a column's 1024 rows run the 256-point machinery side
// by side in the lanes of a quad.  scratch (R = 4): ncu x 16384 points.
//   twl[k] = W_1024^k (k < 1024); twq[n1][q] = W_N^(16 n1 q) (N/1024 x 16); cbt[n1][b + 16 i] = (-1)^n1 W_N^(n1 (b + 256 i)) (N/1024 x 64);
//   shn[k2] = shape[k2] / N (1024); half: the quarters of shn and cbt moved by two, W_N^(512 n1) in cbt
hipError_t init_block1024_kernels();
hipError_t launch_poly_block1024(const BlockLaunch &b);
bool poly_block1024_supports(int N, int R);

// narrow channels, L = 128 or 64, r = 0, L/4, L/2, 3L/4 (fdc_blocknarrow.hip): S = 256/L adjacent columns interleaved into one 256-point virtual column,
// separated and re-joined in registers.  scratch (R = 4): ncu x 16384 points.
//   tab = the table image of poly_block_narrow_tables() (shn[k2] = shape[k2] / N, L values); cbt[V][b] = W_N^(S V b) (N/256 x 16); slot_off[N / L]
bool poly_block_narrow_supports(int N, int L, int R);
hipError_t init_block_narrow_kernels();
int poly_block_narrow_table_points(int L, int N);
void poly_block_narrow_tables(int L, int N, const float *shn, float2 *img, bool half = false /* the bank at f = l slot + l/2; cbt then W_N^(S V (b + l/2)) */,
                              int r = 0 /* l/4 or 3l/4 (not with half): the bank at f = l slot + r; cbt then W_N^(S V (b + r)) */);
hipError_t launch_poly_block_narrow(const BlockLaunch &b);

// forward transform of N-sample blocks (N = 16384 / 32768 / 65536) with the block kernel (both halves of k2 in one launch): shifted, 1/N-scaled spectrum
hipError_t launch_block_fft(int N, const float2 *in, size_t in_stride, float2 *out, int nitems, const float2 *tw256,
                            const float2 *twq, const float2 *cbt0 /* r = 0 */, const float *shn1 /* 256 x 1/N */,
                            const long long *slot_off /* [N / 256]: 256 c */, float2 *scratch /* ncu x 32768 points */,
                            int ncu, int hints, hipStream_t s,
                            hipEvent_t *ev /* null or 3: start, end, end */,
                            const unsigned *keep = nullptr /* [N / 8192][4] words: 64-bin stores some channel reads (fdc_plan.hip), or all */,
                            float *gpow = nullptr /* nitems x N / 16 floats: the power of every 16-bin group of the spectrum, summed in the epilogue */);
// the sinks' power cells from those group sums + the bins of the groups a cell cuts; the group sums of a spectrum in memory (launch groups the block kernel did not transform)
hipError_t launch_cell_power_groups(const float2 *spec, const float *gpow, int N, const PowerCell *cells, int ncells, int nblocks, float *out, hipStream_t s);
hipError_t launch_group_power(const float2 *spec, int N, int nblocks, float *gpow, hipStream_t s);

// real samples -> complex samples with zero imaginary part (the real-input front end)
hipError_t launch_real_to_complex(const float *in, float2 *out, size_t n, hipStream_t s);
// complex integer samples (fmt: kIqSc16 / kIqSc8, fdc_iq.hpp) -> complex float, (I * scale, Q * scale)
hipError_t launch_iq_to_complex(int fmt, float scale, const void *in, float2 *out, size_t n, hipStream_t s);

// The passes behind a plan's kernels (fdc_postpass.hip), over the channel-major float results of a launch group; which of them a call runs, and in
// which order: fdc_enqueue.hip, PostPass
// complex float -> complex integer samples (fmt: kIqSc16 / kIqSc8), each component saturate(round_half_even(x * scale)) (fdc_iq.hpp oq_bits)
hipError_t launch_complex_to_iq(int fmt, float scale, const float2 *in, void *out, size_t n, hipStream_t s);

// Fine tuning (fdc_fine.hpp): blocks [mbase, mbase + nb_chunk) of a call's channel-major float outputs turned in place, channel c by
// exp(-2 pi i frac(fine[c].inc t / 2^64)) at its stream sample t = (first_block + m) lout_c + j; step: the channels' step factors at fine[c].step_off
// levels (fine tuning AND channel levels on): the pass also reduces the turned samples it holds and stores their levels as launch_chan_levels would
hipError_t launch_fine_rotate(float2 *out, const ChanDev *chans, const FineChan *fine, const float2 *step, int nchan, int nb_chunk, int mbase, int nb_call,
                              int64_t first_block, hipStream_t s, float2 *levels = nullptr, const float *gain = nullptr);

// Channel levels (fdc_pipeline_set_levels): blocks [mbase, mbase + nb_chunk) of a call's channel-major float outputs read once; levels[(mbase + m) * nchan + c] =
// (sum of re^2 + im^2, max of |re| and |im|) over the lout_c samples of block m of channel c.  One summation order per lout (fdc_postpass.hip)
hipError_t launch_chan_levels(const float2 *out, const ChanDev *chans, float2 *levels, int nchan, int nb_chunk, int mbase, int nb_call, hipStream_t s);

// Channel gains (fdc_pipeline_set_gains) where no rotation pass runs: blocks [mbase, mbase + nb_chunk) of a call's channel-major float results times
// gain[c], every component rounded once.  fmt 0: in place; kIqSc16 / kIqSc8: `out` is read only and oq_narrow(product, scale) goes to the same sample
// offset of the narrow output `nar`.  levels (null: none): the gained samples' levels as launch_chan_levels would sum them, in the same pass
hipError_t launch_chan_gain(float2 *out, const ChanDev *chans, const float *gain, float2 *levels, int fmt, float scale, void *nar, int nchan, int nb_chunk,
                            int mbase, int nb_call, hipStream_t s);

// Channel lag-1 correlation (fdc_pipeline_set_lag1): blocks [mbase, mbase + nb_chunk) of a call's channel-major float results read once;
// lag1[(mbase + m) * nchan + c] = sum over j >= 1 of y[j] conj(y[j - 1]) over the lout_c samples of block m of channel c.  One summation order per lout
// (fdc_postpass.hip).  gain (null: none): the samples times gain[c] first, where the gain pass in front has left the float results as they were cut
hipError_t launch_chan_lag1(const float2 *out, const ChanDev *chans, const float *gain, float2 *lag1, int nchan, int nb_chunk, int mbase, int nb_call,
                            hipStream_t s);

// Channel demodulation (fdc_pipeline_set_demod): the whole call's channel-major float results `in` (nb_call blocks) read once, one real float32 per
// sample to the same element offset of `out`.  mode: kDemodFm / kDemodMag = FDC_DEMOD_FM / FDC_DEMOD_MAG.  FM: carry_in[c] is the sample in front of
// channel c's first (null: none, the stream starts anew) and carry_out[c] receives its last; two different buffers of nchan float2.  MAG uses neither.
// sum_lout: the plan's output samples per block (sizes the grid)
enum { kDemodFm = 1, kDemodMag = 2 };
hipError_t launch_chan_demod(int mode, float gain, const float2 *in, float *out, const ChanDev *chans, const float2 *carry_in, float2 *carry_out, int nchan,
                             int nb_call, long long sum_lout, hipStream_t s);

// Channel audio (fdc_pipeline_set_audio): the decimating FIR over the whole call's demodulated samples `in` (launch_chan_demod's out), a[n] = sum over
// k ascending of taps[k] d[n decim - k] from +0, every product and sum rounded on its own.  format: kAudioF32 / kAudioS16 = FDC_AUDIO_F32 / _S16 (S16:
// oq_round(a, scale)).  out: row 0 of the call's block-major matrix [nb_call][row] of float / int16; channel c owns the lout_c / decim columns from
// aoff[c] on.  hist_in ([nchan][ntaps - 1] float; null: zeros) stands in front of every channel's first sample, hist_out (another buffer; null only
// where ntaps = 1) receives the last ntaps - 1 values of (what stood in front, the call's samples).  decim divides every lout_c
// gate (null: none): row 0 of the call's squelch mask ([nb_call][nchan] bytes, launch_chan_squelch): the gated forms, which store zero bits for the
// outputs of a closed (block, channel), skip the work of closed tiles and leave the history what the ungated pass leaves
enum { kAudioF32 = 0, kAudioS16 = 1 };
hipError_t launch_chan_audio(int format, int decim, int ntaps, float scale, const float *taps, const long long *aoff, long long row, const float *in,
                             void *out, const ChanDev *chans, const float *hist_in, float *hist_out, int nchan, int nb_call, long long sum_lout,
                             hipStream_t s, const unsigned char *gate = nullptr, const unsigned *pack_off = nullptr);
// pack_off (null: none; it needs gate): row 0 of the call's offsets ([nb_call][nchan] words, launch_audio_pack_offsets over the same mask): the packed
// forms, which store the outputs of an open (block, channel) at out[pack_off[block][channel] + i] and those of a closed one nowhere; out is then element
// 0 of the packed buffer, and exactly the elements the offsets count are written

// Audio resampler (fdc_pipeline_set_audio_resampler): the polyphase FIR with interpolation `up` and decimation `down` over the same samples, a[n] = sum
// over k = 0 .. kp - 1 of h[k up + (n down mod up)] d[(n down div up) - k] with n and the sample index counted from the stream's block 0 (the call
// starts at block first_block), in launch_chan_audio's arithmetic.  taps_pm: the taps phase-major, [up][kp] (taps_pm[ph kp + k] = h[k up + ph], +0
// behind the last).  out: row 0 of the call's block-major matrix [nb_call][row]; channel c owns the ceil(lout_c up / down) columns from aoff[c] on, a
// cell holds the outputs whose newest sample lies in its block, and one zero behind them where it owns a column less.  The histories are [nchan][kp - 1]
// float, as launch_chan_audio's; gate likewise (the gated forms).  Every element of the matrix is written, and nothing else
hipError_t launch_chan_resample(int format, int up, int down, int kp, float scale, const float *taps_pm, const long long *aoff, long long row,
                                const float *in, void *out, const ChanDev *chans, const float *hist_in, float *hist_out, int nchan, int nb_call,
                                long long sum_lout, long long first_block, hipStream_t s, const unsigned char *gate = nullptr);

// Packed audio (fdc_pipeline_set_audio_packing): the offsets of the call's cells in the packed buffer.  mask: row 0 of the call's mask ([nb_call][nchan]
// bytes); off ([nb_call][nchan] words) receives *base_in (null: 0) + the audio samples (lout_c / decim each) of all open cells in front of (block,
// channel), block-major; total (one word, which may be base_in's) receives *base_in + those of all open cells.  Three launches on s
hipError_t launch_audio_pack_offsets(const unsigned char *mask, const ChanDev *chans, int decim, const long long *base_in, unsigned *off, long long *total,
                                     int nchan, int nb_call, hipStream_t s);

// Channel squelch (fdc_pipeline_set_squelch): the decision over the call's rows of the levels ([nb_call][nchan] (power, peak), launch_chan_levels and
// its kin), one byte per (block, channel) to mask ([nb_call][nchan]): open at a block whose power reaches g2 thr_open[c], held while it reaches
// g2 thr_close[c], closed after hang + 1 consecutive blocks below (g2 = gain[c]^2 rounded once; gain null: 1).  state_in ([nchan][2] int: open, h;
// null: all closed) stands in front of the call, state_out (another buffer) receives the state behind its last block.  hang 0 .. 65535
hipError_t launch_chan_squelch(const float2 *levels, const float *gain, const float *thr_open, const float *thr_close, int hang, const int *state_in,
                               int *state_out, unsigned char *mask, int nchan, int nb_call, hipStream_t s);

// Channel tones (fdc_pipeline_set_tones; fdc_tones.hip): the tone bank over the whole call's demodulated samples `in` (launch_chan_demod's out).  inc:
// [nchan][ntones] phase increments per group of `group` samples (which divides every lout_c); tab: tone_table's kToneTable pairs on the device.  The
// call is blocks [first_block, first_block + nb_call) of the stream, `fill` blocks (0 .. frame_blocks - 1) of which stand in the open frame in front of
// it with their accumulators in carry_in ([nchan][ntones] float2; null: zeros; read only where fill > 0).  frames receives the (fill + nb_call) div
// frame_blocks rows the call completes, [frame][nchan][ntones] float2 (null where it completes none), carry_out (another buffer) all nchan * ntones
// accumulators of the frame left open, zeros where none is.  tests/tones_model.py is the arithmetic
constexpr int kToneTable = 1024;
void tone_table(float2 *dst);       // host: (cos, sin)(2 pi k / kToneTable), designed in double, rounded once, the axis entries exact
hipError_t launch_chan_tones(const float *in, const ChanDev *chans, const unsigned *inc, const float2 *tab, const float2 *carry_in, float2 *carry_out,
                             float2 *frames, int nchan, int ntones, int group, int frame_blocks, int fill, long long first_block, int nb_call, hipStream_t s);

// Tone squelch (fdc_pipeline_set_tone_squelch; fdc_tonesquelch.hip): the decision over the (fill + nb_call) div frame_blocks frame rows the call's tones
// pass completed (`frames`, launch_chan_tones' own; null where it completed none), one byte per (frame, channel) to dec ([frame][nchan]); then, unless
// mask is null, the call's carrier mask ([nb_call][nchan], launch_chan_squelch's) ANDed in place with the decision in force at each block: state_in's
// open for the blocks of the frame that was open in front of the call, dec of the frame before otherwise.  tone: [nchan], -1 = the channel is not
// tone-gated; thr_open / thr_close / ratio: [nchan].  state_in ([nchan][2] int: open, h; null: all closed), state_out (another buffer) as the squelch's,
// h counting frames.  tests/tone_squelch_model.py is the rule
hipError_t launch_tone_squelch(const float2 *frames, const int *tone, const float *thr_open, const float *thr_close, const float *ratio, int guard, int hang,
                               const int *state_in, int *state_out, unsigned char *dec, unsigned char *mask, int nchan, int ntones, int frame_blocks,
                               int fill, int nb_call, hipStream_t s);

hipError_t launch_scale(const float2 *in, float2 *out, size_t n, float k, hipStream_t s);

// sinks
hipError_t launch_cell_power(const float2 *spec, int N, const PowerCell *cells, int ncells, int nblocks, float *out,
                             hipStream_t s);
// one width class above 4096 points (two passes through `tmp`, ntasks * w points; slice * window read by pass A, kept samples
// written to their places by pass B)
hipError_t launch_extract_wide(const float2 *spec, int N, const ExtractTask *tasks, int ntasks, int w, int skip, const float2 *wins,
                               float2 *tmp, float2 *out, const float2 *tw, int ntab, hipStream_t s, float scale = 1.0f);
// the channels of one width above 4096 bins of a pipeline as such tasks: task m * ngroup + gi = channel group[gi] in block m of the launch group
hipError_t launch_wide_tasks(ExtractTask *tasks, const ChanDev *chans, const int32_t *group, int ngroup, int R, int nb_chunk, int mbase, int nb_call,
                             int64_t first_block, hipStream_t s);
// several width classes (w <= 4096 each) in one launch: class k = tasks [first[k], first[k] + cnt[k]) of width w[k]
constexpr int kMaxExtractClasses = 12;
struct ExtractClass { int32_t tile0, task0, ntasks, log2w, log2TC, ld, skip, pad; };
struct ExtractClasses { ExtractClass c[kMaxExtractClasses]; int32_t n; };
hipError_t launch_extract_multi(const float2 *spec, int N, const ExtractTask *tasks, const int *w, const size_t *first, const size_t *cnt,
                                int nclass, int R, const float2 *wins, float2 *out, const float2 *tw, int ntab, hipStream_t s);
hipError_t launch_extract(const float2 *spec, int N, const ExtractTask *tasks, int ntasks, int w, int skip,
                          const float2 *wins, float2 *out, const float2 *tw, int ntab, hipStream_t s);

// width 256 on the register kernel of the l = 256 channels (fdc_fast256.hip); tw256: exp(-2 pi i j/256)
hipError_t launch_extract256(const float2 *spec, int N, const ExtractTask *tasks, int ntasks, int skip, const float2 *wins, float2 *out,
                             const float2 *tw256, hipStream_t s);
// ... with the emitted runs narrowed in its own stores (fdc_sinks_set_payload_format, fmt = kIqSc16 / kIqSc8): a task whose out_off lies below used_a
// lands in nout (samples of the format, same sample offset), every other one in out as complex float
hipError_t launch_extract256_narrow(int fmt, float scale, const float2 *spec, int N, const ExtractTask *tasks, int ntasks, int skip, const float2 *wins,
                                    float2 *out, void *nout, long long used_a, const float2 *tw256, hipStream_t s);

// single-block faces
hipError_t launch_overlap_save(const unsigned char *ring, unsigned char *out, size_t in_item_bytes,
                               size_t out_item_bytes, int nitems, hipStream_t s);
hipError_t launch_vector_cut(const unsigned char *in, unsigned char *out, size_t in_item_bytes, size_t shift_bytes,
                             size_t out_item_bytes, int nitems, hipStream_t s);
hipError_t launch_phase_window(const float2 *in, float2 *out, const float2 *win, int l, int R, int shift,
                               int counter0, int nitems, hipStream_t s);

}  // namespace fdc
