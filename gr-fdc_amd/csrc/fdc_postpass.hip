// gfx950 (MI355X, CDNA4) kernels of the frequency-domain channelizer — the passes that run BEHIND a plan's kernels, over the channel-major float
// results of a launch group: the rotation of fine tuning (k_fine_rotate), the channel gains (k_chan_gain), the channel levels (k_chan_levels), the
// channel lag-1 correlation (k_chan_lag1) and the narrowing to complex integers (k_complex_to_iq) — and, over a whole call's float results in the
// place of the narrowing, the channel demodulation (k_chan_demod) and behind it the channel audio (k_chan_audio, at the end of this file), which the
// channel squelch (k_chan_squelch, over the call's levels) gates and, with the audio packing on, the offsets (k_pack_rows, k_pack_scan, over the
// call's mask) place.  Which of them a call runs, and in which order, is decided once per call: PostPass, fdc_enqueue.hip.
//
// One shape for the four per-channel kernels: grid y = channel, a row — the lout samples of one (block, channel) — on a power-of-two set of lanes of one
// wave, 16 bytes per lane and access where the row allows it (lout even, the channel's run 16-byte aligned), 8 bytes otherwise, a grid-stride loop over
// the blocks (channel_grids).  k_chan_levels and k_chan_gain are one loop, walk_rows, with an operation each; it keeps four loads in flight per lane.
// k_chan_lag1 has the same loop written out (lag1_rows): it also needs the sample in front of each pair, which another lane holds.
// k_fine_rotate keeps its own, one-deep loop: moving it onto walk_rows changes how many loads it keeps in flight, which is a speed change to be measured
// on its own.
#include "fdc_kernels.h"
#include <algorithm>
#include <type_traits>
#include "fdc_iq.hpp"
#include "fdc_fine.hpp"
#include "fdc_devutil.hpp"

namespace fdc {

// grid x * 4 waves stride over the rows of a channel (about eight workgroups per unit); grid y = channel, in pieces of 32768 channels.
// launch(grid, c0) enqueues one piece
template <class F>
static hipError_t channel_grids(int nchan, int nb_chunk, F launch)
{
    if (nchan <= 0 || nb_chunk <= 0) return hipSuccess;
    for (int c0 = 0; c0 < nchan; c0 += 32768) {
        const int nc = nchan - c0 < 32768 ? nchan - c0 : 32768;
        const int gx = std::max(1, std::min((nb_chunk + 3) / 4, (2048 + nc - 1) / nc));
        launch(dim3((unsigned)gx, (unsigned)nc), c0);
    }
    return hipGetLastError();
}

// a run-time bool as a compile-time one: f(std::true_type) or f(std::false_type)
template <class F>
static void with_bool(bool b, F f)
{
    if (b) f(std::true_type{}); else f(std::false_type{});
}

// complex float -> complex integer samples, times scale (fdc_iq.hpp oq_narrow): the narrowing back end of the plans without integer stores of their own
template <class TO>
__global__ __launch_bounds__(256) void k_complex_to_iq(const float2 *__restrict__ in, TO *__restrict__ out, size_t n, float scale)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = oq_narrow(TO{}, from2(in[i]), scale);
}

hipError_t launch_complex_to_iq(int fmt, float scale, const float2 *in, void *out, size_t n, hipStream_t s)
{
    if (!n) return hipSuccess;
    size_t g = (n + 255) / 256; if (g > 8192) g = 8192;
    hipError_t e = hipErrorInvalidValue;                        // stays if fmt is no integer format
    for_int_samples(fmt, [&](auto t) {
        hipLaunchKernelGGL(k_complex_to_iq<decltype(t)>, dim3((unsigned)g), dim3(256), 0, s, in, static_cast<decltype(t) *>(out), n, scale);
        e = hipGetLastError();
    });
    return e;
}

// Channel levels (fdc_pipeline_set_levels): power = sum of re^2 + im^2 and peak = max of |re|, |im| (fmax: a NaN component is passed over) of one row.
// ONE ORDER PER SUM: the bits of a row's power depend on lout and the row's samples only.  The row goes to 2^lev_log2_lanes(lout) lanes of one wave, by
// lout alone; lane `sub` takes the sample PAIRS sub, sub + lanes, ... in index order, of a pair the even sample first; a term is (re re + im im), each
// product and each sum rounded on its own (no FMA contraction, as fine_mul and oq_bits); the lanes are joined by an xor butterfly from distance 1
// upwards.  Both access widths of every kernel that sums (walk_rows, k_fine_rotate<true>) keep exactly this, so neither the row's alignment nor how the
// stream was cut, nor which kernel summed it, shows in the result.  No atomics, no LDS.
struct LevAcc { float sum, peak; };

// the lanes of a row of `per` accesses: log2 of the next power of two, a wave at the most
__device__ __forceinline__ unsigned row_log2_lanes(unsigned per)
{
    const unsigned lg = per <= 1 ? 0 : 32 - (unsigned)__clz((int)(per - 1));
    return lg > 6 ? 6 : lg;
}
__device__ __forceinline__ unsigned lev_log2_lanes(unsigned lout) { return row_log2_lanes((lout + 1) >> 1); }

// a lane starts from (0, NaN): a lane without samples adds +0 and its NaN is passed over by fmax; a row of NaN only keeps NaN (np.fmax.reduce)
__device__ __forceinline__ LevAcc lev_zero() { return LevAcc{0.0f, __builtin_nanf("")}; }

__device__ __forceinline__ void lev_add(LevAcc &a, cf y)
{
#pragma clang fp contract(off)
    const float p = y.x * y.x, q = y.y * y.y;
    const float t = p + q;
    a.sum = a.sum + t;
    a.peak = fmaxf(a.peak, fmaxf(fabsf(y.x), fabsf(y.y)));
}

// the row's 2^lg lanes joined: every lane of the row ends with the row's values (float addition commutes, so with the same bits)
__device__ __forceinline__ void lev_join(LevAcc &a, unsigned lg)
{
    for (unsigned d = 1; d < (1u << lg); d <<= 1) {
        a.sum = a.sum + __shfl_xor(a.sum, (int)d, 64);
        a.peak = fmaxf(a.peak, __shfl_xor(a.peak, (int)d, 64));
    }
}

// where the levels of channel c go: row m of the launch group is block mbase + m of the call
struct LevDst {
    float2 *levels; int mbase, nchan, c;
    __device__ __forceinline__ void store(unsigned m, LevAcc acc) const
    {
        levels[(size_t)(mbase + (int)m) * (size_t)nchan + (size_t)c] = make_float2(acc.sum, acc.peak);
    }
};

// the channel gain (fdc_pipeline_set_gains): each component times gain[c], rounded once, on its own
__device__ __forceinline__ cf gain_mul(cf y, float g) { return mk(iq_mul(y.x, g), iq_mul(y.y, g)); }

// Fine tuning behind the channel kernels of a launch group (fdc_fine.hpp): blocks [mbase, mbase + nb) of the call's channel-major float outputs, in
// place; a channel's rows of the group are one contiguous run, a row has one base (the step table's rows start at even offsets, so a 16-byte row
// reads 16-byte steps).  GAIN: the turned sample times gain[c] (gain_mul), and it is the gained sample that is stored and reduced.  LEVELS: the
// samples are reduced while the lane holds them and one lane of the row stores the row's levels; the lanes then take sample pairs in both access
// widths (the levels' one order).  Without LEVELS an 8-byte row spreads its samples over the lanes instead: contiguous 8-byte accesses.
// gain, levels and nchan are null / 0 where the form does not use them.
template <bool LEVELS, bool GAIN>
__global__ __launch_bounds__(256) void k_fine_rotate(float2 *out, const ChanDev *__restrict__ chans, const FineChan *__restrict__ fine,
                                                     const float2 *__restrict__ step, const float *__restrict__ gain, float2 *levels, int c0, int nchan,
                                                     int nb, int mbase, long long nb_call, unsigned long long first_block)
{
    const int c = c0 + (int)blockIdx.y;
    const unsigned lout = (unsigned)chans[c].lout;
    const FineChan fc = fine[c];
    float g = 1.0f;
    if constexpr (GAIN) g = gain[c];
    float2 *o = out + nb_call * chans[c].out_off + (long long)mbase * lout;
    const float2 *st = step + fc.step_off;
    const bool wide = !(lout & 1) && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
    const unsigned per = LEVELS || wide ? (lout + 1) >> 1 : lout;                  // accesses per row: pairs, or the samples of an 8-byte row without levels
    const unsigned lg = row_log2_lanes(per);
    const unsigned lanes = 1u << lg, lane = threadIdx.x & 63, sub = lane & (lanes - 1), rows = 64u >> lg;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const LevDst dst{levels, mbase, nchan, c};
    // (whole waves leave together: the trip count depends on the wave alone, so every lane of a row is there for the butterfly)
    for (unsigned m0 = wave * rows; m0 < (unsigned)nb; m0 += nwaves * rows) {
        const unsigned m = m0 + (lane >> lg);
        const bool live = m < (unsigned)nb;
        LevAcc acc = lev_zero();
        if (live) {
            const cf base = fine_base(fc.inc, first_block + (unsigned long long)(mbase + (int)m), lout);
            float2 *row = o + (size_t)m * lout;
            if (wide) {
                for (unsigned i = sub; i < per; i += lanes) {
                    const float4 y = ld4(row + 2 * i), s = ld4(st + 2 * i);
                    cf a = fine_rotate(mk(y.x, y.y), base, mk(s.x, s.y)), b = fine_rotate(mk(y.z, y.w), base, mk(s.z, s.w));
                    if constexpr (GAIN) { a = gain_mul(a, g); b = gain_mul(b, g); }
                    st4(row + 2 * i, a, b);
                    if constexpr (LEVELS) { lev_add(acc, a); lev_add(acc, b); }
                }
            } else {
                // LEVELS: i counts pairs, whose odd sample the last one of an odd row lacks; else i counts samples
                constexpr unsigned k = LEVELS ? 2 : 1;
                for (unsigned i = sub; i < per; i += lanes) {
#pragma unroll
                    for (unsigned j = k * i; j < k * i + k; j++) {
                        if (j < lout) {
                            cf a = fine_rotate(ld2(row + j), base, ld2(st + j));
                            if constexpr (GAIN) a = gain_mul(a, g);
                            st2(row + j, a);
                            if constexpr (LEVELS) lev_add(acc, a);
                        }
                    }
                }
            }
        }
        if constexpr (LEVELS) {
            lev_join(acc, lg);
            if (live && sub == 0) dst.store(m, acc);
        }
    }
}

// levels: null = fine tuning alone; else the levels of the call's block 0 ([block][nchan] float2): the turned samples are reduced in the same pass
// gain: null = none; else the nchan channel gains: the turned samples are multiplied in the same pass, in front of the reduction
hipError_t launch_fine_rotate(float2 *out, const ChanDev *chans, const FineChan *fine, const float2 *step, int nchan, int nb_chunk, int mbase, int nb_call,
                              int64_t first_block, hipStream_t s, float2 *levels, const float *gain)
{
    return channel_grids(nchan, nb_chunk, [&](dim3 grid, int c0) {
        with_bool(levels != nullptr, [&](auto lv) {
            with_bool(gain != nullptr, [&](auto gn) {
                hipLaunchKernelGGL((k_fine_rotate<decltype(lv)::value, decltype(gn)::value>), grid, dim3(256), 0, s, out, chans, fine, step, gain, levels, c0,
                                   nchan, nb_chunk, mbase, (long long)nb_call, (unsigned long long)first_block);
            });
        });
    });
}

// The row walker of k_chan_levels and k_chan_gain: the rows [0, nb) of one channel's run `o`, each row on 2^lev_log2_lanes(lout) lanes, the lanes taking
// sample pairs (the levels' one order, above); WIDE: one 16-byte load per pair, else two 8-byte loads.  A trip issues all its loads — four pairs per
// lane: four rows where a row is one pair per lane, four steps along a longer row — before the first is used.
// (no branch around a load: a lane without a pair of its own loads one that exists — the row's last pair, the group's last row — and leaves it out, so
// that the four loads of a trip are in flight together and not each behind its own wait)
// The walker owns which lane holds which pair of which row; what happens to a held pair is the operation's:
//   op.transform(a, b)         the pair's two samples, changed in place (any lane, any pair: no side effect)
//   op.store(m, i, a, b)       pair i of row m, the lane's own: b is a sample of the row where 2 i + 1 < lout
//   Op::kLevels, op.dst        whether the transformed samples are reduced, and where the row's levels go
template <bool WIDE>
__device__ __forceinline__ void row_load(const float2 *row, unsigned i, unsigned lout, cf &a, cf &b)
{
    if (WIDE) {
        const float4 y = ld4(row + 2 * i);
        a = mk(y.x, y.y); b = mk(y.z, y.w);
    } else {
        a = ld2(row + 2 * i);
        b = ld2(row + (2 * i + 1 < lout ? 2 * i + 1 : lout - 1));
    }
}

template <bool WIDE, class Op>
__device__ __forceinline__ void walk_rows(const float2 *o, unsigned lout, unsigned nb, const Op &op)
{
    const unsigned npair = (lout + 1) >> 1, lg = lev_log2_lanes(lout);
    const unsigned lanes = 1u << lg, lane = threadIdx.x & 63, sub = lane & (lanes - 1), rows = 64u >> lg;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    if (npair <= lanes) {
        // a row is at most one pair per lane: four rows per trip, a grid stride apart
        const bool has = sub < npair, two = 2 * sub + 1 < lout;
        const unsigned i = has ? sub : npair - 1;
        for (unsigned m0 = wave * rows; m0 < nb; m0 += 4 * nwaves * rows) {
            cf a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const unsigned m = m0 + (unsigned)u * nwaves * rows + (lane >> lg);
                row_load<WIDE>(o + (size_t)(m < nb ? m : nb - 1) * lout, i, lout, a[u], b[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const unsigned m = m0 + (unsigned)u * nwaves * rows + (lane >> lg);
                op.transform(a[u], b[u]);
                if (has && m < nb) op.store(m, i, a[u], b[u]);
                if constexpr (Op::kLevels) {
                    LevAcc acc = lev_zero();
                    if (has) { lev_add(acc, a[u]); if (two) lev_add(acc, b[u]); }
                    lev_join(acc, lg);
                    if (m < nb && sub == 0) op.dst.store(m, acc);
                }
            }
        }
    } else {
        // a long row (more than 64 pairs) takes the whole wave: four steps of the row per trip, in index order
        for (unsigned m = wave; m < nb; m += nwaves) {
            const float2 *row = o + (size_t)m * lout;
            LevAcc acc = lev_zero();
            for (unsigned i0 = sub; i0 < npair; i0 += 4 * lanes) {
                cf a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const unsigned i = i0 + (unsigned)u * lanes;
                    row_load<WIDE>(row, i < npair ? i : npair - 1, lout, a[u], b[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const unsigned i = i0 + (unsigned)u * lanes;
                    if (i < npair) {
                        op.transform(a[u], b[u]);
                        op.store(m, i, a[u], b[u]);
                        if constexpr (Op::kLevels) { lev_add(acc, a[u]); if (2 * i + 1 < lout) lev_add(acc, b[u]); }
                    }
                }
            }
            if constexpr (Op::kLevels) {
                lev_join(acc, lg);
                if (sub == 0) op.dst.store(m, acc);
            }
        }
    }
}

// Channel levels of a launch group: blocks [mbase, mbase + nb) of the call's channel-major float outputs, read once; one float2 (power, peak) per
// (block, channel) goes to levels[(mbase + m) * nchan + c] and nothing else is written: the walker with "accumulate only"
struct LevelsOp {
    static constexpr bool kLevels = true;
    LevDst dst;
    __device__ __forceinline__ void transform(cf &, cf &) const {}
    __device__ __forceinline__ void store(unsigned, unsigned, cf, cf) const {}
};

__global__ __launch_bounds__(256) void k_chan_levels(const float2 *__restrict__ out, const ChanDev *__restrict__ chans, float2 *__restrict__ levels, int c0,
                                                     int nchan, int nb, int mbase, long long nb_call)
{
    const int c = c0 + (int)blockIdx.y;
    const unsigned lout = (unsigned)chans[c].lout;
    const float2 *o = out + nb_call * chans[c].out_off + (long long)mbase * lout;
    const LevelsOp op{{levels, mbase, nchan, c}};
    if (!(lout & 1) && (reinterpret_cast<uintptr_t>(o) & 15) == 0) walk_rows<true>(o, lout, (unsigned)nb, op);
    else walk_rows<false>(o, lout, (unsigned)nb, op);
}

hipError_t launch_chan_levels(const float2 *out, const ChanDev *chans, float2 *levels, int nchan, int nb_chunk, int mbase, int nb_call, hipStream_t s)
{
    return channel_grids(nchan, nb_chunk, [&](dim3 grid, int c0) {
        hipLaunchKernelGGL(k_chan_levels, grid, dim3(256), 0, s, out, chans, levels, c0, nchan, nb_chunk, mbase, (long long)nb_call);
    });
}

// Channel lag-1 correlation (fdc_pipeline_set_lag1): S = sum over j = 1 .. lout - 1 of y[j] conj(y[j - 1]) of one row, the row's own samples only.
// ONE ORDER PER SUM, the levels': the row on 2^lev_log2_lanes(lout) lanes, lane `sub` the pairs sub, sub + lanes, ... in index order; the lane that owns
// pair i adds y[2i] conj(y[2i - 1]) where i >= 1, then y[2i + 1] conj(y[2i]) where 2i + 1 < lout; a term a conj(b) is (a.x b.x + a.y b.y, a.y b.x -
// a.x b.y), every product and sum rounded on its own, Re and Im summed apart from +0; the lanes joined by the xor butterfly from distance 1 upwards.
struct LagAcc { float re, im; };

__device__ __forceinline__ void lag_add(LagAcc &s, cf a, cf b)
{
#pragma clang fp contract(off)
    const float p = a.x * b.x, q = a.y * b.y;
    const float t = p + q;
    s.re = s.re + t;
    const float u = a.y * b.x, v = a.x * b.y;
    const float w = u - v;
    s.im = s.im + w;
}

__device__ __forceinline__ void lag_join(LagAcc &s, unsigned lg)
{
    for (unsigned d = 1; d < (1u << lg); d <<= 1) {
        s.re = s.re + __shfl_xor(s.re, (int)d, 64);
        s.im = s.im + __shfl_xor(s.im, (int)d, 64);
    }
}

// the value of the lane below (lane 0: its own), and of lane 63; both are run by the whole wave
__device__ __forceinline__ cf lane_below(cf v) { return mk(__shfl_up(v.x, 1, 64), __shfl_up(v.y, 1, 64)); }
__device__ __forceinline__ cf lane_63(cf v)
{
    return mk(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), 63)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), 63)));
}

// The rows [0, nb) of one channel's run `o`, in the shape of walk_rows: four pairs per lane and trip, all loaded before the first is used, a lane
// without a pair of its own loading one that exists and leaving it out.  The sample in front of pair i, y[2i - 1], is the odd sample of pair i - 1:
// the lane below holds it (lane_below), or, for lane 0 of a row that takes the whole wave, lane 63 at the step before (lane_63: a register of this
// trip, or `carry` from the trip before).  Every loop here has a trip count that depends on the wave alone and the moves across lanes stand outside
// every per-lane condition, so the whole wave runs them.  A lane that loaded a substitute is never below a lane with a first term: the pair below
// pair i < npair is pair i - 1, a pair of the row with both its samples; and lane sub = 0 of a row of fewer than 64 lanes takes no first term, so
// what lane_below hands it from the neighbouring row is not used.
// g (GAINED: the narrowing gain pass runs in front and leaves the float results as they were cut): the samples times g first (gain_mul), which
// are the bits the in-place gain pass would have left.
template <bool WIDE, bool GAINED>
__device__ __forceinline__ void lag1_rows(const float2 *o, unsigned lout, unsigned nb, float g, float2 *lag1, int mbase, int nchan, int c)
{
    const unsigned npair = (lout + 1) >> 1, lg = lev_log2_lanes(lout);
    const unsigned lanes = 1u << lg, lane = threadIdx.x & 63, sub = lane & (lanes - 1), rows = 64u >> lg;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    float2 *dst = lag1 + (size_t)mbase * (size_t)nchan + (size_t)c;
    if (npair <= lanes) {
        // a row is at most one pair per lane: four rows per trip, a grid stride apart
        const bool has = sub < npair, first = has && sub >= 1, two = 2 * sub + 1 < lout;
        const unsigned i = has ? sub : npair - 1;
        for (unsigned m0 = wave * rows; m0 < nb; m0 += 4 * nwaves * rows) {
            cf a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const unsigned m = m0 + (unsigned)u * nwaves * rows + (lane >> lg);
                row_load<WIDE>(o + (size_t)(m < nb ? m : nb - 1) * lout, i, lout, a[u], b[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const unsigned m = m0 + (unsigned)u * nwaves * rows + (lane >> lg);
                if (GAINED) { a[u] = gain_mul(a[u], g); b[u] = gain_mul(b[u], g); }
                const cf z = lane_below(b[u]);
                LagAcc acc{0.0f, 0.0f};
                if (first) lag_add(acc, a[u], z);
                if (has && two) lag_add(acc, b[u], a[u]);
                lag_join(acc, lg);
                if (m < nb && sub == 0) dst[(size_t)m * (size_t)nchan] = make_float2(acc.re, acc.im);
            }
        }
    } else {
        // a long row (more than 64 pairs) takes the whole wave: four steps of the row per trip, in index order
        for (unsigned m = wave; m < nb; m += nwaves) {
            const float2 *row = o + (size_t)m * lout;
            LagAcc acc{0.0f, 0.0f};
            cf carry = mk(0.0f, 0.0f);                          // the odd sample of the lane's last pair of the trip before
            for (unsigned i0 = 0; i0 < npair; i0 += 4 * 64) {
                cf a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const unsigned i = i0 + (unsigned)u * 64 + lane;
                    row_load<WIDE>(row, i < npair ? i : npair - 1, lout, a[u], b[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const unsigned i = i0 + (unsigned)u * 64 + lane;
                    if (i0 + (unsigned)u * 64 >= npair) break;          // (the same for the whole wave) no lane has a pair at this step or behind it
                    if (GAINED) { a[u] = gain_mul(a[u], g); b[u] = gain_mul(b[u], g); }
                    const cf below = lane_below(b[u]), wrap = lane_63(u ? b[u - 1] : carry);
                    const cf z = lane ? below : wrap;
                    if (i < npair) {
                        if (i >= 1) lag_add(acc, a[u], z);
                        if (2 * i + 1 < lout) lag_add(acc, b[u], a[u]);
                    }
                }
                carry = b[3];
            }
            lag_join(acc, lg);
            if (lane == 0) dst[(size_t)m * (size_t)nchan] = make_float2(acc.re, acc.im);
        }
    }
}

// Channel lag-1 correlation of a launch group: blocks [mbase, mbase + nb) of the call's channel-major float results, read once; one float2 (Re S, Im S)
// per (block, channel) goes to lag1[(mbase + m) * nchan + c] and nothing else is written.  gain: null, or the channel gains the samples are to be
// multiplied by first
__global__ __launch_bounds__(256) void k_chan_lag1(const float2 *__restrict__ out, const ChanDev *__restrict__ chans, const float *__restrict__ gain,
                                                   float2 *__restrict__ lag1, int c0, int nchan, int nb, int mbase, long long nb_call)
{
    const int c = c0 + (int)blockIdx.y;
    const unsigned lout = (unsigned)chans[c].lout;
    const float2 *o = out + nb_call * chans[c].out_off + (long long)mbase * lout;
    const bool wide = !(lout & 1) && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
    if (gain) {
        const float g = gain[c];
        if (wide) lag1_rows<true, true>(o, lout, (unsigned)nb, g, lag1, mbase, nchan, c);
        else lag1_rows<false, true>(o, lout, (unsigned)nb, g, lag1, mbase, nchan, c);
    } else {
        if (wide) lag1_rows<true, false>(o, lout, (unsigned)nb, 1.0f, lag1, mbase, nchan, c);
        else lag1_rows<false, false>(o, lout, (unsigned)nb, 1.0f, lag1, mbase, nchan, c);
    }
}

hipError_t launch_chan_lag1(const float2 *out, const ChanDev *chans, const float *gain, float2 *lag1, int nchan, int nb_chunk, int mbase, int nb_call,
                            hipStream_t s)
{
    return channel_grids(nchan, nb_chunk, [&](dim3 grid, int c0) {
        hipLaunchKernelGGL(k_chan_lag1, grid, dim3(256), 0, s, out, chans, gain, lag1, c0, nchan, nb_chunk, mbase, (long long)nb_call);
    });
}

// Channel gains of a launch group where no rotation pass runs (fdc_pipeline_set_gains): blocks [mbase, mbase + nb) of the call's channel-major float
// results times gain[c] (gain_mul): the walker with "gain, store, accumulate if LEVELS".  TO = float2: the product goes back where it was read (in
// place).  TO = sc16 / sc8: the float staging is read only and oq_narrow(TO, product, scale) goes to the same sample offset of the call's narrow output
// `nar` — two samples per store where the row is read 16 bytes at a time and the narrow run is aligned for it (pair), one otherwise.  LEVELS: the gained
// samples are reduced in the levels' one order, so k_chan_levels is not launched behind this kernel.
template <bool WIDE, bool LEVELS, class TO>
struct GainOp {
    static constexpr bool kLevels = LEVELS;
    float2 *o; TO *nar; unsigned lout; bool pair; float g, scale;      // o, nar: the channel's run in the float results and in the narrow output
    LevDst dst;
    __device__ __forceinline__ void transform(cf &a, cf &b) const { a = gain_mul(a, g); b = gain_mul(b, g); }
    __device__ __forceinline__ void store(unsigned m, unsigned i, cf a, cf b) const
    {
        if constexpr (std::is_same<TO, float2>::value) {
            float2 *row = o + (size_t)m * lout;
            if (WIDE) st4(row + 2 * i, a, b);
            else { st2(row + 2 * i, a); if (2 * i + 1 < lout) st2(row + 2 * i + 1, b); }
        } else {
            TO *nrow = nar + (size_t)m * lout;
            if (pair) {
                if constexpr (std::is_same<TO, sc16>::value) *reinterpret_cast<uint2 *>(nrow + 2 * i) = make_uint2(oq_bits(TO{}, a, scale), oq_bits(TO{}, b, scale));
                else *reinterpret_cast<unsigned *>(nrow + 2 * i) = oq_bits(TO{}, a, scale) | (oq_bits(TO{}, b, scale) << 16);
            } else {
                nrow[2 * i] = oq_narrow(TO{}, a, scale);
                if (2 * i + 1 < lout) nrow[2 * i + 1] = oq_narrow(TO{}, b, scale);
            }
        }
    }
};

// (out: read and written for TO = float2, read only otherwise; nar, scale: the narrow forms' output and its factor; levels, nchan: the LEVELS forms')
template <bool LEVELS, class TO = float2>
__global__ __launch_bounds__(256) void k_chan_gain(float2 *out, const ChanDev *__restrict__ chans, const float *__restrict__ gain, TO *nar, float scale,
                                                   float2 *__restrict__ levels, int c0, int nchan, int nb, int mbase, long long nb_call)
{
    const int c = c0 + (int)blockIdx.y;
    const unsigned lout = (unsigned)chans[c].lout;
    const long long run = nb_call * chans[c].out_off + (long long)mbase * lout;      // the channel's run of this launch group, in samples of either output
    float2 *o = out + run;
    TO *n = std::is_same<TO, float2>::value ? nullptr : nar + run;
    const bool wide = !(lout & 1) && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
    const bool pair = wide && (reinterpret_cast<uintptr_t>(n) & (2 * sizeof(TO) - 1)) == 0;
    const LevDst dst{levels, mbase, nchan, c};
    if (wide) walk_rows<true>(o, lout, (unsigned)nb, GainOp<true, LEVELS, TO>{o, n, lout, pair, gain[c], scale, dst});
    else walk_rows<false>(o, lout, (unsigned)nb, GainOp<false, LEVELS, TO>{o, n, lout, false, gain[c], scale, dst});
}

// fmt 0: in place on `out`; kIqSc16 / kIqSc8: `out` read, oq_narrow(product, scale) to `nar`.  levels: null = none
hipError_t launch_chan_gain(float2 *out, const ChanDev *chans, const float *gain, float2 *levels, int fmt, float scale, void *nar, int nchan, int nb_chunk,
                            int mbase, int nb_call, hipStream_t s)
{
    if (nchan <= 0 || nb_chunk <= 0) return hipSuccess;
    if (fmt != kIqFloat && fmt != kIqSc16 && fmt != kIqSc8) return hipErrorInvalidValue;
    if (fmt != kIqFloat && !nar) return hipErrorInvalidValue;
    return channel_grids(nchan, nb_chunk, [&](dim3 grid, int c0) {
        with_bool(levels != nullptr, [&](auto lv) {
            for_samples(fmt, [&](auto t) {                      // float2: in place, no narrow output
                constexpr bool kNarrow = !std::is_same<decltype(t), float2>::value;
                hipLaunchKernelGGL((k_chan_gain<decltype(lv)::value, decltype(t)>), grid, dim3(256), 0, s, out, chans, gain,
                                   static_cast<decltype(t) *>(kNarrow ? nar : nullptr), scale, levels, c0, nchan, nb_chunk, mbase, (long long)nb_call);
            });
        });
    });
}

// Channel demodulation (fdc_pipeline_set_demod): one real float32 sample per complex float32 sample of a call's channel-major float results, 8 bytes
// read and 4 written per sample.  FM: d[t] = gain * atan2f(Im P, Re P), P = y[t] conj(y[t - 1]) with lag_add's products (every product and sum
// rounded on its own); where both components of P compare equal to zero d[t] = +0 (a silent channel, a stream start: no +-pi from signed zeros).
// MAG: d[t] = gain * sqrt(re re + im im), the products, the sum and the correctly rounded root each rounded on their own.
template <int MODE>
__device__ __forceinline__ float demod_one(cf a, cf b, float gain)
{
#pragma clang fp contract(off)
    if constexpr (MODE == kDemodFm) {
        const float p = a.x * b.x, q = a.y * b.y;
        const float re = p + q;
        const float u = a.y * b.x, v = a.x * b.y;
        const float im = u - v;
        const float d = gain * atan2f(im, re);
        return re == 0.0f && im == 0.0f ? 0.0f : d;
    } else {
        const float p = a.x * a.x, q = a.y * a.y;
        const float s = p + q;
        // (sqrtf is the correctly rounded root: hipcc's default, and the Makefile has no fast-math flag.  __fsqrt_rn is the native, 1 ulp instruction in
        // this HIP unless OCML_BASIC_ROUNDED_OPERATIONS is defined)
        return gain * sqrtf(s);
    }
}

// One channel's run of the call: T = nblocks * lout consecutive samples y -> d (a channel's stream is contiguous across the blocks of a call, so the
// sample in front of y[t] is y[t - 1] whatever the block).  A wave takes 256 consecutive samples per trip, a lane four of them: two 16-byte loads and
// one 16-byte store (WIDE: both runs 16-byte aligned; the run's last lane may hold fewer than four), else four 8-byte loads and up to four 4-byte
// stores; the arithmetic is the same, so both give the same bits.  All loads of a trip are issued before the first is used; a lane past the run's
// end loads its last sample and stores nothing.  FM: the sample in front of a lane's first comes from the lane below (lane_below, run by the whole
// wave: the trip count depends on the wave alone and the move stands outside every per-lane condition, as in lag1_rows); lane 0 loads it, 8 bytes
// more: the element in front of the wave's 256, or at t = 0 the carry (cin; null: the stream starts anew, zero).  The lane that holds y[T - 1]
// writes it to cout, the carry of the next call: another buffer than cin, so no workgroup reads what another writes.
template <int MODE, bool WIDE>
__device__ __forceinline__ void demod_run(const float2 *y, float *d, unsigned T, float gain, const float2 *cin, float2 *cout)
{
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    for (unsigned base = wave * 256; base < T; base += nwaves * 256) {
        const unsigned t = base + 4 * lane;
        const bool full = t + 4 <= T;
        cf v[4];
        if (WIDE && full) {
            const float4 lo = ld4(y + t), hi = ld4(y + t + 2);
            v[0] = mk(lo.x, lo.y); v[1] = mk(lo.z, lo.w); v[2] = mk(hi.x, hi.y); v[3] = mk(hi.z, hi.w);
        } else {
#pragma unroll
            for (unsigned j = 0; j < 4; j++) v[j] = ld2(y + (t + j < T ? t + j : T - 1));
        }
        float r[4];
        if constexpr (MODE == kDemodFm) {
            cf front = mk(0.0f, 0.0f);
            if (lane == 0) {
                if (base) front = ld2(y + base - 1);
                else if (cin) front = ld2(cin);
            }
            const cf below = lane_below(v[3]);
            const cf prev = lane ? below : front;
            r[0] = demod_one<MODE>(v[0], prev, gain);
#pragma unroll
            for (unsigned j = 1; j < 4; j++) r[j] = demod_one<MODE>(v[j], v[j - 1], gain);
#pragma unroll
            for (unsigned j = 0; j < 4; j++)
                if (t + j + 1 == T) st2(cout, v[j]);
        } else {
#pragma unroll
            for (unsigned j = 0; j < 4; j++) r[j] = demod_one<MODE>(v[j], v[j], gain);
        }
        if (WIDE && full) {
            *reinterpret_cast<float4 *>(d + t) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (unsigned j = 0; j < 4; j++)
                if (t + j < T) d[t + j] = r[j];
        }
    }
}

// in: the call's float results ([channel][nb_call * lout] float2 at nb_call * out_off); out: its real output, the same element offsets.  carry_in
// (null: no sample in front) and carry_out: [nchan] float2, FM only
template <int MODE>
__global__ __launch_bounds__(256) void k_chan_demod(const float2 *__restrict__ in, float *__restrict__ out, const ChanDev *__restrict__ chans,
                                                    const float2 *__restrict__ carry_in, float2 *__restrict__ carry_out, float gain, int c0,
                                                    long long nb_call)
{
    const int c = c0 + (int)blockIdx.y;
    const long long run = nb_call * chans[c].out_off;
    const unsigned T = (unsigned)(nb_call * chans[c].lout);
    const float2 *y = in + run;
    float *d = out + run;
    const float2 *cin = carry_in ? carry_in + c : nullptr;
    float2 *cout = MODE == kDemodFm ? carry_out + c : nullptr;
    if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) demod_run<MODE, true>(y, d, T, gain, cin, cout);
    else demod_run<MODE, false>(y, d, T, gain, cin, cout);
}

// mode kDemodFm / kDemodMag; sum_lout: the plan's output samples per block (the grid: a wave per 256 samples of a run of mean length)
hipError_t launch_chan_demod(int mode, float gain, const float2 *in, float *out, const ChanDev *chans, const float2 *carry_in, float2 *carry_out, int nchan,
                             int nb_call, long long sum_lout, hipStream_t s)
{
    if (nchan <= 0 || nb_call <= 0) return hipSuccess;
    if (mode != kDemodFm && mode != kDemodMag) return hipErrorInvalidValue;
    if (mode == kDemodFm && !carry_out) return hipErrorInvalidValue;
    const long long trips = ((long long)nb_call * sum_lout / nchan + 255) / 256;
    return channel_grids(nchan, (int)std::max<long long>(1, std::min<long long>(trips, 1 << 20)), [&](dim3 grid, int c0) {
        if (mode == kDemodFm)
            hipLaunchKernelGGL(k_chan_demod<kDemodFm>, grid, dim3(256), 0, s, in, out, chans, carry_in, carry_out, gain, c0, (long long)nb_call);
        else
            hipLaunchKernelGGL(k_chan_demod<kDemodMag>, grid, dim3(256), 0, s, in, out, chans, carry_in, carry_out, gain, c0, (long long)nb_call);
    });
}

// Channel squelch (fdc_pipeline_set_squelch): per channel a state machine over the blocks of the stream — open at a block whose power reaches the
// open threshold, held while it reaches the close threshold, closed after hang + 1 consecutive blocks below it — in the PARALLEL form
// tests/squelch_model.py proves equal to the sequential rule.  With strong = (p >= To) and low = neither p >= To nor p >= Tc, block m is open iff a
// strong block lies at or before m and no run of hang + 1 consecutive low blocks has ended behind that strong block and at or before m.  Three
// inclusive max-scans over the block index give that: s = the last strong block, nl = the last block that is not low (m - nl is the length of the run
// of low blocks that ends at m), e = the last block at which that length reached hang + 1; open = s > e.  A carried open state (1, h) stands for
// a strong block at index -1 - (hang - h) with hang - h low blocks behind it; a closed one for none (kSqNeg).  The scans are on integers, so
// the order in which they are joined does not show in the result.
// One workgroup per channel.  A trip covers 256 * kSqPer consecutive blocks, a lane kSqPer consecutive ones: the lane walks its own blocks, the lanes
// of a wave are joined by __shfl_up, the four waves through LDS, the trips by a carry every lane holds.  The trip count depends on nb alone and both
// barriers of a trip stand outside every per-lane condition (the rule of lag1_rows); the LDS slots alternate with the trip, so no third barrier guards
// them.  The powers of the next trip are loaded before this trip's scans.  The thread that decides block nb - 1 writes the new state, to ANOTHER
// buffer than the one read.
// kSqPer = 16 (4096 blocks a trip).  On a call of four channels and 16384 blocks (four workgroups) it takes about 0.025 ms, 0.86 of k_chan_levels
// (profiles/squelch/README.md), and WHAT BOUNDS IT THERE HAS NOT BEEN MEASURED.  Known: 8 blocks a lane, twice the trips, took the same time within
// the spread, so the trip count alone is not it.  A hypothesis from the code: within one load or store instruction every lane touches another
// cache line (rows of C (power, peak) pairs, a lane's rows 16 apart), so a compute unit issues 64 line requests per instruction, although a lane's
// later loads reuse its lines and the four workgroups read the same ones; latency and launch overhead of four workgroups may weigh as much.
// Staging a trip's rows through LDS with the lanes on consecutive rows, and a wave per channel for short calls, are not built.  At 32 blocks a
// lane the kernel spilled scalar registers.
constexpr int kSqNeg = -(1 << 30);
constexpr unsigned kSqPer = 16;

// inclusive max-scan over the lanes of a wave (run by the whole wave)
__device__ __forceinline__ int wave_max_scan(int v)
{
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, (unsigned)d, 64);
        v = lane >= d && u > v ? u : v;
    }
    return v;
}

// the value in front of this thread's: carry, the waves below (tot: their totals) and the lanes below (inc: the wave's inclusive scan)
__device__ __forceinline__ int scan_front(int inc, int carry, const int *tot, int &total)
{
    const int w = (int)(threadIdx.x >> 6), up = __shfl_up(inc, 1u, 64);
    int below = carry;
    total = carry;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int t = tot[u];
        if (u < w && t > below) below = t;
        if (t > total) total = t;
    }
    return (threadIdx.x & 63) && up > below ? up : below;
}

// levels: row 0 of the call ([nb][nchan] (power, peak)); mask: row 0 of the call's mask ([nb][nchan] bytes); gain: null = all ones;
// state_in: null = every channel (0, 0); state_out: [nchan][2] int (open, h)
__global__ __launch_bounds__(256) void k_chan_squelch(const float2 *__restrict__ levels, const float *__restrict__ gain, const float *__restrict__ thr_open,
                                                      const float *__restrict__ thr_close, const int *__restrict__ state_in, int *__restrict__ state_out,
                                                      unsigned char *__restrict__ mask, int hang, int nchan, int nb)
{
    __shared__ int tot[2][3][4];
    const int c = (int)blockIdx.x;
    const unsigned tid = threadIdx.x, w = tid >> 6;
    float To, Tc;
    {
#pragma clang fp contract(off)
        const float g = gain ? gain[c] : 1.0f;
        const float g2 = g * g;
        To = g2 * thr_open[c];
        Tc = g2 * thr_close[c];
    }
    int cs = kSqNeg, cn = -1, ce = kSqNeg;                  // the carries in front of the trip: last strong, last not low, last run end
    if (state_in) {
        const int so = state_in[2 * c], sh = state_in[2 * c + 1];
        if (so != 0) {
            const int h = sh < 0 ? 0 : sh > hang ? hang : sh;
            cs = cn = -1 - (hang - h);
        }
    }
    const float2 *lv = levels + c;
    unsigned char *mrow = mask + c;
    const unsigned per_trip = 256 * kSqPer;
    float p[kSqPer], pn[kSqPer];
#pragma unroll
    for (unsigned v = 0; v < kSqPer; v++) {
        const unsigned m = tid * kSqPer + v;
        pn[v] = lv[(size_t)(m < (unsigned)nb ? m : (unsigned)nb - 1) * (size_t)nchan].x;
    }
    for (unsigned m0 = 0, par = 0; m0 < (unsigned)nb; m0 += per_trip, par ^= 1) {
        const unsigned mb = m0 + tid * kSqPer;
#pragma unroll
        for (unsigned v = 0; v < kSqPer; v++) p[v] = pn[v];
        if (m0 + per_trip < (unsigned)nb) {                 // (the same for the whole workgroup)
#pragma unroll
            for (unsigned v = 0; v < kSqPer; v++) {
                const unsigned m = mb + per_trip + v;
                pn[v] = lv[(size_t)(m < (unsigned)nb ? m : (unsigned)nb - 1) * (size_t)nchan].x;
            }
        }
        // the lane's own blocks: their classes, its last strong and last not-low block
        unsigned strong = 0, low = 0;
        int ls = kSqNeg, ln = kSqNeg;
#pragma unroll
        for (unsigned v = 0; v < kSqPer; v++) {
            if (mb + v < (unsigned)nb) {
                const bool s = p[v] >= To, l = !s && !(p[v] >= Tc);
                strong |= (unsigned)s << v; low |= (unsigned)l << v;
                if (s) ls = (int)(mb + v);
                if (!l) ln = (int)(mb + v);
            }
        }
        const int is = wave_max_scan(ls), in = wave_max_scan(ln);
        if ((tid & 63) == 63) { tot[par][0][w] = is; tot[par][1][w] = in; }
        __syncthreads();
        int ts, tn, te;
        const int fs = scan_front(is, cs, tot[par][0], ts), fn = scan_front(in, cn, tot[par][1], tn);
        // where a run of low blocks reached hang + 1 among the lane's own
        int n = fn, le = kSqNeg;
#pragma unroll
        for (unsigned v = 0; v < kSqPer; v++) {
            if (mb + v < (unsigned)nb) {
                if (!((low >> v) & 1)) n = (int)(mb + v);
                if ((int)(mb + v) - n >= hang + 1) le = (int)(mb + v);
            }
        }
        const int ie = wave_max_scan(le);
        if ((tid & 63) == 63) tot[par][2][w] = ie;
        __syncthreads();
        const int fe = scan_front(ie, ce, tot[par][2], te);
        // the decisions of the lane's own blocks
        int s = fs, e = fe;
        n = fn;
#pragma unroll
        for (unsigned v = 0; v < kSqPer; v++) {
            const int m = (int)(mb + v);
            if (m < nb) {
                if ((strong >> v) & 1) s = m;
                if (!((low >> v) & 1)) n = m;
                if (m - n >= hang + 1) e = m;
                const int open = s > e;
                mrow[(size_t)m * (size_t)nchan] = (unsigned char)open;
                if (m == nb - 1) { state_out[2 * c] = open; state_out[2 * c + 1] = open ? hang - (m - n) : 0; }
            }
        }
        cs = ts; cn = tn; ce = te;
    }
}

hipError_t launch_chan_squelch(const float2 *levels, const float *gain, const float *thr_open, const float *thr_close, int hang, const int *state_in,
                               int *state_out, unsigned char *mask, int nchan, int nb_call, hipStream_t s)
{
    if (nchan <= 0 || nb_call <= 0) return hipSuccess;
    if (!levels || !thr_open || !thr_close || !state_out || !mask || state_in == state_out || hang < 0 || hang > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chan_squelch, dim3((unsigned)nchan), dim3(256), 0, s, levels, gain, thr_open, thr_close, state_in, state_out, mask, hang,
                       nchan, nb_call);
    return hipGetLastError();
}

// Packed audio (fdc_pipeline_set_audio_packing): where every (block, channel) of the call goes in the packed buffer.  The weight of a cell is
// mask[m][c] * npb_c (npb_c = lout_c / D, the cell's audio samples), the cells are ordered block-major, off[m][c] is base + the sum of the weights of
// all cells in front of (m, c) (closed cells too: where they would go) and total is base + the sum over all.  Integers only, so the order of
// the sums does not show.  Three launches, none of which waits for another workgroup:
//   k_pack_rows<L, false>  the sum of every row, parked in the row's own first word off[m][0] (no scratch: the footprint is the table's);
//   k_pack_scan            ONE workgroup turns the nb row sums into the rows' bases, in place: a trip covers 256 * kPackPer = 1024 consecutive rows,
//                          a lane kPackPer = 4 consecutive ones, the lanes of a wave are joined by __shfl_up, the four waves through LDS, the trips
//                          by a carry every lane holds (k_chan_squelch's scheme).  The trip count depends on nb alone, the one barrier of a trip
//                          stands outside every per-lane condition, and the LDS slots alternate with the trip, so no second barrier guards them.
//                          It reads base_in (null: 0) in front of its first barrier and writes total behind its last, so both may be one word;
//   k_pack_rows<L, true>   every row again: its base (off[m][0]) plus the exclusive scan along the row, into off[m][c].
// The lane mapping of k_pack_rows goes by the channel count: up to kPackSerial channels a lane takes a row and walks it (L = 1; four channels are
// four bytes of mask), above that a wave takes a row, 64 channels a trip, joined by __shfl_up with a carry (L = 64).  No barrier in either.
constexpr unsigned kPackPer = 4;
constexpr int kPackSerial = 8;

template <class T>
__device__ __forceinline__ T wave_sum_scan(T v)                   // inclusive, run by the whole wave
{
    const unsigned lane = threadIdx.x & 63;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

template <int L, bool WRITE>
__global__ __launch_bounds__(256) void k_pack_rows(const unsigned char *__restrict__ mask, const ChanDev *__restrict__ chans, unsigned *off, int D,
                                                   int nchan, int nb)
{
    static_assert(L == 1 || L == 64, "a lane or a wave per row");
    const unsigned rows = 256 / L;                                  // rows a workgroup takes per trip
    for (unsigned m = blockIdx.x * rows + threadIdx.x / L; m < (unsigned)nb; m += gridDim.x * rows) {      // (L = 64: the same for the whole wave)
        const unsigned char *mr = mask + (size_t)m * (size_t)nchan;
        unsigned *orow = off + (size_t)m * (size_t)nchan;
        unsigned run = WRITE ? orow[0] : 0u;                        // the row's base (WRITE stores the same value back as cell 0's offset)
        if constexpr (L == 1) {
            for (int c = 0; c < nchan; c++) {
                const unsigned w = mr[c] ? (unsigned)chans[c].lout / (unsigned)D : 0u;
                if (WRITE) orow[c] = run;
                run += w;
            }
        } else {
            const unsigned lane = threadIdx.x & 63;
            for (int c0 = 0; c0 < nchan; c0 += 64) {                // (the trip count is the wave's)
                const int c = c0 + (int)lane;
                const unsigned w = c < nchan && mr[c] ? (unsigned)chans[c].lout / (unsigned)D : 0u;
                const unsigned inc = wave_sum_scan(w);
                if (WRITE && c < nchan) orow[c] = run + inc - w;
                run += __shfl(inc, 63, 64);
            }
        }
        if (!WRITE && (L == 1 || (threadIdx.x & 63) == 0)) orow[0] = run;
    }
}

// off: row m's sum at off[m * pitch] in, row m's base out; base_in (null: 0) and total may be the same word
__global__ __launch_bounds__(256) void k_pack_scan(unsigned *off, int pitch, int nb, const long long *base_in, long long *total)
{
    __shared__ unsigned long long tot[2][4];
    const unsigned tid = threadIdx.x, wv = tid >> 6;
    unsigned long long carry = base_in ? (unsigned long long)*base_in : 0ull;
    for (unsigned m0 = 0, par = 0; m0 < (unsigned)nb; m0 += 256 * kPackPer, par ^= 1) {
        const unsigned mb = m0 + tid * kPackPer;
        unsigned w[kPackPer];
        unsigned long long s = 0;
#pragma unroll
        for (unsigned v = 0; v < kPackPer; v++) {
            w[v] = mb + v < (unsigned)nb ? off[(size_t)(mb + v) * (size_t)pitch] : 0u;
            s += w[v];
        }
        const unsigned long long inc = wave_sum_scan(s);
        if ((tid & 63) == 63) tot[par][wv] = inc;
        __syncthreads();
        unsigned long long run = carry + inc - s;
#pragma unroll
        for (unsigned u = 0; u < 4; u++) {
            const unsigned long long t = tot[par][u];
            if (u < wv) run += t;
            carry += t;
        }
#pragma unroll
        for (unsigned v = 0; v < kPackPer; v++) {
            if (mb + v < (unsigned)nb) off[(size_t)(mb + v) * (size_t)pitch] = (unsigned)run;
            run += w[v];
        }
    }
    if (tid == 0) *total = (long long)carry;
}

hipError_t launch_audio_pack_offsets(const unsigned char *mask, const ChanDev *chans, int decim, const long long *base_in, unsigned *off, long long *total,
                                     int nchan, int nb_call, hipStream_t s)
{
    if (nchan <= 0 || nb_call <= 0) return hipSuccess;
    if (!mask || !chans || !off || !total || decim < 1) return hipErrorInvalidValue;
    const bool serial = nchan <= kPackSerial;
    const unsigned rows = serial ? 256u : 4u, grid = std::min<unsigned>(((unsigned)nb_call + rows - 1) / rows, 1u << 16);
    if (serial) hipLaunchKernelGGL((k_pack_rows<1, false>), dim3(grid), dim3(256), 0, s, mask, chans, off, decim, nchan, nb_call);
    else hipLaunchKernelGGL((k_pack_rows<64, false>), dim3(grid), dim3(256), 0, s, mask, chans, off, decim, nchan, nb_call);
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(256), 0, s, off, nchan, nb_call, base_in, total);
    if (serial) hipLaunchKernelGGL((k_pack_rows<1, true>), dim3(grid), dim3(256), 0, s, mask, chans, off, decim, nchan, nb_call);
    else hipLaunchKernelGGL((k_pack_rows<64, true>), dim3(grid), dim3(256), 0, s, mask, chans, off, decim, nchan, nb_call);
    return hipGetLastError();
}

// Channel audio (fdc_pipeline_set_audio): the decimating FIR behind the demodulation, a[n] = sum over k = 0 .. K - 1 of h[k] d[n D - k] over one
// channel's run d of the call (T = nblocks * lout real samples, contiguous across the blocks; in front of d[0] stand the K - 1 values of the history,
// or zeros).  THE ORDER IS THE DEFINITION: k ascending from acc = +0, every product and every sum rounded on its own (audio_mac).
// A workgroup takes a TILE of consecutive outputs: the tile's samples — the K - 1 in front of its first output's and D per output — are staged
// in LDS DE-INTERLEAVED BY PHASE: tile sample i at plane i mod D, index i / D.  Output j of the tile reads, for tap k, tile sample j D + (K - 1 - k):
// plane (K - 1 - k) mod D and index j + (K - 1 - k) / D, so the lanes of a wave — consecutive j — read consecutive words of one plane, whatever D
// is (staged in sample order they would read words D apart: a D-way bank conflict).  The plane pitch is ceil(64 / D) modulo 64, so that the 64
// consecutive samples a wave stages fall into different banks where D divides 64.  The tap of a step is the same for the whole workgroup: a scalar
// load.  The staging loops' trip counts depend on the workgroup alone, the computing loop's on the wave alone; the barriers stand outside both and
// outside every per-lane condition.
// The outputs go to the block-major audio matrix: output n of the run is column aoff + n mod (lout / D) of row n / (lout / D).  The workgroup of
// the run's first tile also writes the new history, the last K - 1 values of (what stood in front, d), to ANOTHER buffer than the one read.
constexpr unsigned kAudioLdsWords = 10240;        // 40 KiB: four workgroups per compute unit

struct AudioTile { unsigned pitch, front, outs; };   // plane pitch in words; ceil((K - 1) / D), the planes' words in front of output 0; outputs per tile

__host__ __device__ inline AudioTile audio_tile(unsigned D, unsigned K)
{
    AudioTile t;
    const unsigned w = ((64 + D - 1) / D) & 63;
    t.pitch = kAudioLdsWords / D;
    t.pitch -= (t.pitch - w) & 63;                  // pitch = w modulo 64; D * pitch <= kAudioLdsWords; pitch >= 97 (D <= 64)
    t.front = (K - 1 + D - 1) / D;                  // <= 255 at D = 1, where pitch is 10240; <= 8 where pitch is below 160
    t.outs = t.pitch - t.front;                     // the tile's last sample, outs D + K - 2, has index outs + front - 1 < pitch
    if (t.outs >= 256) t.outs &= ~255u;             // whole trips of a wave's 256 outputs where the tile holds that many
    return t;
}

__device__ __forceinline__ float audio_mac(float acc, float h, float z)
{
#pragma clang fp contract(off)
    const float p = h * z;
    return acc + p;
}

__device__ __forceinline__ void audio_store(float *out, long long at, float a, float) { out[at] = a; }
__device__ __forceinline__ void audio_store(short *out, long long at, float a, float scale) { out[at] = (short)oq_round(a, scale, -32768, 32767); }

// sample t of (history, run): t in [-(K - 1), T)
__device__ __forceinline__ float audio_sample(const float *d, const float *hin, int K, long long t)
{
    return t >= 0 ? d[t] : hin ? hin[K - 1 + t] : 0.0f;
}

// THE GATED FORMS (GATE; the channel squelch on, fdc_pipeline_set_squelch): an output of a closed (block, channel) is stored as zero bits, the
// footprint is the ungated pass's, and the history runs on over the ungated samples.  What they save is the work: a tile none of whose rows is open
// stages nothing and runs no tap loop (every wave looks at the same rows of the mask and joins its lanes by a ballot, so the condition is the same
// for the whole workgroup, and both barriers stand outside it); a wave whose trip of 256 outputs lies in closed rows skips the tap loop; otherwise
// the store selects per output.  The ungated forms take no gate arguments and are the code they were.
__device__ __forceinline__ const unsigned char *gate_mask(const unsigned char *m, int) { return m; }
__device__ __forceinline__ unsigned gate_pitch(const unsigned char *, int nchan) { return (unsigned)nchan; }

// whether any of the rows [r0, r1] of one channel's mask column is open: the same answer in every lane of the wave
__device__ __forceinline__ bool gate_any_open(const unsigned char *col, unsigned pitch, unsigned r0, unsigned r1)
{
    bool open = false;
    for (unsigned r = r0; r <= r1; r += 64) {               // (the trip count is the wave's)
        const unsigned rr = r + (threadIdx.x & 63);
        open = open || (rr <= r1 && col[(size_t)rr * pitch] != 0);
    }
    return __builtin_amdgcn_ballot_w64(open) != 0;
}

// THE PACKED FORMS (GATE with four gate arguments: mask, nchan, offsets, their pitch; fdc_pipeline_set_audio_packing): the outputs of an open
// (block, channel) go to out[off[block][channel] + i], i counting within the block, and a closed output is not stored at all: nothing is stored as
// zero anywhere.  off is what launch_audio_pack_offsets made of the same mask, so the open cells lie one behind the other in block-major order and
// the pass writes exactly `total` elements.  The lanes of a wave hold consecutive outputs, which within a row are consecutive elements of the packed
// buffer as they are of the matrix.  Skipping and the history are the gated forms'.
__device__ __forceinline__ const unsigned char *gate_mask(const unsigned char *m, int, const unsigned *, int) { return m; }
__device__ __forceinline__ unsigned gate_pitch(const unsigned char *, int nchan, const unsigned *, int) { return (unsigned)nchan; }
__device__ __forceinline__ const unsigned *pack_table(const unsigned char *, int, const unsigned *off, int) { return off; }
__device__ __forceinline__ unsigned pack_pitch(const unsigned char *, int, const unsigned *, int pitch) { return (unsigned)pitch; }

// in: the call's demodulated samples ([channel][nb_call * lout] float at nb_call * out_off); out: row 0 of the call's audio ([nb_call][A] TO);
// hist_in (null: zeros) and hist_out (null where K = 1): [nchan][K - 1] float; gate (GATE only): row 0 of the call's mask ([nb_call][nchan] bytes), nchan;
// and, the packed forms only, row 0 of the call's offsets ([nb_call][pitch] words) and pitch: out is then element 0 of the packed buffer
template <class TO, bool GATE, class... Gate>
__global__ __launch_bounds__(256) void k_chan_audio(const float *__restrict__ in, TO *__restrict__ out, const ChanDev *__restrict__ chans,
                                                    const long long *__restrict__ aoff, const float *__restrict__ taps,
                                                    const float *__restrict__ hist_in, float *__restrict__ hist_out, int D, int K, float scale,
                                                    long long A, int c0, long long nb_call, Gate... gate)
{
    static_assert(GATE == (sizeof...(Gate) == 2 || sizeof...(Gate) == 4), "the gated forms take (mask, nchan), the packed ones (mask, nchan, offsets, pitch)");
    constexpr bool PACK = sizeof...(Gate) == 4;
    __shared__ float tile[kAudioLdsWords];
    const int c = c0 + (int)blockIdx.y;
    const unsigned char *gcol = nullptr;                            // GATE: the channel's column of the mask and the pitch of its rows
    unsigned gpitch = 0;
    if constexpr (GATE) { gcol = gate_mask(gate...) + c; gpitch = gate_pitch(gate...); }
    const unsigned lout = (unsigned)chans[c].lout, tid = threadIdx.x;
    const unsigned npb = lout / (unsigned)D;                        // outputs per block
    const unsigned nout = (unsigned)nb_call * npb;
    const long long T = nb_call * (long long)lout;
    const float *d = in + nb_call * chans[c].out_off;
    const float *hin = hist_in ? hist_in + (size_t)c * (size_t)(K - 1) : nullptr;
    TO *o = out;
    if constexpr (!PACK) o += aoff[c];                              // (PACK: out is element 0 of the packed buffer, the offsets place the cell)
    const AudioTile g = audio_tile((unsigned)D, (unsigned)K);
    const unsigned magic = (unsigned)(0x100000000ull / (unsigned)D) + 1u;      // i / D = umulhi(i, magic) for i < 2^16, D >= 2
    // where tile sample i lies in LDS: plane i mod D, index i / D
    const auto lds_at = [&](unsigned i) {
        const unsigned q = D == 1 ? i : __umulhi(i, magic);
        return (i - q * (unsigned)D) * g.pitch + q;
    };
    // (PACK: the new history first, so that its buffer is not held in scalar registers, of which this form needs three more, across the tiles; it
    // depends on the input alone)
    if constexpr (PACK)
        if (blockIdx.x == 0 && tid < (unsigned)(K - 1))
            hist_out[(size_t)c * (size_t)(K - 1) + tid] = audio_sample(d, hin, K, T - (K - 1) + (long long)tid);
    for (unsigned o0 = blockIdx.x * g.outs; o0 < nout; o0 += gridDim.x * g.outs) {
        const unsigned nt = nout - o0 < g.outs ? nout - o0 : g.outs;            // outputs of this tile
        const long long t0 = (long long)o0 * D - (K - 1);
        // GATE: a tile without an open row stages nothing (its samples count as none: no lane below has anything to load), and its waves run no tap
        // loop and store zeros.  The same for the whole workgroup, and both barriers stand outside the condition
        bool tile_open = true;
        if constexpr (GATE) tile_open = gate_any_open(gcol, gpitch, o0 / npb, (o0 + nt - 1) / npb);
        // stage.  The samples in front of the run (the first tile's K - 1) come from the history.  Those of the run are loaded 16 bytes at a time
        // between the 16-byte boundaries inside them, four such loads in flight per lane (a lane past the last quad loads that one again and stores
        // nothing); the up to three samples in front of the first boundary and behind the last are loaded one by one
        const long long tb = t0 < 0 ? 0 : t0;
        if (tile_open && t0 < 0 && tid < (unsigned)(K - 1)) tile[lds_at(tid)] = hin ? hin[tid] : 0.0f;                 // (tile sample i is t = i - (K - 1))
        // element e of da is sample tb - lo + e of the run, da 16-byte aligned: the tile's are [lo, hi), and e is tile sample e + first
        const unsigned lo = (unsigned)((reinterpret_cast<uintptr_t>(d + tb) >> 2) & 3), hi = lo + (tile_open ? (unsigned)((long long)(o0 + nt) * D - tb) : 0u);
        const unsigned first = (unsigned)(tb - t0) - lo;
        const unsigned up = (lo + 3) & ~3u, down = hi & ~3u;
        const unsigned lo4 = up < hi ? up : hi, hi4 = down > lo4 ? down : lo4;      // the quads are [lo4, hi4): lo <= lo4 <= hi4 <= hi
        const float *da = d + tb - lo;
        if (tid < lo4 - lo) tile[lds_at(lo + tid + first)] = da[lo + tid];
        if (tid < hi - hi4) tile[lds_at(hi4 + tid + first)] = da[hi4 + tid];
        for (unsigned q0 = lo4 >> 2, qe = hi4 >> 2; q0 < qe; q0 += 1024) {
            float4 v[4];
#pragma unroll
            for (unsigned u = 0; u < 4; u++) {
                const unsigned q = q0 + u * 256 + tid;
                v[u] = *reinterpret_cast<const float4 *>(da + 4 * (q < qe ? q : qe - 1));
            }
#pragma unroll
            for (unsigned u = 0; u < 4; u++) {
                const unsigned q = q0 + u * 256 + tid, i = 4 * q + first;
                if (q < qe) {
                    tile[lds_at(i)] = v[u].x; tile[lds_at(i + 1)] = v[u].y; tile[lds_at(i + 2)] = v[u].z; tile[lds_at(i + 3)] = v[u].w;
                }
            }
        }
        __syncthreads();
        // compute.  A wave takes 256 consecutive outputs of the tile per trip, a lane four of them, 64 apart: the trip count depends on the wave alone
        for (unsigned j0 = (tid >> 6) * 256; j0 < nt; j0 += 1024) {
            unsigned j[4]; float acc[4];
#pragma unroll
            for (unsigned u = 0; u < 4; u++) {
                const unsigned jj = j0 + u * 64 + (tid & 63);
                j[u] = jj < nt ? jj : nt - 1;                                   // (a lane without an output computes the tile's last and leaves it out)
                acc[u] = 0.0f;
            }
            // GATE: a trip that lies wholly in closed rows runs no tap loop (the same for the whole wave)
            bool taps_run = true;
            if constexpr (GATE) taps_run = tile_open && gate_any_open(gcol, gpitch, (o0 + j0) / npb, (o0 + (j0 + 256 < nt ? j0 + 256 : nt) - 1) / npb);
            // tap k reads tile sample j D + (K - 1 - k): the plane and the index in front go down with k
            unsigned r = (unsigned)(K - 1) % (unsigned)D, at = r * g.pitch + (unsigned)(K - 1) / (unsigned)D;
            // (four taps a trip, which is what the scalar registers hold without a spill: their scalar loads and LDS reads are in flight together, not each behind its own wait)
#pragma unroll 4
            for (int k = 0; k < (taps_run ? K : 0); k++) {
                const float h = taps[k];
#pragma unroll
                for (unsigned u = 0; u < 4; u++) acc[u] = audio_mac(acc[u], h, tile[at + j[u]]);
                if (r) { r--; at -= g.pitch; } else { r = (unsigned)D - 1; at += r * g.pitch - 1; }
            }
#pragma unroll
            for (unsigned u = 0; u < 4; u++) {
                const unsigned jj = j0 + u * 64 + (tid & 63);
                if (jj < nt) {
                    const unsigned n = o0 + jj, m = n / npb;
                    if constexpr (PACK) {
                        // (the table and its pitch are read from the arguments here, not held in scalar registers across the tap loop)
                        if (gcol[(size_t)m * gpitch])
                            audio_store(o, (long long)pack_table(gate...)[m * pack_pitch(gate...) + (unsigned)c] + (long long)(n - m * npb), acc[u], scale);
                    } else {
                        const long long at_out = (long long)m * A + (long long)(n - m * npb);
                        if (GATE && !gcol[(size_t)m * gpitch]) o[at_out] = TO(0);
                        else audio_store(o, at_out, acc[u], scale);
                    }
                }
            }
        }
        __syncthreads();                                                        // the tile is read: the next trip may overwrite it
    }
    if constexpr (!PACK)
        if (blockIdx.x == 0 && tid < (unsigned)(K - 1))
            hist_out[(size_t)c * (size_t)(K - 1) + tid] = audio_sample(d, hin, K, T - (K - 1) + (long long)tid);
}

hipError_t launch_chan_audio(int format, int decim, int ntaps, float scale, const float *taps, const long long *aoff, long long row, const float *in,
                             void *out, const ChanDev *chans, const float *hist_in, float *hist_out, int nchan, int nb_call, long long sum_lout,
                             hipStream_t s, const unsigned char *gate, const unsigned *pack_off)
{
    if (nchan <= 0 || nb_call <= 0) return hipSuccess;
    if (format != kAudioF32 && format != kAudioS16) return hipErrorInvalidValue;
    if (pack_off && !gate) return hipErrorInvalidValue;
    if (decim < 1 || decim > 64 || ntaps < 1 || ntaps > 256 || !taps || !aoff || !in || !out) return hipErrorInvalidValue;
    if (ntaps > 1 && (!hist_out || hist_in == hist_out)) return hipErrorInvalidValue;
    // the grid: a workgroup per tile of a run of mean length (channel_grids takes it in units of four)
    const long long tiles = ((long long)nb_call * sum_lout / nchan / decim) / audio_tile((unsigned)decim, (unsigned)ntaps).outs + 1;
    return channel_grids(nchan, (int)std::min<long long>(4 * tiles, 1 << 20), [&](dim3 grid, int c0) {
        if (pack_off) {
            if (format == kAudioS16)
                hipLaunchKernelGGL((k_chan_audio<short, true, const unsigned char *, int, const unsigned *, int>), grid, dim3(256), 0, s, in,
                                   static_cast<short *>(out), chans, aoff, taps, hist_in, hist_out, decim, ntaps, scale, row, c0, (long long)nb_call, gate,
                                   nchan, pack_off, nchan);
            else
                hipLaunchKernelGGL((k_chan_audio<float, true, const unsigned char *, int, const unsigned *, int>), grid, dim3(256), 0, s, in,
                                   static_cast<float *>(out), chans, aoff, taps, hist_in, hist_out, decim, ntaps, scale, row, c0, (long long)nb_call, gate,
                                   nchan, pack_off, nchan);
        } else if (gate) {
            if (format == kAudioS16)
                hipLaunchKernelGGL((k_chan_audio<short, true, const unsigned char *, int>), grid, dim3(256), 0, s, in, static_cast<short *>(out), chans, aoff,
                                   taps, hist_in, hist_out, decim, ntaps, scale, row, c0, (long long)nb_call, gate, nchan);
            else
                hipLaunchKernelGGL((k_chan_audio<float, true, const unsigned char *, int>), grid, dim3(256), 0, s, in, static_cast<float *>(out), chans, aoff,
                                   taps, hist_in, hist_out, decim, ntaps, scale, row, c0, (long long)nb_call, gate, nchan);
        } else if (format == kAudioS16)
            hipLaunchKernelGGL((k_chan_audio<short, false>), grid, dim3(256), 0, s, in, static_cast<short *>(out), chans, aoff, taps, hist_in, hist_out, decim,
                               ntaps, scale, row, c0, (long long)nb_call);
        else
            hipLaunchKernelGGL((k_chan_audio<float, false>), grid, dim3(256), 0, s, in, static_cast<float *>(out), chans, aoff, taps, hist_in, hist_out, decim,
                               ntaps, scale, row, c0, (long long)nb_call);
    });
}

}  // namespace fdc
