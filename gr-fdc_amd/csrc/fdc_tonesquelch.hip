// gfx950 (MI355X, CDNA4) kernels of the frequency-domain channelizer — the tone squelch (fdc_pipeline_set_tone_squelch): thresholds on the frame rows
// the channel tones complete (fdc_tones.hip) decide, per channel and frame, whether the selected tone is there; the decision of the frame before gates
// the carrier squelch's mask, which gates the audio and feeds the pack offsets.  tests/tone_squelch_model.py is the definition; behind the e_t both
// kernels are integer or compare-only, so any scan order gives that model's bytes however the stream is cut.
//
// THE DEFINITION.  Per channel a tone index sel (-1: not tone-gated), thresholds open >= close >= 0 and a ratio >= 0; for all channels a guard and a hang
// count in frames.  Of the row Z[f][c][0 .. T - 1]: e_t = re re + im im, every product and the sum rounded on its own; e = e_sel; o = the largest e_t
// over |t - sel| > guard, from +0 by "e_t > o ? e_t : o" (a NaN is never taken); R = ratio o; strong = e >= open and e >= R; hold = e >= close and
// e >= R; low = neither.  Over the frames the carrier squelch's state machine (fdc_postpass.hip, k_chan_squelch) with frames in place of blocks gives
// dec[f][c].  Block m of a call stands in frame j = (fill + m) div W of the call; the decision in force for it is the carried state's open for j = 0 and
// dec[j - 1][c] otherwise (frame j - 1 is completed inside the call): mask[m][c] &= in force.  A channel with sel = -1 keeps its mask, has dec = 1 and
// the state (0, 0).
//
// k_tone_decide.  One wave (a workgroup of 64) per channel; a trip covers 64 completed frames, joined by carries every lane holds.  Phase one, the lanes
// are TONES: for each frame of the trip the wave reads the frame's row of its channel (T <= 64 float2, contiguous), every lane forms its e_t, the guarded
// maximum is a butterfly of __shfl_xor, e_sel a readlane at the wave-uniform index sel, and the lane whose index is the frame's place in the trip keeps
// the class.  Phase two, the lanes are FRAMES: the three inclusive max-scans of scan_classes by __shfl_up (last strong, last not low, last end of a run
// of hang + 1 low frames), the carried open state standing as a strong frame at index -1 - (hang - h).  Every shuffle and readlane stands outside every
// per-lane condition (the rule lag1_rows documents), the trip counts depend on the wave alone.  No atomics, no LDS, no wave waits on another workgroup.
// The state is read from one buffer and written to ANOTHER: the gate reads the carried one behind this kernel.
//
// k_tone_gate.  Over the flat index of the call's nb C mask bytes, lanes on consecutive bytes (coalesced at C = 4 as at C = 256): one byte read, the
// decision in force read, one byte stored.  It writes exactly the mask's bytes.
#include "fdc_kernels.h"
#include <algorithm>
#include <cstdint>

namespace fdc {

constexpr int kTsNeg = -(1 << 30);

// THE ORDER IS THE DEFINITION: both products and the sum rounded on their own, no contraction
__device__ __forceinline__ float tone_energy(float2 z)
{
#pragma clang fp contract(off)
    const float a = z.x * z.x, b = z.y * z.y;
    return a + b;
}

__device__ __forceinline__ float tone_ratio_product(float ratio, float o)
{
#pragma clang fp contract(off)
    return ratio * o;
}

// inclusive max-scan over the lanes of the wave (run by the whole wave)
__device__ __forceinline__ int ts_max_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, (unsigned)d, 64);
        v = lane >= d && u > v ? u : v;
    }
    return v;
}

// frames: the call's first completed frame row ([nf][nchan][T] float2; not read where nf = 0); tone / thr_open / thr_close / ratio: [nchan];
// state_in: null = every channel (0, 0); state_out: [nchan][2] int (open, h), another buffer; dec: [nf][nchan] bytes
__global__ __launch_bounds__(64) void k_tone_decide(const float2 *__restrict__ frames, const int *__restrict__ tone, const float *__restrict__ thr_open,
                                                    const float *__restrict__ thr_close, const float *__restrict__ ratio, const int *__restrict__ state_in,
                                                    int *__restrict__ state_out, unsigned char *__restrict__ dec, int c0, int nchan, int T, int guard, int hang,
                                                    int nf)
{
    const int lane = (int)threadIdx.x;
    const int c = c0 + (int)blockIdx.x;
    const int sel = __builtin_amdgcn_readfirstlane(tone[c]);
    const bool gated = sel >= 0;
    const int rsel = gated ? sel : 0;                          // (a lane index the readlane may take; the class of an ungated channel is not looked at)
    const float To = thr_open[c], Tc = thr_close[c], rt = ratio[c];
    // the carries in front of the trip: last strong, last not low, last run end
    int cs = kTsNeg, cn = -1, ce = kTsNeg, so = 0, sh = 0;
    if (state_in && gated) {
        so = state_in[2 * c] != 0;
        const int h = state_in[2 * c + 1];
        sh = so ? (h < 0 ? 0 : h > hang ? hang : h) : 0;
        if (so) cs = cn = -1 - (hang - sh);
    }
    if (nf <= 0) {                                             // no frame completed: the state as it was read
        if (lane == 0) { state_out[2 * c] = so; state_out[2 * c + 1] = sh; }
        return;
    }
    // lane t is other than the selected tone by more than the guard (lanes behind the last tone never are)
    const int dist = lane > rsel ? lane - rsel : rsel - lane;
    const bool other = lane < T && dist > guard;
    const float2 *row = frames + (size_t)c * (size_t)T + (size_t)(lane < T ? lane : 0);
    const size_t pitch = (size_t)nchan * (size_t)T;
    for (int f0 = 0; f0 < nf; f0 += 64) {
        const int n = nf - f0 < 64 ? nf - f0 : 64;             // (the same for the whole wave)
        bool strong = false, low = true;
        for (int k = 0; k < n; k++) {
            const float e_t = tone_energy(row[(size_t)(f0 + k) * pitch]);
            float o = other && e_t > 0.0f ? e_t : 0.0f;        // (e_t is >= +0 or NaN: "e_t > o ? e_t : o" from +0 takes neither a NaN nor a zero)
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float u = __shfl_xor(o, d, 64);
                o = u > o ? u : o;
            }
            const float e = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e_t), rsel));
            const float R = tone_ratio_product(rt, o);
            const bool above = e >= R, s = e >= To && above, hold = e >= Tc && above;
            if (lane == k) { strong = s; low = !s && !hold; }
        }
        // the lanes are frames now
        const int idx = f0 + lane;
        const bool valid = lane < n;
        const int is = ts_max_scan(valid && strong ? idx : kTsNeg, lane), in = ts_max_scan(valid && !low ? idx : kTsNeg, lane);
        const int s = is > cs ? is : cs, nl = in > cn ? in : cn;
        const int ie = ts_max_scan(valid && idx - nl >= hang + 1 ? idx : kTsNeg, lane);
        const int e = ie > ce ? ie : ce;
        const int open = gated ? (s > e ? 1 : 0) : 1;
        if (valid) {
            dec[(size_t)idx * (size_t)nchan + (size_t)c] = (unsigned char)open;
            if (idx == nf - 1) {
                state_out[2 * c] = gated ? open : 0;
                state_out[2 * c + 1] = gated && open ? hang - (idx - nl) : 0;
            }
        }
        cs = __shfl(s, 63, 64); cn = __shfl(nl, 63, 64); ce = __shfl(e, 63, 64);
    }
}

// mask: row 0 of the call's carrier mask ([nb][nchan] bytes), combined in place; dec: the call's decisions ([nf][nchan]); state_in: the state carried
// INTO the call (null: (0, 0)), which k_tone_decide has left as it was
__global__ __launch_bounds__(256) void k_tone_gate(unsigned char *__restrict__ mask, const unsigned char *__restrict__ dec, const int *__restrict__ tone,
                                                   const int *__restrict__ state_in, int nchan, int W, int fill, unsigned long long total)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= total) return;
    const unsigned long long m = i / (unsigned)nchan;
    const int c = (int)(i - m * (unsigned)nchan);
    const unsigned long long j = ((unsigned long long)fill + m) / (unsigned)W;
    unsigned in_force = 1;
    if (tone[c] >= 0) in_force = j == 0 ? (state_in ? state_in[2 * c] != 0 : 0) : dec[(size_t)(j - 1) * (size_t)nchan + (size_t)c] != 0;
    mask[i] = (unsigned char)(mask[i] & in_force);
}

hipError_t launch_tone_squelch(const float2 *frames, const int *tone, const float *thr_open, const float *thr_close, const float *ratio, int guard, int hang,
                               const int *state_in, int *state_out, unsigned char *dec, unsigned char *mask, int nchan, int ntones, int frame_blocks,
                               int fill, int nb_call, hipStream_t s)
{
    if (nchan <= 0 || nb_call <= 0) return hipSuccess;
    if (ntones < 1 || ntones > 64 || frame_blocks < 1 || fill < 0 || fill >= frame_blocks || guard < 0 || hang < 0 || hang > 65535) return hipErrorInvalidValue;
    const int nf = (int)(((long long)fill + nb_call) / frame_blocks);
    if (!tone || !thr_open || !thr_close || !ratio || !state_out || state_in == state_out || (nf > 0 && (!frames || !dec))) return hipErrorInvalidValue;
    // one wave per channel, in pieces of 32768 channels
    for (int c0 = 0; c0 < nchan; c0 += 32768)
        hipLaunchKernelGGL(k_tone_decide, dim3((unsigned)std::min(nchan - c0, 32768)), dim3(64), 0, s, frames, tone, thr_open, thr_close, ratio, state_in,
                           state_out, dec, c0, nchan, ntones, guard, hang, nf);
    if (mask) {
        const unsigned long long total = (unsigned long long)nb_call * (unsigned long long)nchan;
        hipLaunchKernelGGL(k_tone_gate, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, mask, dec, tone, state_in, nchan, frame_blocks, fill, total);
    }
    return hipGetLastError();
}

}  // namespace fdc
