// gfx950 (MI355X, CDNA4) kernel of the frequency-domain channelizer — the channel tones (fdc_pipeline_set_tones): behind the channel demodulation, over
// the whole call's demodulated samples, a bank of T narrow correlators per channel, integrated over frames of W blocks.  tests/tones_model.py is
// the definition; this file computes it in the same order, so the frame rows are that model's byte for byte however the stream is cut.
//
// THE DEFINITION.  d: channel c's demodulated stream, G = lout_c / S groups per block.  The group sum u(g) of the stream's group g is the sum of its S
// samples, ascending from +0, every sum rounded on its own.  The reference of tone t at group g is table[(inc[c][t] g mod 2^32) >> 22], 1024 (cos, sin)
// pairs; the accumulator of (c, t) takes re = re + u cs, im = im - u sn per group, g ascending, every product and sum rounded on its own (tone_mac),
// runs on over the W blocks of a frame, is stored as the frame's row and starts the next frame at (+0, +0).
//
// THE KERNEL.  A channel's demodulated run is contiguous across the blocks of a call (k_chan_demod), and S divides lout_c, so a frame of the call is a
// contiguous range of the call's groups.  One wave (a workgroup of 64) per (frame of the call, channel): grid y = channel, grid x strides over the
// ceil((fill + nb) / W) frames the call touches, the continued first one and an unfinished last one included.  The wave walks its frame 64 groups at a
// time.  First the lanes are GROUPS: lane q sums group q's S samples, 16 bytes per load where S is a multiple of 4 and the run is 16-byte aligned, one
// sample per load otherwise (the same sums in the same order, so the same bits).  Then the lanes are TONES: the wave goes through the 64 sums in g order,
// each read from its lane (a wave-uniform lane index: the move stands outside every per-lane condition, the rule lag1_rows documents), the reference
// from the table in LDS, the phase advanced by inc per group, which is exact mod 2^32.  The wave of a continued first frame starts from carry_in, the
// wave of an unfinished last frame writes carry_out in the place of a row, and the wave of a call's last frame writes all T entries of its channel's
// carry_out in every call (zeros where no frame is open), so its bytes are defined.  No atomics, no wave waits on another workgroup; the only barrier
// stands behind the table's copy to LDS, in front of every condition.
#include "fdc_kernels.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace fdc {

// the reference table: (cos, sin)(2 pi k / 1024) designed in double, rounded once; the four axis entries exact
void tone_table(float2 *dst)
{
    for (int k = 0; k < kToneTable; k++) {
        const double a = 2.0 * M_PI * (double)k / (double)kToneTable;
        dst[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    dst[0] = make_float2(1.0f, 0.0f); dst[kToneTable / 4] = make_float2(0.0f, 1.0f);
    dst[kToneTable / 2] = make_float2(-1.0f, 0.0f); dst[3 * kToneTable / 4] = make_float2(0.0f, -1.0f);
}

// THE ORDER IS THE DEFINITION: every sum and every product rounded on its own, no contraction
__device__ __forceinline__ float tone_sum(float u, float d)
{
#pragma clang fp contract(off)
    return u + d;
}

__device__ __forceinline__ void tone_mac(float &re, float &im, float u, float2 w)
{
#pragma clang fp contract(off)
    const float a = u * w.x, b = u * w.y;
    re = re + a;
    im = im - b;
}

// the sum of one group: S consecutive samples from d on, ascending from +0
template <bool WIDE>
__device__ __forceinline__ float tone_group(const float *d, unsigned S)
{
    float u = 0.0f;
    if constexpr (WIDE) {
#pragma unroll 4
        for (unsigned i = 0; i < S; i += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(d + i);
            u = tone_sum(tone_sum(tone_sum(tone_sum(u, v.x), v.y), v.z), v.w);
        }
    } else {
#pragma unroll 4
        for (unsigned i = 0; i < S; i++) u = tone_sum(u, d[i]);
    }
    return u;
}

// in: the call's demodulated samples ([channel][nb_call * lout] float at nb_call * out_off); frames: where the call's first completed frame row goes
// ([frame][nchan][T] float2); carry_in (null: zeros) / carry_out: [nchan][T] float2, two different buffers; fill: the blocks of the stream already inside
// the open frame (0 .. W - 1; carry_in is read only where fill > 0)
__global__ __launch_bounds__(64) void k_chan_tones(const float *__restrict__ in, const ChanDev *__restrict__ chans, const unsigned *__restrict__ inc,
                                                   const float2 *__restrict__ tab, const float2 *__restrict__ carry_in, float2 *__restrict__ carry_out,
                                                   float2 *__restrict__ frames, int c0, int nchan, int T, unsigned S, int W, int fill, long long first_block,
                                                   int nb_call)
{
    __shared__ float2 lut[kToneTable];
    const unsigned lane = threadIdx.x;
    for (unsigned i = lane; i < kToneTable / 2; i += 64) reinterpret_cast<float4 *>(lut)[i] = reinterpret_cast<const float4 *>(tab)[i];
    __syncthreads();
    const int c = c0 + (int)blockIdx.y;
    const unsigned G = (unsigned)chans[c].lout / S;
    const float *d = in + (size_t)nb_call * (size_t)chans[c].out_off;
    const bool wide = (S & 3) == 0 && (reinterpret_cast<uintptr_t>(d) & 15) == 0;
    const int nfr = (fill + nb_call + W - 1) / W, nf = (fill + nb_call) / W;      // frames the call touches / completes
    const bool tone = (int)lane < T;
    const unsigned my_inc = tone ? inc[(size_t)c * (size_t)T + lane] : 0u;
    const size_t ct = (size_t)c * (size_t)T + lane;
    for (int f = (int)blockIdx.x; f < nfr; f += (int)gridDim.x) {
        // the frame's blocks of the call, and its groups
        const long long lo = (long long)f * W - fill, hi = lo + W;
        const long long b0 = lo > 0 ? lo : 0, b1 = hi < nb_call ? hi : (long long)nb_call;
        const unsigned long long g0 = (unsigned long long)b0 * G, g1 = (unsigned long long)b1 * G;
        float re = 0.0f, im = 0.0f;
        if (f == 0 && fill > 0 && carry_in && tone) { const float2 z = carry_in[ct]; re = z.x; im = z.y; }
        // the phase of the frame's first group: inc g mod 2^32, g the STREAM's group index
        unsigned ph = my_inc * (unsigned)((unsigned long long)first_block * G + g0);
        for (unsigned long long gg = g0; gg < g1; gg += 64) {
            const unsigned n = g1 - gg < 64 ? (unsigned)(g1 - gg) : 64u;
            float u = 0.0f;
            if (lane < n) {
                const float *x = d + (size_t)(gg + lane) * S;
                u = wide ? tone_group<true>(x, S) : tone_group<false>(x, S);
            }
            const int ubits = __float_as_int(u);
            for (unsigned j = 0; j < n; j++) {
                const float uj = __int_as_float(__builtin_amdgcn_readlane(ubits, (int)j));
                tone_mac(re, im, uj, lut[ph >> 22]);
                ph += my_inc;
            }
        }
        if (tone) {
            const float2 z = make_float2(re, im);
            if (f < nf) frames[((size_t)f * (size_t)nchan) * (size_t)T + ct] = z;
            if (f == nfr - 1) carry_out[ct] = f < nf ? make_float2(0.0f, 0.0f) : z;
        }
    }
}

hipError_t launch_chan_tones(const float *in, const ChanDev *chans, const unsigned *inc, const float2 *tab, const float2 *carry_in, float2 *carry_out,
                             float2 *frames, int nchan, int ntones, int group, int frame_blocks, int fill, long long first_block, int nb_call, hipStream_t s)
{
    if (nchan <= 0 || nb_call <= 0) return hipSuccess;
    if (ntones < 1 || ntones > 64 || group < 1 || frame_blocks < 1 || fill < 0 || fill >= frame_blocks || !carry_out) return hipErrorInvalidValue;
    const int nfr = (int)(((long long)fill + nb_call + frame_blocks - 1) / frame_blocks);
    // grid y = channel, in pieces of 32768 channels; grid x: the frames, strided where there are more than fill the device a few times over
    for (int c0 = 0; c0 < nchan; c0 += 32768) {
        const int nc = std::min(nchan - c0, 32768);
        const int gx = std::max(1, std::min(nfr, (8192 + nc - 1) / nc));
        hipLaunchKernelGGL(k_chan_tones, dim3((unsigned)gx, (unsigned)nc), dim3(64), 0, s, in, chans, inc, tab, carry_in, carry_out, frames, c0, nchan, ntones,
                           (unsigned)group, frame_blocks, fill, first_block, nb_call);
    }
    return hipGetLastError();
}

}  // namespace fdc
