// gfx950 (MI355X, CDNA4) kernel of the frequency-domain channelizer — the audio resampler (fdc_pipeline_set_audio_resampler): the second form of the
// channel audio behind the demodulation, a polyphase FIR with interpolation L = up and decimation M = down.  tests/resample_model.py is the
// definition.  With t the ABSOLUTE sample index of a channel's demodulated stream d, h the prototype taps padded with +0 to L Kp entries:
//
//     a[n] = sum over k = 0 .. Kp - 1 of h[k L + (n M mod L)] d[floor(n M / L) - k]
//
// THE ORDER IS THE DEFINITION: k ascending from acc = +0, every product and every sum rounded on its own (k_chan_audio's audio_mac; the padded zero
// taps are part of the sum).  Output n belongs to the block its newest sample floor(n M / L) lies in.
//
// THE CALL.  A call starts at block first_block; e0 = (-first_block lout L) mod M is where its first output stands on the upsampled grid, counted from
// the call's first sample.  Output i of the call (i = 0, 1, ...) stands at e0 + i M: its newest sample is t_i = (e0 + i M) div L of the call's run
// and its tap phase (e0 + i M) mod L.  Only first_block mod M enters, which the host passes, so nothing here grows with the absolute index.
//
// PHASE CLASSES.  Outputs i and i + L have the same phase and their samples lie M apart.  The outputs are cut into rounds of L; class r of a round
// (r = i mod L) has phase (e0 + r M) mod L and sample offset off_r = (e0 + r M) div L < M, whichever round it is.  Lane q of a class reads sample
// tb + off_r + q M - k for tap k: k_chan_audio's decimate-by-M access, so the staging is k_chan_audio's with D = M and K = Kp: a TILE of R rounds
// is the M R samples from tb = M R tile on and the Kp - 1 in front of them, staged in LDS DE-INTERLEAVED BY t mod M (tile sample i at plane i mod M,
// index i / M), consecutive lanes on consecutive words of one plane, the plane pitch ceil(64 / M) modulo 64.  The tap of a step is the same for
// the whole wave: a scalar load from the table stored phase-major, [phase][k].  A wave takes (class, trip of 256 rounds) items, the items of a tile
// dealt round the four waves; a lane holds four rounds of the class, 64 apart.
//
// THE STORES are strided: the lanes of a class hold outputs L elements apart, and each stores its own element of the block-major matrix; the
// other classes, on the other waves of the same workgroup, fill the elements between them, and the L2 merges them (DESIGN.md section 7 has the
// measurement).  Cell (block, channel) has W = ceil(lout L / M) columns and owns W or W - 1 outputs: a pad element of zero bits follows the
// W - 1; the pads are written by a loop of their own over the call's rows, in 64-bit integers.  Every offset into the matrix is 64-bit.
//
// The staging loops' trip counts depend on the workgroup alone, the computing loop's on the wave alone; the barriers stand outside both and outside
// every per-lane condition.  No load leaves (history, the call's run of the channel); a lane without an output computes its class's last valid one
// and stores nothing.  The workgroup of the run's first tile also writes the new history, to ANOTHER buffer than the one read.
//
// THE GATED FORM (GATE; the channel squelch on): an output of a closed (block, channel) is stored as zero bits, the footprint is the ungated
// pass's, and the history runs on over the ungated samples.  A tile none of whose rows is open stages nothing and runs no tap loop, a trip whose
// rows are all closed runs no tap loop (the same for the whole workgroup / wave: every wave looks at the same rows and joins its lanes by a ballot).
#include "fdc_kernels.h"
#include <algorithm>
#include "fdc_iq.hpp"

namespace fdc {

constexpr unsigned kRsLdsWords = 10240;           // 40 KiB: four workgroups per compute unit

struct RsTile { unsigned pitch, front, rounds; };  // plane pitch in words; ceil((Kp - 1) / M), the planes' words in front of round 0; rounds per tile

__host__ __device__ inline RsTile rs_tile(unsigned M, unsigned Kp)
{
    RsTile t;
    const unsigned w = ((64 + M - 1) / M) & 63;
    t.pitch = kRsLdsWords / M;                      // >= 80 (M <= 128)
    t.pitch -= (t.pitch - w) & 63;                  // pitch = w modulo 64; M * pitch <= kRsLdsWords; pitch >= 65
    t.front = (Kp - 1 + M - 1) / M;                 // <= 255 at M = 1, where pitch is 10240; <= 2 where pitch is 65
    t.rounds = t.pitch - t.front;                   // the tile's last sample, rounds M + Kp - 2, has index rounds + front - 1 < pitch
    if (t.rounds >= 256) t.rounds &= ~255u;         // whole trips of a wave's 256 rounds where the tile holds that many
    return t;
}

__device__ __forceinline__ float rs_mac(float acc, float h, float z)
{
#pragma clang fp contract(off)
    const float p = h * z;
    return acc + p;
}

__device__ __forceinline__ void rs_store(float *out, long long at, float a, float) { out[at] = a; }
__device__ __forceinline__ void rs_store(short *out, long long at, float a, float scale) { out[at] = (short)oq_round(a, scale, -32768, 32767); }

// sample t of (history, run): t in [-(Kp - 1), T)
__device__ __forceinline__ float rs_sample(const float *d, const float *hin, int Kp, long long t)
{
    return t >= 0 ? d[t] : hin ? hin[Kp - 1 + t] : 0.0f;
}

// whether any of the rows [r0, r1] of one channel's mask column is open: the same answer in every lane of the wave
__device__ __forceinline__ bool rs_any_open(const unsigned char *col, unsigned pitch, unsigned r0, unsigned r1)
{
    bool open = false;
    for (unsigned r = r0; r <= r1; r += 64) {               // (the trip count is the wave's)
        const unsigned rr = r + (threadIdx.x & 63);
        open = open || (rr <= r1 && col[(size_t)rr * pitch] != 0);
    }
    return __builtin_amdgcn_ballot_w64(open) != 0;
}

// x / d for a divisor that does not change (Granlund and Montgomery's multiply-high form, exact for every 32-bit x and d >= 1): with l = ceil(log2 d)
// and m = floor(2^32 (2^l - d) / d) + 1, t = umulhi(m, x) and x / d = (t + ((x - t) >> min(l, 1))) >> max(l - 1, 0).  The pass divides every output's
// sample offset by lout and its position by M; as divisions they were most of its vector instructions at 16 taps per phase
struct UDiv { unsigned m, s1, s2; };
__device__ __forceinline__ UDiv udiv_make(unsigned d)
{
    const unsigned l = d <= 1 ? 0u : 32u - (unsigned)__clz((int)(d - 1));
    UDiv u;
    u.m = (unsigned)((((1ull << l) - d) << 32) / d) + 1u;
    u.s1 = l < 1 ? l : 1u;
    u.s2 = l > 1 ? l - 1 : 0u;
    return u;
}
__device__ __forceinline__ unsigned udiv(unsigned x, UDiv u)
{
    const unsigned t = __umulhi(u.m, x);
    return (t + ((x - t) >> u.s1)) >> u.s2;
}

// how many outputs of the call stand in front of position x of the upsampled grid (they stand at e0, e0 + M, ...)
__device__ __forceinline__ long long rs_below(long long x, unsigned e0, unsigned M)
{
    return x > (long long)e0 ? (x - (long long)e0 + (long long)M - 1) / (long long)M : 0;
}

// in: the call's demodulated samples ([channel][nb_call * lout] float at nb_call * out_off); out: row 0 of the call's audio ([nb_call][A] TO);
// tp: the taps phase-major, [L][Kp]; hist_in (null: zeros) and hist_out (null where Kp = 1): [nchan][Kp - 1] float; fbm: first_block mod M;
// mask (GATE only): row 0 of the call's mask ([nb_call][nchan] bytes)
template <class TO, bool GATE>
__global__ __launch_bounds__(256) void k_chan_resample(const float *__restrict__ in, TO *__restrict__ out, const ChanDev *__restrict__ chans,
                                                       const long long *__restrict__ aoff, const float *__restrict__ tp,
                                                       const float *__restrict__ hist_in, float *__restrict__ hist_out, int L, int M, int Kp, float scale,
                                                       long long A, int c0, long long nb_call, unsigned fbm, const unsigned char *__restrict__ mask,
                                                       int nchan)
{
    __shared__ float tile[kRsLdsWords];
    const int c = c0 + (int)blockIdx.y;
    const unsigned char *gcol = nullptr;                            // GATE: the channel's column of the mask and the pitch of its rows
    unsigned gpitch = 0;
    if constexpr (GATE) { gcol = mask + c; gpitch = (unsigned)nchan; }
    const unsigned lout = (unsigned)chans[c].lout, tid = threadIdx.x;
    const unsigned uL = (unsigned)L, uM = (unsigned)M;
    const long long T = nb_call * (long long)lout;
    const float *d = in + nb_call * chans[c].out_off;
    const float *hin = hist_in ? hist_in + (size_t)c * (size_t)(Kp - 1) : nullptr;
    TO *o = out + aoff[c];
    const unsigned span = (unsigned)(((unsigned long long)lout * uL) % uM);         // lout L mod M
    const unsigned e0 = (uM - (fbm * span) % uM) % uM;                              // (-first_block lout L) mod M
    const unsigned W = (unsigned)(((unsigned long long)lout * uL + uM - 1) / uM);   // the columns of a cell
    const RsTile g = rs_tile(uM, (unsigned)Kp);
    const unsigned magic = (unsigned)(0x100000000ull / uM) + 1u;                    // i / M = umulhi(i, magic) for i < 2^16, M >= 2
    const UDiv by_lout = udiv_make(lout), by_M = udiv_make(uM), by_L = udiv_make(uL);
    // where tile sample i lies in LDS: plane i mod M, index i / M
    const auto lds_at = [&](unsigned i) {
        const unsigned q = uM == 1 ? i : __umulhi(i, magic);
        return (i - q * uM) * g.pitch + q;
    };
    // the pads: a cell that owns W - 1 outputs has a zero behind them (no barrier inside: the trip count may be the lane's)
    for (long long m = (long long)blockIdx.x * 256 + tid; m < nb_call; m += (long long)gridDim.x * 256) {
        const long long x = m * (long long)lout * (long long)uL;
        const long long cnt = rs_below(x + (long long)lout * (long long)uL, e0, uM) - rs_below(x, e0, uM);
        if (cnt < (long long)W) o[m * A + (long long)(W - 1)] = TO(0);
    }
    const unsigned tspan = uM * g.rounds;                                           // samples of a tile
    const unsigned trips = (g.rounds + 255) / 256, items = uL * trips;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (long long tb = (long long)blockIdx.x * tspan; tb < T; tb += (long long)gridDim.x * tspan) {
        const unsigned lim = T - tb < (long long)tspan ? (unsigned)(T - tb) : tspan;    // samples of this tile: outputs whose newest sample is among them
        const long long t0 = tb - (Kp - 1);
        const unsigned mb = (unsigned)(tb / (long long)lout), rem = (unsigned)(tb - (long long)mb * (long long)lout);   // the tile's first row
        // GATE: a tile without an open row stages nothing (its samples count as none: no lane below has anything to load), and its waves run no tap
        // loop and store zeros.  The same for the whole workgroup, and both barriers stand outside the condition
        bool tile_open = true;
        if constexpr (GATE) tile_open = rs_any_open(gcol, gpitch, mb, mb + (rem + lim - 1) / lout);
        // stage, as k_chan_audio does.  The samples in front of the run (the first tile's Kp - 1) come from the history.  Those of the run are loaded
        // 16 bytes at a time between the 16-byte boundaries inside them, four such loads in flight per lane (a lane past the last quad loads that one
        // again and stores nothing); the up to three samples in front of the first boundary and behind the last are loaded one by one
        const long long ts = t0 < 0 ? 0 : t0;
        if (tile_open && t0 < 0 && tid < (unsigned)(Kp - 1)) tile[lds_at(tid)] = hin ? hin[tid] : 0.0f;                // (tile sample i is t = t0 + i)
        // element e of da is sample ts - lo + e of the run, da 16-byte aligned: the tile's are [lo, hi), and e is tile sample e + first
        const unsigned lo = (unsigned)((reinterpret_cast<uintptr_t>(d + ts) >> 2) & 3), hi = lo + (tile_open ? (unsigned)(tb + (long long)lim - ts) : 0u);
        const unsigned first = (unsigned)(ts - t0) - lo;
        const unsigned up4 = (lo + 3) & ~3u, down4 = hi & ~3u;
        const unsigned lo4 = up4 < hi ? up4 : hi, hi4 = down4 > lo4 ? down4 : lo4;      // the quads are [lo4, hi4): lo <= lo4 <= hi4 <= hi
        const float *da = d + ts - lo;
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
        // compute.  Item `it` is trip it mod trips of class it div trips; a wave takes the items wave, wave + 4, ...: the trip count depends on the wave alone
        for (unsigned it = wave; it < items; it += 4) {
            const unsigned r = trips == 1 ? it : it / trips, j0 = (it - r * trips) * 256;
            const unsigned er = e0 + r * uM, off = udiv(er, by_L), ph = er - off * uL;  // the class's sample offset (< M) and tap phase
            const unsigned nq = lim > off ? udiv(lim - off + uM - 1, by_M) : 0;         // the class's rounds with an output in this tile (<= rounds)
            if (j0 >= nq) continue;                                                     // (the same for the whole wave; no barrier below)
            unsigned j[4]; float acc[4];
#pragma unroll
            for (unsigned u = 0; u < 4; u++) {
                const unsigned jj = j0 + u * 64 + (tid & 63);
                j[u] = jj < nq ? jj : nq - 1;                                   // (a lane without an output computes the class's last and leaves it out)
                acc[u] = 0.0f;
            }
            // GATE: a trip that lies wholly in closed rows runs no tap loop (the same for the whole wave)
            bool taps_run = true;
            if constexpr (GATE)
                taps_run = tile_open && rs_any_open(gcol, gpitch, mb + udiv(rem + off + j0 * uM, by_lout),
                                                    mb + udiv(rem + off + ((j0 + 256 < nq ? j0 + 256 : nq) - 1) * uM, by_lout));
            // tap k reads tile sample (Kp - 1) + off + j M - k: the plane and the index in front go down with k
            const unsigned base = (unsigned)(Kp - 1) + off;
            const unsigned bq = udiv(base, by_M);
            unsigned rr = base - bq * uM, at = rr * g.pitch + bq;
            const float *th = tp + (size_t)ph * (size_t)Kp;
#pragma unroll 4
            for (int k = 0; k < (taps_run ? Kp : 0); k++) {
                const float h = th[k];
#pragma unroll
                for (unsigned u = 0; u < 4; u++) acc[u] = rs_mac(acc[u], h, tile[at + j[u]]);
                if (rr) { rr--; at -= g.pitch; } else { rr = uM - 1; at += rr * g.pitch - 1; }
            }
#pragma unroll
            for (unsigned u = 0; u < 4; u++) {
                const unsigned jj = j0 + u * 64 + (tid & 63);
                if (jj < nq) {
                    // the output's newest sample is sample `in_tile` of the tile's first row on: its row, and its place among the row's outputs
                    const unsigned in_tile = rem + off + jj * uM, dm = udiv(in_tile, by_lout), in_row = in_tile - dm * lout;
                    const unsigned col = udiv(uL * in_row + ph, by_M);
                    const long long m = (long long)(mb + dm), at_out = m * A + (long long)col;
                    if (GATE && !gcol[(size_t)m * gpitch]) o[at_out] = TO(0);
                    else rs_store(o, at_out, acc[u], scale);
                }
            }
        }
        __syncthreads();                                                        // the tile is read: the next trip may overwrite it
    }
    if (blockIdx.x == 0 && tid < (unsigned)(Kp - 1))
        hist_out[(size_t)c * (size_t)(Kp - 1) + tid] = rs_sample(d, hin, Kp, T - (Kp - 1) + (long long)tid);
}

hipError_t launch_chan_resample(int format, int up, int down, int kp, float scale, const float *taps_pm, const long long *aoff, long long row,
                                const float *in, void *out, const ChanDev *chans, const float *hist_in, float *hist_out, int nchan, int nb_call,
                                long long sum_lout, long long first_block, hipStream_t s, const unsigned char *gate)
{
    if (nchan <= 0 || nb_call <= 0) return hipSuccess;
    if (format != kAudioF32 && format != kAudioS16) return hipErrorInvalidValue;
    if (up < 1 || up > 64 || down < 1 || down > 128 || kp < 1 || kp > 256 || first_block < 0 || !taps_pm || !aoff || !in || !out) return hipErrorInvalidValue;
    if (kp > 1 && (!hist_out || hist_in == hist_out)) return hipErrorInvalidValue;
    const RsTile g = rs_tile((unsigned)down, (unsigned)kp);
    const unsigned fbm = (unsigned)(first_block % down);
    // the grid: a workgroup per tile of a run of mean length, about eight workgroups per unit; grid y = channel, in pieces of 32768 channels
    const long long tiles = ((long long)nb_call * sum_lout / nchan) / ((long long)down * g.rounds) + 1;
    for (int c0 = 0; c0 < nchan; c0 += 32768) {
        const int nc = nchan - c0 < 32768 ? nchan - c0 : 32768;
        const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(tiles, (2048 + nc - 1) / nc)), (unsigned)nc);
        if (gate) {
            if (format == kAudioS16)
                hipLaunchKernelGGL((k_chan_resample<short, true>), grid, dim3(256), 0, s, in, static_cast<short *>(out), chans, aoff, taps_pm, hist_in, hist_out,
                                   up, down, kp, scale, row, c0, (long long)nb_call, fbm, gate, nchan);
            else
                hipLaunchKernelGGL((k_chan_resample<float, true>), grid, dim3(256), 0, s, in, static_cast<float *>(out), chans, aoff, taps_pm, hist_in, hist_out,
                                   up, down, kp, scale, row, c0, (long long)nb_call, fbm, gate, nchan);
        } else if (format == kAudioS16)
            hipLaunchKernelGGL((k_chan_resample<short, false>), grid, dim3(256), 0, s, in, static_cast<short *>(out), chans, aoff, taps_pm, hist_in, hist_out, up,
                               down, kp, scale, row, c0, (long long)nb_call, fbm, gate, nchan);
        else
            hipLaunchKernelGGL((k_chan_resample<float, false>), grid, dim3(256), 0, s, in, static_cast<float *>(out), chans, aoff, taps_pm, hist_in, hist_out, up,
                               down, kp, scale, row, c0, (long long)nb_call, fbm, gate, nchan);
    }
    return hipGetLastError();
}

}  // namespace fdc
