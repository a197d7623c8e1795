// The core the four one-block-per-CU kernels share (fdc_block256.hip, fdc_block512.hip, fdc_block1024.hip, fdc_blocknarrow.hip): the G register
// packing, the quad exchanges, the DFT over the pass index, the per-wave exchange strip with the 256-point transforms that go through it, the XCD
// block order, and the host-side choice of a kernel variant.  Everything here is forced inline: a kernel that uses a piece compiles to the
// instructions it had with the piece written out (tools/compare_block_isa.py checks that against another commit).
#pragma once
#include <hip/hip_ext.h>
#include <type_traits>
#include "fdc_kernels.h"
#include "fdc_radix16.hpp"
#include "fdc_devutil.hpp"
#include "fdc_forms.hpp"

namespace fdc {

// G: one complex value = one 64-bit vector element (two floats packed into an integer; fdc_block256.hip says why)
__device__ __forceinline__ unsigned long long pack_cf(cf v) { return ((unsigned long long)__float_as_uint(v.y) << 32) | __float_as_uint(v.x); }
__device__ __forceinline__ cf unpack_cf(unsigned long long u) { return mk(__uint_as_float((unsigned)u), __uint_as_float((unsigned)(u >> 32))); }
// The SI load/store optimizer would pair the exchange reads into ds_read2_b64, which moves 128 B/clk where
// ds_read_b64 moves 256 (MI355X_MICROARCH.md, LDS table): switched off for these kernels (device pass only).
#if defined(__HIP_DEVICE_COMPILE__)
#define FDC_PLAIN_DS __attribute__((target("no-load-store-opt")))
#else
#define FDC_PLAIN_DS
#endif

// the value of lane ^ 1 / lane ^ 2 of the quad: DPP quad_perm [1, 0, 3, 2] / [2, 3, 0, 1]
__device__ __forceinline__ cf quad_xor1(cf x)
{
    return mk(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x.x), 0xB1, 0xF, 0xF, true)),
              __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x.y), 0xB1, 0xF, 0xF, true)));
}
__device__ __forceinline__ cf quad_xor2(cf x)
{
    return mk(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x.x), 0x4E, 0xF, 0xF, true)),
              __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x.y), 0x4E, 0xF, 0xF, true)));
}

// DFT over the pass index (the register index of G): P points in place; the result X[k] is read through pass_idx<P>(k)
template <int P> __device__ __forceinline__ constexpr int pass_idx(int k) { return P == 8 ? 4 * (k & 1) + (k >> 1) : k; }
template <int P>
__device__ __forceinline__ void pass_dft(cf (&a)[P])
{
    if constexpr (P == 8) dft8<false>(a);                          // klo = k0 + 2 k1 in a[4 k0 + k1]
    else if constexpr (P == 4) dft4<false>(a[0], a[1], a[2], a[3]);   // natural order
    else { const cf s0 = a[0] + a[1], d0 = a[0] - a[1]; a[0] = s0; a[1] = d0; }
}

// Block order: round rho, XCD x = workgroup mod 8 (round-robin dispatch), slot = workgroup / 8: block = rho*grid + x*(grid/8) + slot, i.e. one
// XCD works on grid/8 consecutive blocks at a time.  Consecutive blocks overlap (by half at R = 2): the shared part is fetched from memory once
// and served to the neighbour from that XCD's L2.  Returns the workgroup's block of round 0; a round adds gridDim.x.
__device__ __forceinline__ int xcd_first_block()
{
    const int grid = gridDim.x, per = grid >> 3;
    const bool xmap = (grid & 7) == 0;
    return xmap ? (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
}

// n consecutive table entries in 16-byte reads (the twiddle row of the two transforms below; the kernels' own row reads in stage 2 and the
// cb-folding inverses of k_blk256 / k_blknar stay written out: called from there, the compiler schedules those kernels otherwise)
template <int n>
__device__ __forceinline__ void ld_row(cf (&t)[n], const float2 *row)
{
#pragma unroll
    for (int i = 0; i < n / 2; i++) {
        const float4 q = ld4(&row[2 * i]);
        t[2 * i] = mk(q.x, q.y); t[2 * i + 1] = mk(q.z, q.w);
    }
}

// The same row stored one element down (k_blk256): entry p at index p - 1, p = 1 ... 15.  Entry 0 is W^0 = 1 and never multiplied; with the row
// stored from entry 0 the compiler drops that element and pairs the rest as (1, 2), (3, 4), ..., which are only 8-byte aligned: seven ds_read2_b64
// (128 B/clk) and a lone ds_read_b64 where the shifted row takes seven ds_read_b128 (256 B/clk) and the same lone read.  WRAP: the row has a
// live entry 0 (the forward row of the offset plans), kept at index 15: eight 16-byte reads, the last one (15, 0).  t[0] is not written otherwise.
template <bool WRAP>
__device__ __forceinline__ void ld_row_sh(cf (&t)[16], const float2 *row)
{
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const float4 q = ld4(&row[2 * i]);
        t[2 * i + 1] = mk(q.x, q.y); t[2 * i + 2] = mk(q.z, q.w);
    }
    if constexpr (WRAP) {
        const float4 q = ld4(&row[14]);
        t[15] = mk(q.x, q.y); t[0] = mk(q.z, q.w);
    } else
        t[15] = ld2(&row[14]);
}

// The per-wave exchange strip of stage 1: 68*15 + 64 = 1084 points, element (p; lane) at lane + 68 p.  A lane = col + 4 b writes its sixteen
// values from scrw = strip + lane and reads the sixteen of (col, row 16 b + bb) from scrr = strip + col + 68 b.  Both 16 x 16 exchanges of
// the FFT-256 / IFFT-256 pair stay inside the wave (in-order LDS queue: a wave barrier, no s_barrier).
constexpr int kStripPts = 1084;
constexpr int kStripsEnd = 8 * kStripPts * 8;                    // 69376 bytes: the eight waves' strips
__device__ __forceinline__ void strip_get(cf (&v)[16], const float2 *scrr)
{
#pragma unroll
    for (int bb = 0; bb < 16; bb++) v[bb] = ld2(&scrr[4 * bb]);
}
// u[rev16(p)] through the strip and back
__device__ __forceinline__ void strip_trip(cf (&u)[16], float2 *scrw, const float2 *scrr)
{
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < 16; p++) st2(&scrw[68 * p], u[rev16(p)]);
    __builtin_amdgcn_wave_barrier();
    strip_get(u, scrr);
}
// The 256-point forward transform of a lane group's column: rows 16 a + b in cur[a], wr = row b of [b][p] = W_256^(b p) (rows of 18);
// the result's index b + 16 q in v[rev16(q)]
__device__ __forceinline__ void strip_fft256(cf (&cur)[16], cf (&v)[16], const float2 *wr, float2 *scrw, const float2 *scrr)
{
    dft16<false>(cur);                                            // in place, over a: index p in cur[rev16(p)]
    {
        cf tw[16];
        ld_row(tw, wr);
        st2(&scrw[0], cur[rev16(0)]);                             // W_256^0 = 1
#pragma unroll
        for (int p = 1; p < 16; p++) st2(&scrw[68 * p], cmul(cur[rev16(p)], tw[p]));
    }
    __builtin_amdgcn_wave_barrier();
    strip_get(v, scrr);
    dft16<false>(v);
}
// The 256-point inverse transform: index b + 16 q in u[q] going in, sample b + 16 q in u[rev16(q)] coming out.
__device__ __forceinline__ void strip_ifft256(cf (&u)[16], const float2 *wr, float2 *scrw, const float2 *scrr)
{
    dft16<true>(u);
    {
        cf tw[16];
        ld_row(tw, wr);
#pragma unroll
        for (int p = 1; p < 16; p++) u[rev16(p)] = cmulc(u[rev16(p)], tw[p]);
    }
    strip_trip(u, scrw, scrr);
    dft16<true>(u);
}
// ---- host: which instantiation a launch takes (fdc_forms.hpp)
// the (NT, R4, P) forms of a channelizer kernel: streamed stores (hints bit 0), R = 4, P = N / 8192 passes
template <class F>
inline void for_block_variants(int nt, int r4, int p, F &&f)
{
    for_values<8, 4, 2>(p, [&](auto P) {
        for_values<0, 1>(r4, [&](auto R4) { for_values<1, 0>(nt, [&](auto NT) { f(NT, R4, P); }); });
    });
}

}  // namespace fdc
