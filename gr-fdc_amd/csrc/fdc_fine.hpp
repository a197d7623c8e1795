// Fine tuning (fdc_pipeline_set_fine_tuning): sample t of channel c's stream is turned by exp(-2 pi i phi_c(t)), phi_c(t) = ((inc_c t) mod 2^64) / 2^64 —
// an INTEGER function of the stream's own sample index, so it has no drift and does not depend on how the stream is cut into calls or launch groups.
// Per sample the kernels multiply y * base * step, in this order: base = the phasor of phi_c(block * lout_c), computed here once per (block, channel),
// step = step_c[j] = exp(-2 pi i frac(inc_c j / 2^64)), j < lout_c, a table designed in double on the host and rounded once.  The products are kept out
// of FMA contraction (as oq_bits, fdc_iq.hpp), so every route (k_fine_rotate behind the channel kernels, k_f4096's own stores) gives the same bytes from the same y.
#pragma once
#include <hip/hip_runtime.h>
#include "fdc_radix16.hpp"

namespace fdc {

// one channel's (k_fine_rotate) or one schedule row's (k_f4096) part of the setting: the increment and where its lout step factors start in the step table
struct FineChan { unsigned long long inc; long long step_off; };

// exp(-2 pi i ph / 2^64).  The nearest quarter turn comes off the top bits (exact: a swap and signs); the rest, |r| <= 1/8 turn, keeps its top 30 bits —
// the conversion to float rounds them to 24, under 2^-27 turn — and goes through sincospif (no fast-math sine).
__device__ __forceinline__ cf fine_phasor(unsigned long long ph)
{
    const unsigned long long q = ph + (1ull << 61);
    const unsigned quad = (unsigned)(q >> 62);
    const int r = (int)(unsigned)((q & ((1ull << 62) - 1)) >> 32) - (1 << 29);      // r / 2^32 turns, in [-1/8, 1/8)
    float s, c;
    sincospif((float)r * (1.0f / 2147483648.0f), &s, &c);                           // half turns: 2 r / 2^32
    // exp(-i (quad pi/2 + a)) = (cos, -sin) of the sum
    return quad == 0 ? mk(c, -s) : quad == 1 ? mk(-s, -c) : quad == 2 ? mk(-c, s) : mk(s, c);
}

// base of block `block` of a channel with lout samples per block (64-bit wrapping products: the phase modulo one turn)
__device__ __forceinline__ cf fine_base(unsigned long long inc, unsigned long long block, unsigned lout)
{
    return fine_phasor(inc * (block * (unsigned long long)lout));
}

__device__ __forceinline__ cf fine_mul(cf y, cf w)
{
#pragma clang fp contract(off)
    const float a = y.x * w.x, b = y.y * w.y, c = y.x * w.y, d = y.y * w.x;
    return mk(a - b, c + d);
}

// one sample: y * base * step, in this order
__device__ __forceinline__ cf fine_rotate(cf y, cf base, cf step) { return fine_mul(fine_mul(y, base), step); }

}  // namespace fdc
