// Complex integer input (fdc_pipeline_work_iq and friends): interleaved int16 (sc16) or int8 (sc8) I/Q, sample k = (I_k * scale, Q_k * scale).
// The int -> float conversion is exact; the product is rounded once in f32 and kept out of FMA contraction with whatever consumes it (the first
// butterfly of a transform), so a kernel that converts in its own loads gives the bytes of the complex path on the numpy-converted input.
#pragma once
#include <hip/hip_runtime.h>
#include "fdc_radix16.hpp"
#include "fdc_forms.hpp"

namespace fdc {

enum IqFormat { kIqFloat = 0, kIqSc16 = 1, kIqSc8 = 2 };   // kIqSc16 / kIqSc8 = FDC_IQ_SC16 / FDC_IQ_SC8 (include/fdc_amd.h)

struct __attribute__((aligned(4))) sc16 { short i, q; };
struct __attribute__((aligned(2))) sc8 { signed char i, q; };

inline size_t iq_bytes(int fmt) { return fmt == kIqSc16 ? 4 : fmt == kIqSc8 ? 2 : 8; }
constexpr size_t kIqRingBytes = 4;      // bytes per sample of the widest integer format (sc16): what a handle's integer ring is sized for

__device__ __forceinline__ float iq_mul(float a, float s)
{
#pragma clang fp contract(off)
    return a * s;      // (__fmul_rn is a plain, contractable product in this HIP)
}
__device__ __forceinline__ cf iq_widen(sc16 v, float s) { return mk(iq_mul((float)v.i, s), iq_mul((float)v.q, s)); }
__device__ __forceinline__ cf iq_widen(sc8 v, float s) { return mk(iq_mul((float)v.i, s), iq_mul((float)v.q, s)); }
__device__ __forceinline__ cf iq_widen(float2 v, float) { return mk(v.x, v.y); }

// The last argument of the kernels with integer forms (k_blk256, k_f4096): the float2 forms' epilogue output pointer, which the integer forms never
// use; they take the scale in its place, so the argument block of every float2 form stays what it was.  TO: the output sample (float2, or sc16 /
// sc8 for integer output, fdc_pipeline_set_output_format): one integer side, its scale (a float); both sides, (input scale, output scale)
template <class TI, class TO = float2> struct IqTail { typedef float2 type; };
template <class TI> struct IqTail<TI, float2> { typedef float type; };
template <class TO> struct IqTail<float2, TO> { typedef float type; };
template <> struct IqTail<float2, float2> { typedef float *__restrict__ type; };
__device__ __forceinline__ float iq_tail_scale(float s) { return s; }
__device__ __forceinline__ float iq_tail_scale(float2 s) { return s.x; }
__device__ __forceinline__ float iq_tail_scale(const float *) { return 1.0f; }
__device__ __forceinline__ float oq_tail_scale(float s) { return s; }
__device__ __forceinline__ float oq_tail_scale(float2 s) { return s.y; }
__device__ __forceinline__ float oq_tail_scale(const float *) { return 1.0f; }
// host: that argument of one launch — ptr (may be null) for the float2 forms, the scale(s) of the integer side(s) otherwise
template <class TI, class TO>
inline typename IqTail<TI, TO>::type iq_tail(float *ptr, float iscale, float oscale)
{
    constexpr bool kIq = !std::is_same<TI, float2>::value, kOq = !std::is_same<TO, float2>::value;
    if constexpr (kIq && kOq) return make_float2(iscale, oscale);
    else if constexpr (kIq) return iscale;
    else if constexpr (kOq) return oscale;
    else return ptr;
}

// host: which sample type a launch takes (fdc_forms.hpp): f(float2{}), f(sc16{}) or f(sc8{}) for the type of format fmt, or for every one (fmt = kEvery);
// for_int_samples: the kernels without a float2 form
template <int FMT> struct IqSample { typedef float2 type; };
template <> struct IqSample<kIqSc16> { typedef sc16 type; };
template <> struct IqSample<kIqSc8> { typedef sc8 type; };
template <int... FMTS, class F>
inline void for_sample_formats(int fmt, F &&f)
{
    for_values<FMTS...>(fmt, [&](auto V) { f(typename IqSample<decltype(V)::value>::type{}); });
}
template <class F> inline void for_samples(int fmt, F &&f) { for_sample_formats<kIqFloat, kIqSc16, kIqSc8>(fmt, f); }
template <class F> inline void for_int_samples(int fmt, F &&f) { for_sample_formats<kIqSc16, kIqSc8>(fmt, f); }

// one sample's raw bits (a dword / a 16-bit load), widened later by iq_widen_bits
__device__ __forceinline__ unsigned iq_bits(const sc16 *p) { return *reinterpret_cast<const unsigned *>(p); }
__device__ __forceinline__ unsigned iq_bits(const sc8 *p) { return *reinterpret_cast<const unsigned short *>(p); }

// raw sample bits in a buffer-load register: sc16 one dword, sc8 the low half of one (a 2-byte load)
__device__ __forceinline__ cf iq_widen_bits(sc16, unsigned u, float s)
{
    return mk(iq_mul((float)(int)(short)(u & 0xFFFFu), s), iq_mul((float)(int)(short)(u >> 16), s));
}
__device__ __forceinline__ cf iq_widen_bits(sc8, unsigned u, float s)
{
    return mk(iq_mul((float)(int)(signed char)(u & 0xFFu), s), iq_mul((float)(int)(signed char)((u >> 8) & 0xFFu), s));
}

// Complex integer OUTPUT (fdc_pipeline_set_output_format): each component q = saturate(round_half_even(y * scale)), the product rounded once in f32 and
// kept out of FMA contraction with whatever produced y (as iq_mul); NaN -> 0, +-Inf -> the limits.  The one rule of every kernel that narrows
// (k_blk256 and k_f4096 in their stores, k_complex_to_iq, k_scatter_oq).
// v_cvt_i32_f32 itself maps NaN to 0 and saturates out-of-range values and +-Inf to the int32 limits (a C++ cast leaves those undefined), so the
// clamp is one integer med3 — the form that keeps k_f4096's sc16 stores inside its 128 registers
__device__ __forceinline__ int oq_round(float a, float s, int lo, int hi)
{
    const float t = __builtin_rintf(iq_mul(a, s));                 // v_rndne_f32
    int i;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(i) : "v"(t));
    return i < lo ? lo : i > hi ? hi : i;
}
// the packed bits of one output sample: sc16 one dword (I low), sc8 one 16-bit word (I low)
__device__ __forceinline__ unsigned oq_bits(sc16, cf v, float s)
{
    return (unsigned)(unsigned short)oq_round(v.x, s, -32768, 32767) | ((unsigned)(unsigned short)oq_round(v.y, s, -32768, 32767) << 16);
}
__device__ __forceinline__ unsigned oq_bits(sc8, cf v, float s)
{
    return (unsigned)(unsigned char)oq_round(v.x, s, -128, 127) | ((unsigned)(unsigned char)oq_round(v.y, s, -128, 127) << 8);
}
__device__ __forceinline__ sc16 oq_narrow(sc16, cf v, float s) { const unsigned u = oq_bits(sc16{}, v, s); return sc16{(short)(u & 0xFFFFu), (short)(u >> 16)}; }
__device__ __forceinline__ sc8 oq_narrow(sc8, cf v, float s) { const unsigned u = oq_bits(sc8{}, v, s); return sc8{(signed char)(u & 0xFFu), (signed char)(u >> 8)}; }

}  // namespace fdc
