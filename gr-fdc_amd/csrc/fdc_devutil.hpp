// Small device helpers shared by the gfx950 fast kernels: 16-B / 8-B accesses on float2 arrays and buffer (SRD)
// addressing with an optional cache-policy word (aux: 0 = default, 16 = sc1 = device-scope write-through / L1 bypass).
#pragma once
#include <hip/hip_runtime.h>
#include "fdc_radix16.hpp"

namespace fdc {

__device__ __forceinline__ float4 ld4(const float2 *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float2 *p, cf a, cf b)
{
    *reinterpret_cast<float4 *>(p) = make_float4(a.x, a.y, b.x, b.y);
}
__device__ __forceinline__ cf ld2(const float2 *p) { return *reinterpret_cast<const cf *>(p); }

// Buffer addressing (SRD in SGPRs + 32-bit per-lane byte offset + scalar offset): no 64-bit VGPR address per access.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ cf bld2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    return mk(__uint_as_float(t.x), __uint_as_float(t.y));
}
// sc1 load: bypasses this CU's L1 and is served by the XCD's L2 (MI355X_MICROARCH.md, "__hip_atomic_load/store ... sc1")
__device__ __forceinline__ cf bld2_sc1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 16);
    return mk(__uint_as_float(t.x), __uint_as_float(t.y));
}
__device__ __forceinline__ void bst2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, cf v)
{
    u32x2 t;
    t.x = __float_as_uint(v.x); t.y = __float_as_uint(v.y);
    __builtin_amdgcn_raw_buffer_store_b64(t, r, voff, soff, 0);
}
// sc1 store: written through to the device-coherent level and dropped from this XCD's L2 (MI355X_MICROARCH.md,
// "stores of each flavour"); with every storing wave's s_waitcnt vmcnt(0) it needs no release fence before a flag.
__device__ __forceinline__ void bst2_sc1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, cf v)
{
    u32x2 t;
    t.x = __float_as_uint(v.x); t.y = __float_as_uint(v.y);
    __builtin_amdgcn_raw_buffer_store_b64(t, r, voff, soff, 16);
}
// nt = streamed once: the line is not kept against data that will be re-read (aux bit 1)
__device__ __forceinline__ cf bld2_nt(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 2);
    return mk(__uint_as_float(t.x), __uint_as_float(t.y));
}
__device__ __forceinline__ void bst2_nt(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, cf v)
{
    u32x2 t;
    t.x = __float_as_uint(v.x); t.y = __float_as_uint(v.y);
    __builtin_amdgcn_raw_buffer_store_b64(t, r, voff, soff, 2);
}
// ---- loads of the persistent two-launch kernels (k_p1 / k_p2 / k_p2k) -------------------------------------------------------------------
// Round 5 issued these loads as inline assembly and stated every wait by hand (vm_wait<N>): 1.2 % on the two-launch form at N = 65536, nothing
// at N = 262144 or on the headline block kernel (profiles/r05/NOTES.md section 2).  Round 6 went back to compiler-visible loads and the
// compiler's own waits: the hand-stated counts were correct only while the register allocator never moved an asm result ahead of its wait
// and the vector-memory instructions behind the loads matched the count, which nothing checked.  What is left of that form:
// the descriptor as four plain integers, and the empty asm ties of vm_wait / vm_settle, which pin the schedule the kernels were measured with.
typedef int srd_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ srd_t make_srd(const void *base, unsigned bytes)
{
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    srd_t r;
    r.x = (int)(unsigned)a; r.y = (int)((unsigned)(a >> 32) & 0xFFFFu); r.z = (int)bytes; r.w = 0x00020000;   // as make_rsrc: stride 0, raw
    return r;
}
template <bool NT>
__device__ __forceinline__ cf ald2(srd_t r, unsigned voff, unsigned soff)
{
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((unsigned long long)(unsigned)(r.y & 0xFFFF) << 32) | (unsigned)r.x), 0, r.z, 0x00020000);
    const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(rr, voff, soff, NT ? 2 : 0);
    return mk(__uint_as_float(t.x), __uint_as_float(t.y));
}
// the sixteen values of a tile's loads, needed HERE: the compiler puts its own wait in front of these empty ties, and no use moves ahead of them
__device__ __forceinline__ void vm_wait(cf (&a)[16])
{
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]) :: "memory");
    asm volatile("" : "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15]) :: "memory");
}
// a value from a compiler-visible load, made ready HERE (the compiler puts its own wait in front of this use)
__device__ __forceinline__ void vm_settle(cf &v) { asm volatile("" : "+v"(v) :: "memory"); }

template <bool NT>
__device__ __forceinline__ void bst2t(__amdgpu_buffer_rsrc_t r, unsigned voff, cf v)
{
    u32x2 t;
    t.x = __float_as_uint(v.x); t.y = __float_as_uint(v.y);
    __builtin_amdgcn_raw_buffer_store_b64(t, r, voff, 0, NT ? 2 : 0);
}
__device__ __forceinline__ void st2(float2 *p, cf a) { *reinterpret_cast<cf *>(p) = a; }
// output samples of the channel kernels (k_c256 / k_c512 / k_c1024): written once, read by nobody on the device: streamed (nt) stores, round 6:
// -4 % on the wide kernels (profiles/r06/ch_nt_stores_ab.txt)
__device__ __forceinline__ void st2_out(float2 *p, cf a)
{
    __builtin_nontemporal_store(a, reinterpret_cast<cf *>(p));
}

// 16-byte buffer store of two complex values (NT: streamed, aux bit 1)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// 16-byte buffer load (two complex values)
__device__ __forceinline__ u32x4 bld4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
}
template <bool NT>
__device__ __forceinline__ void bst4(__amdgpu_buffer_rsrc_t r, unsigned voff, cf a, cf b)
{
    u32x4 t;
    t.x = __float_as_uint(a.x); t.y = __float_as_uint(a.y); t.z = __float_as_uint(b.x); t.w = __float_as_uint(b.y);
    __builtin_amdgcn_raw_buffer_store_b128(t, r, voff, 0, NT ? 2 : 0);
}
// the value of the neighbouring lane (lane ^ 1): DPP quad_perm [1, 0, 3, 2]
__device__ __forceinline__ float swap_pair(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));
}
// the sum over the lane's quad (lanes 4 q .. 4 q + 3), the same bits in all four: (x0 + x1) + (x2 + x3) by DPP quad_perm [1, 0, 3, 2], [2, 3, 0, 1]
__device__ __forceinline__ float quad_sum(float x)
{
    x += swap_pair(x);
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, true));
}


}  // namespace fdc
