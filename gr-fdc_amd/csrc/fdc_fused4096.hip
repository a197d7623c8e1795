// N = 4096 in ONE launch (round 6): overlap-save gather + forward transform + every channel's slice, phase / window, ifftshift,
// inverse transform, overlap discard and * l — the spectrum of a block never leaves its compute unit.  This is the block length of the
// reference's own example flowgraph (examples/FDC_example.grc: l = 256 / 512 / 1024 / 512 at N = 4096) and of BASELINE configs[0]; the
// two-launch spectrum path it replaces there (k_fft4096 + k_c256 / k_c512 / k_c1024) writes the bins some channel reads to memory and reads
// them back: python/FrequencyDomainChannelizer.py:206 (fft_vcc) -> :214-216 (vector_cut_vxx, phase_shifting_windowing_vcc) -> :218-226
// (ifft, vector_cut_vxx, multiply_const) per channel.
//
//   a workgroup takes T blocks, T teams of four waves: each team transforms one block (4096 points = 32 KiB, the same three DFT-16 layers as
//   k_fft4096, fdc_chanwide.hip) and stores the shifted, 1/N-scaled spectrum to LDS over its exchange tile (32 KiB); every one of the 4 T
//   WAVES then owns rows — (block of the workgroup, channel) — of ONE channel width: the plan's schedule, made by the host (fdc_plan.hip,
//   plan_fused4096).  T = 2 (512 threads, two workgroups on a unit) for plans with wide rows: a wave's instructions cost the same for one
//   row as for a full wave of them, and the reference's example plan fills its 1024- and 512-bin waves only with the rows of two blocks;
//   T = 1 (256 threads, FOUR workgroups on a unit: four barrier domains instead of two, 11 - 12 % faster) where no row is wide.
//       l =  256: 16 lanes x 16 points per row, up to eight rows (two sets of four) per wave   (the row machinery of k_c256)
//       l =  512: 16 lanes x 32 points, up to four rows                                        (k_c512)
//       l = 1024: 32 lanes x 32 points, up to two rows                                         (k_c1024)
//       l =  128:  8 lanes x 16 points, eight rows; l = 64 / 32 / 16: 4 / 2 / 1 lanes, eight rows   (DFT-16 over a, exchange inside the row, DFT-8 / 4 / 2 over b)
//     a row reads its slice from the LDS spectrum and its window row (phase counter in closed form) from memory, runs its first DFT
//     layer in registers; ONE workgroup barrier (every slice has been read) and the tile is free for the rows' own exchanges, which stay
//     inside a wave: no further barrier.  Sum of the rows' exchange areas <= the T tiles, at most 4 T waves of rows: plans with more
//     (channels that overlap to more than 4096 bins in total, more than 32 narrow channels) stay on the spectrum path.
// Bytes per block: H = N - N/R new input samples + sum(lout) output samples, nothing else (the window rows and tables are cache hits).
#include "fdc_kernels.h"
#include "fdc_radix16.hpp"
#include "fdc_devutil.hpp"
#include <type_traits>
#include "fdc_iq.hpp"
#include "fdc_fine.hpp"

namespace fdc {

extern __shared__ __attribute__((aligned(16))) unsigned char fdc_smem_f4[];

// output stores streamed (nt), input loads plain (A/B: profiles/r06/NOTES.md section 8)
namespace {
constexpr int kF4TilePts = 16 * 272;                         // exchange tile of one block's forward transform; then its spectrum; then rows' exchanges
// LDS image for T blocks (teams of four waves) per workgroup: [T tiles][W_256^(x y) 16 x 18][W_4096^(x y) 16 x 18][schedule: 4 T waves x 8 slots]
// and, with wide rows, [W_1024^(x p) 16 x 34][W_64^(c p) 2 x 34]
constexpr int f4_off_t256(int T) { return T * kF4TilePts * 8; }
constexpr int f4_off_t4k(int T) { return f4_off_t256(T) + 16 * 18 * 8; }
constexpr int f4_off_rows(int T) { return f4_off_t4k(T) + 16 * 18 * 8; }
constexpr int f4_lds(int T) { return f4_off_rows(T) + 32 * T * 32; }                 // T = 2: 76288 (two workgroups per unit); T = 1: 40448 (four)
constexpr int f4_off_w1k(int T) { return f4_lds(T); }
constexpr int f4_off_w64(int T) { return f4_off_w1k(T) + 16 * 34 * 8; }
constexpr int f4_lds_wide(int T) { return f4_off_w64(T) + 2 * 34 * 8; }              // T = 2: 81184
static_assert(sizeof(F4Row) == 32, "schedule rows are copied 16 bytes at a time");
static_assert(2 * f4_lds_wide(2) <= 160 * 1024 && 4 * f4_lds(1) <= 160 * 1024 && 3 * f4_lds_wide(1) <= 160 * 1024, "LDS budget");

__device__ __forceinline__ constexpr int pos32(int k) { return 16 * (k & 1) + rev16(k >> 1); }   // dft32 leaves X[k0 + 2 k1] in v[16 k0 + rev16(k1)]

// stores of some lanes of a wave, then loads of others of the SAME wave: LDS serves a wave's accesses in order, the compiler is told not to move them
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void out_st(float2 *p, cf v, float)
{
    __builtin_nontemporal_store(v, reinterpret_cast<cf *>(p));
}
// integer output (fdc_pipeline_set_output_format): the sample narrowed times s (oq_bits), one dword (sc16) / one 16-bit store (sc8), nt as above
template <class TO, class TU>
__device__ __forceinline__ void out_st_oq(TO *p, cf v, float s)
{
    const TU u = (TU)oq_bits(TO{}, v, s);
    __builtin_nontemporal_store(u, reinterpret_cast<TU *>(p));
}
__device__ __forceinline__ void out_st(sc16 *p, cf v, float s) { out_st_oq<sc16, unsigned>(p, v, s); }
__device__ __forceinline__ void out_st(sc8 *p, cf v, float s) { out_st_oq<sc8, unsigned short>(p, v, s); }

// Fine tuning in the stores (the FINE forms; fdc_fine.hpp): rows[wave][slot] = the increment of the schedule row's channel and where its step factors start,
// block0 = the stream's index of the launch's block 0
struct F4Fine { const FineChan *rows; const float2 *step; unsigned long long block0; };
// what the stores of one row need: its base (once per row) and its step factors, moved so that sample t of the L-point transform reads st[t]
__device__ __forceinline__ void fine_row(const F4Fine &fa, int slot, const F4Row &ri, int m0, int L, cf &base, const float2 *&st)
{
    const FineChan f = fa.rows[slot];
    base = fine_base(f.inc, fa.block0 + (unsigned long long)(m0 + (ri.valid ? ri.valid - 1 : 0)), (unsigned)ri.lout);
    st = fa.step + (f.step_off - (L - ri.lout));
}
// the value of sample t of a row as it is stored; FINE: turned first
template <bool FINE>
__device__ __forceinline__ cf fine_val(cf v, [[maybe_unused]] cf base, [[maybe_unused]] const float2 *st, [[maybe_unused]] int t)
{
    if constexpr (FINE) return fine_rotate(v, base, ld2(st + t));
    else return v;
}

struct RowAt { const float2 *win; const float2 *spec; long long dst; bool on; };
// ri.valid: 0 = no row, 1 + k = a row of the workgroup's block k
// fbm = (first block of the call + first block of the launch) mod R
__device__ __forceinline__ RowAt row_at(const F4Row &ri, int L, int m0, int nb, int mbase, int fbm, int R, const float2 *wins,
                                        long long nb_call, const float2 *tiles)
{
    const int k = ri.valid ? ri.valid - 1 : 0, m = m0 + k;
    const int cnt = (int)(((unsigned)(fbm + m) % (unsigned)R) * (unsigned)ri.shift % (unsigned)R);     // phase counter in closed form (lib/phase_shifting_windowing_vcc_impl.cc:58,83-89)
    return RowAt{wins + (ri.win_off + cnt * L), tiles + k * kF4TilePts + ri.f, nb_call * ri.out_off + ((long long)mbase + m) * ri.lout - (L - ri.lout),
                 ri.valid != 0 && m < nb};
}
}  // namespace

// TEAMS teams of four waves (256 TEAMS threads): team t transforms block TEAMS g + t of workgroup g's blocks; then every wave runs the rows the schedule gives it.
// TEAMS = 2 wherever rows of ONE block would leave waves part empty (all wide rows: the reference's example fills its 1024- and 512-bin waves only with the
// rows of two blocks); TEAMS = 1 — four independent workgroups per unit instead of two of twice the size — where the schedule of one block fits four waves.
// wcls: four bits per wave: 0 = no rows, 1 = l = 256 (slots 0..3), 2 = l = 256 two sets (slots 0..7), 3 = l = 512 (slots 0..3), 4 = l = 1024 (slots 0..1),
// 5 = l = 128, 6 = l = 64, 7 = l = 32, 8 = l = 16 (slots 0..7 each)
// ROWS: the waterfall epilogue (fdc_waterfall.hip): wf[m][p] = sum of |X|^2 over shifted bins 4 p .. 4 p + 3 of the 1/N-scaled spectrum, taken from the
// registers the spectrum store leaves; ROWS = false is the kernel without it, instruction for instruction
// TI: the input sample, float2 or complex integer (sc16 / sc8, fdc_iq.hpp: widened times iq_scale right after its load)
// TO: the output sample, float2 or complex integer (sc16 / sc8: narrowed times oq_scale in out_st)
// (the body is fdc_fused4096_body.inc, shared with the FINE forms below)
template <bool WIDE, int TEAMS, bool ROWS, class TI = float2, class TO = float2>
__global__ __launch_bounds__(256 * TEAMS, 4 /* waves per SIMD */) void k_f4096(const TI *__restrict__ in, size_t in_stride, TO *__restrict__ out, int nb, int R,
                                                  int mbase, int nb_call, int fbm /* (first block of the call + mbase) mod R */, const float2 *__restrict__ tw,
                                                  int twstride /* ntab / 4096 */, const float2 *__restrict__ wins,
                                                  const F4Row *__restrict__ rows, unsigned wcls,
                                                  typename IqTail<TI, TO>::type wf /* integer TI / TO: iq_scale / oq_scale */)
{
    constexpr bool FINE = false;
    [[maybe_unused]] const F4Fine fa{};
#include "fdc_fused4096_body.inc"
}

// FINE: fine tuning (fdc_fine.hpp) in the stores: every sample turned by base * step before it is stored (and before oq_bits for integer TO).  The same
// arguments and the fine-tuning tables behind them; no waterfall form
template <bool WIDE, int TEAMS, class TI = float2, class TO = float2>
__global__ __launch_bounds__(256 * TEAMS, 4 /* waves per SIMD */) void k_f4096_fine(const TI *__restrict__ in, size_t in_stride, TO *__restrict__ out, int nb, int R,
                                                  int mbase, int nb_call, int fbm, const float2 *__restrict__ tw, int twstride, const float2 *__restrict__ wins,
                                                  const F4Row *__restrict__ rows, unsigned wcls, typename IqTail<TI, TO>::type wf, const F4Fine fa)
{
    constexpr bool FINE = true, ROWS = false;
#include "fdc_fused4096_body.inc"
}

// The forms of the kernel, stated ONCE (fdc_forms.hpp): (WIDE, TEAMS) of either kernel on every input and output sample type; FINE takes
// k_f4096_fine, which has no waterfall form; ROWS on float input and float output only.  f(kernel, TEAMS, LDS bytes, TI{}, TO{}, FINE) for the forms
// that match (kEvery: every value of that argument)
template <class F>
static void for_f4_forms(int wide, int teams, int rows, int fine, int ifmt, int ofmt, F &&f)
{
    auto form = [&](auto W, auto T, auto ROWS, auto FINE, auto ti, auto to) {
        using TI = decltype(ti);
        using TO = decltype(to);
        constexpr bool kWide = W() != 0, kFloat = std::is_same<TI, float2>::value && std::is_same<TO, float2>::value;
        constexpr int kLds = kWide ? f4_lds_wide(T()) : f4_lds(T());
        if constexpr (FINE() && !ROWS()) f(k_f4096_fine<kWide, T(), TI, TO>, T, kLds, ti, to, FINE);
        else if constexpr (!FINE() && (!ROWS() || kFloat)) f(k_f4096<kWide, T(), ROWS() != 0, TI, TO>, T, kLds, ti, to, FINE);
    };
    for_values<0, 1>(wide, [&](auto W) { for_values<1, 2>(teams, [&](auto T) { for_values<0, 1>(rows, [&](auto ROWS) { for_values<0, 1>(fine, [&](auto FINE) {
        for_samples(ifmt, [&](auto ti) { for_samples(ofmt, [&](auto to) { form(W, T, ROWS, FINE, ti, to); }); });
    }); }); }); });
}

hipError_t init_fused4096_kernels()
{
    hipError_t e = hipSuccess;
    for_f4_forms(kEvery, kEvery, kEvery, kEvery, kEvery, kEvery, [&](auto k, auto, int lds, auto, auto, auto) {
        if (e == hipSuccess) e = set_block_lds(reinterpret_cast<const void *>(k), lds);
    });
    return e;
}

int fused4096_tile_points() { return kF4TilePts; }

hipError_t launch_fused4096(const F4Launch &a)
{
    if (a.nb_chunk <= 0) return hipSuccess;
    if (a.teams == kEvery || a.ifmt == kEvery || a.ofmt == kEvery) return hipErrorInvalidValue;      // a launch names one form
    // whether a wave holds wide rows (l = 512 / 1024: the WIDE form)
    bool wide = false;
    for (int w = 0; w < 8; w++) wide = wide || ((a.wcls >> (4 * w)) & 0xfu) == 3 || ((a.wcls >> (4 * w)) & 0xfu) == 4;
    const int fbm = (int)((a.first_block + a.mbase) % a.R);
    const F4Fine fa{a.fine_rows, a.fine_step, (unsigned long long)(a.first_block + a.mbase)};
    hipError_t e = hipErrorInvalidValue;                        // stays if no form matches
    for_f4_forms(wide, a.teams, a.wf != nullptr, a.fine_rows != nullptr, a.ifmt, a.ofmt, [&](auto k, auto T, int lds, auto ti, auto to, auto FINE) {
        using TI = decltype(ti);
        using TO = decltype(to);
        // one workgroup per T blocks, a multiple of the eight XCDs
        const dim3 grid((unsigned)(8 * (((a.nb_chunk + T() - 1) / T() + 7) / 8)));
        const TI *in = static_cast<const TI *>(a.in);
        TO *out = static_cast<TO *>(a.out);
        const typename IqTail<TI, TO>::type tail = iq_tail<TI, TO>(a.wf, a.iscale, a.oscale);
        if constexpr (FINE())
            hipLaunchKernelGGL(k, grid, dim3(256 * T()), lds, a.s, in, a.in_stride, out, a.nb_chunk, a.R, a.mbase, a.nb_call, fbm, a.tw, a.ntab / 4096, a.wins, a.rows,
                               a.wcls, tail, fa);
        else
            hipLaunchKernelGGL(k, grid, dim3(256 * T()), lds, a.s, in, a.in_stride, out, a.nb_chunk, a.R, a.mbase, a.nb_call, fbm, a.tw, a.ntab / 4096, a.wins, a.rows,
                               a.wcls, tail);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace fdc
