// gfx950 "one block per CU" form of the uniform-plan path for N = 65536 = 256 x 256, l = 256, R = 2
// (BASELINE configs[1] / [2]): overlap-save gather, forward FFT, window, per-channel IFFT, overlap discard and the
// FFT over the channel slots in ONE kernel, with the intermediate G (fdc_fast256.hip: 128 rows t' x 256 columns n1
// per block = 256 KiB) never leaving the compute unit.
//
// Why: the two-launch form (k_p1 + k_p2) moves G out to memory and back, 2.03x the algorithmic bytes, and both of
// its kernels sit at the copy rate of their own traffic (profiles/r01/NOTES.md); only moving fewer bytes helps.
// G does not fit the 160 KiB of LDS, but it fits the register file: ONE 512-thread workgroup per CU (8 waves, 2 per
// SIMD, 256 VGPRs each) keeps a whole block's G in 128 VGPRs per lane.
//
//   stage 1, 8 passes of 32 columns: every wave owns 4 columns per pass, lane = col + 4*b holds the 16 rows
//       n2 = 16a + b of its column.  Both 16 x 16 exchanges of the FFT-256 / IFFT-256 pair stay inside the wave
//       (a private 8.5 KiB LDS scratch, in-order LDS queue, no s_barrier), so the eight waves drift apart and one
//       wave's LDS phases overlap the other waves' DFT-16 arithmetic.  The next pass's rows are loaded into
//       registers a pass ahead: at the top of the pass into a second row set, or (SPREAD) four at a time between its phases — at P >= 4 into the
//       registers the pass computes on, dead by then, with the lane's twiddle row in the second set's place (kBlkOneSet).  The 8 kept outputs t = b + 16q, q >= 8, of every pass go
//       into the G registers (indexed by the pass: s_set_gpr_idx).
//   stage 2, 2 chunks of 64 rows t': the FFT-256 over n1 = 32 pass + c5 starts with a DFT-8 over the pass index, which
//       is the register index of G (no exchange), then W_256^(c5 klo), then ONE trip through LDS ([row][klo][c5]) to the
//       lane that owns (row, klo) and transforms the remaining 32 points over c5 in registers.  Slot klo + 8 khi of 64
//       consecutive rows: every wave store is a 512-byte run of one channel.  Two s_barriers per chunk.
// Every LDS access is base register + immediate offset; all layouts are padded (not XOR-swizzled) so that no
// per-element address arithmetic is left, and conflict-free for the lane groups of ds_write_b64 (16 lanes) and
// ds_read_b64 (32 lanes) (MI355X_MICROARCH.md, LDS table).
//
// Input rows are read in 32-byte pieces per wave (4 columns x 8 B); the 8 waves of the workgroup cover 256
// contiguous bytes of each row in the same pass.  Consecutive blocks overlap by half (R = 2): the workgroups of one
// XCD take CONSECUTIVE blocks in the same round, so the shared half is fetched from memory once and served to the
// neighbour from that XCD's L2.
//
// The arithmetic is the uniform-plan commutation of fdc_fast256.hip with the same number of multiplications per value.  At N = 16384 the
// tables and rounding points are the same too; at N = 32768 and 65536 stage 1 factors its tables otherwise (k_blk256, kSplit), and at N = 65536 the
// channelizer on the grid and half a slot up takes the wave's part of them from memory through the scalar path and cb as one table entry
// (kBlkSrow, SROW), so the result matches k_p1 + k_p2 to a few ulps either way; parity against the oracle: tests/test_parity_gpu.py,
// tests/test_block256_stage1_tables_gpu.py, tests/test_block256_scalar_row_gpu.py.
#include "fdc_blockcommon.hpp"
#include "fdc_iq.hpp"

namespace fdc {

extern __shared__ __attribute__((aligned(16))) unsigned char fdc_smem_blk[];

typedef unsigned long long u8v __attribute__((ext_vector_type(8)));

// SROW (k_blk256): four table entries at a wave-uniform address in the constant address space, i.e. one s_load_dwordx8 (two adjacent ones: the
// compiler makes them one s_load_dwordx16), and the complex multiplication that takes such an entry from its scalar register pair (cmul,
// fdc_radix16.hpp, with b in SGPRs)
typedef unsigned int u32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(4))) u32x8 srow_piece;
__device__ __forceinline__ cf cmul_s(cf a, cf b)
{
    cf r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "=&v"(r) : "v"(a), "s"(b));
    return r;
}

// The block length is a template parameter: N = 256 rows x (32 P) columns with P = 2, 4, 8 passes of 32 columns, i.e. N = 16384,
// 32768, 65536; the number of channel slots is the number of columns N1 = 32 P.  Stage 1 does not depend on P except through the row
// pitch and the table sizes (a pass is a pass); G is 16 P registers per lane; stage 2 is a DFT-P over the pass index in registers, one
// trip through LDS and the same DFT-32 over c5.  With P < 8 a trip holds all 128 rows of a run (P = 8: 64) and a wave reads
// (klo = wave mod P, row half = wave div P).
//
// LDS map (bytes).  Stage-1 scratch: the eight per-wave exchange strips (fdc_blockcommon.hpp), kStripsEnd bytes.
// Which forms of k_blk256 have a spread instantiation (SPREAD: the next pass's row loads in four groups over the pass, one_pass): the channelizer on
// the grid and half a slot up.  Not the forms whose registers the placement costs
// (scratch, a spill): offset plans, the forward transform, and at P = 8 the forms at R = 4 or with integer output.
template <int P, bool OFF, bool FWD, bool R4, class TO>
constexpr bool kBlkSpread = !OFF && !FWD && !(P == 8 && (R4 || !std::is_same<TO, float2>::value));

// Which forms of k_blk256 take the wave's twiddle row through the scalar path (SROW, one_pass) instead of the LDS table UR, and cb as one entry of a
// table of N1 / 4 rows in UR's place: at P = 8 the channelizer on the grid and half a slot up at R = 2, whatever the sample formats.  The forms that must
// give the same values go together: both spread twins of a form (tests/test_block256_load_placement_gpu.py), and the integer-output forms with the float
// form whose narrowed output theirs must equal byte for byte (tests/test_iq_output_gpu.py) — cb is one table entry here and a float product of two
// there.  Not P = 2 (no UR there); not P = 4, where it is worth nothing measurable and costs the spread forms 14 - 26 spilled SGPRs; offset plans,
// R = 4 and the forward transform have not been built this way (they stand at 94 - 106 of 106 SGPRs and 250 - 256 VGPRs as they are, and the scheme
// takes 7 - 16 SGPRs more): profiles/srow/NOTES.md.
template <int P, bool OFF, bool FWD, bool R4>
constexpr bool kBlkSrow = P == 8 && !OFF && !FWD && !R4;

// Which forms of k_blk256 run stage 1 on ONE row set, with the lane's twiddle row W_256^(b p) held in registers for the length of a block's stage 1
// (one_pass, the pass loop): the spread forms at P >= 4.  A spread pass is done with its rows at its first exchange write (22 % of the pass); with the
// first group of the next pass's loads behind that write instead of behind the first dft16, all sixteen land in the registers they are used from, and the
// second set's 32 registers hold the row that every pass otherwise reads from LDS twice (forward, and conjugated for the inverse).  The spread forms are
// never offset plans: one row serves both uses.  Not P = 2: two workgroups per CU there, 128 registers each, and the row does not fit beside G and the
// rows (128 VGPRs with 10 of them spilled to 44 bytes of scratch, against 126 and none): profiles/one_row_set/NOTES.md.
template <int P, bool SPREAD>
constexpr bool kBlkOneSet = SPREAD && P >= 4;

template <int P, bool SROW = false>
struct BlkGeom {
    static_assert(P == 2 || P == 4 || P == 8, "passes of 32 columns: N = 16384, 32768 or 65536");
    static_assert(!SROW || P > 2, "the scalar wave row replaces UR, which P = 2 does not have");
    static constexpr int kN1 = 32 * P;                            // columns = channel slots
    static constexpr int kN = 256 * kN1;
    static constexpr int kJT = P == 8 ? 4 : 8;                    // 16-row groups per stage-2 trip (64 or 128 rows)
    static constexpr int kJB = P == 8 ? 2 : P == 4 ? 4 : 8;       // 16-row groups within reach of one ds base register (16-bit byte offset)
    // stage-2 trip: [rows][32 P + 6] (P klo x 32 c5 + 6).  The row stride in dwords is 12 mod 64 for every P: the 16-lane groups of
    // ds_read_b128 (lanes {0-3,12-15,20-27}, ...; MI355X_MICROARCH.md, LDS table) then cover all 64 banks, and the 16 contiguous lanes
    // of a ds_write_b64 group (4 rows x 4 columns) all 32 (a stride of 8 mod 64 is conflict-free for the stores only: 1.46 M conflict
    // cycles at P = 8)
    // P = 2: 32 P + 2 (4 dwords mod 64: as clean for the reads), which brings the workgroup under half of the LDS: two workgroups per CU
    static constexpr int kLd = P == 2 ? 32 * P + 2 : 32 * P + 6;
    static constexpr int kTripBytes = 16 * kJT * kLd * 8;         // P = 8: 134144
    static constexpr int kOffCt = kTripBytes > kStripsEnd ? kTripBytes : kStripsEnd;   // stage-2 twiddles [32][P], behind the trip buffer and the strips
    static constexpr int kOffWrow = P == 8 ? 136960 : kOffCt + 32 * P * 8;   // tables: above the strips and the trip buffer
    // The stage-1 tables behind wrow.  kSplit (P > 2): the lane table LT (64 rows of 18), the wave rows UR ([kN1 / 4][16]) and the rows of CB
    // ([P + 8][16]) — cb comes from LDS.  SROW: no UR (the wave row comes from memory through the scalar path) and CB whole, [kN1 / 4][16], in its place.
    // P = 2: Bt (32 rows of 18) and SA (16 P rows of 18), cb from memory: the on-grid form there runs two workgroups per CU on
    // 81664 of 81920 bytes and has no room for the two wave tables.
    static constexpr bool kSplit = P > 2;
    static constexpr int kOffLT = kOffWrow + 16 * 18 * 8;
    static constexpr int kOffUR = kOffLT + 64 * 18 * 8;
    static constexpr int kOffB = kOffLT, kOffSA = kOffB + 32 * 18 * 8;
    static constexpr int kOffSoff = kSplit ? kOffUR + (SROW ? 0 : kN1 * 4 * 8) : kOffSA + 16 * P * 18 * 8;
    static constexpr int kOffCbl = kOffSoff + kN1 * 4;
    static constexpr int kCblRows = SROW ? kN1 / 4 : P + 8;
    static constexpr int kLds = kOffCbl + (kSplit ? kCblRows * 16 * 8 : 0);   // P = 8: 159744 (SROW: 157696); P = 2: 81664
    static constexpr int kOffWrowF = kLds;                        // offset plans: the forward twiddle rows behind everything else
    static constexpr int kLdsOff = kOffWrowF + 16 * 18 * 8;       // P = 8: 162048
    static_assert(kLdsOff <= 160 * 1024 && kLds <= 160 * 1024, "LDS budget");
    static_assert(kOffCt >= kStripsEnd && kOffCt + 32 * P * 8 <= kOffWrow, "stage-2 trip buffer and twiddles below the tables, tables above the strips");
    static_assert((16 * (kJB - 1) * kLd + 32 * (P - 1)) * 8 < 65536, "ds offsets of a base register");
    static_assert(!SROW || kCblRows * 16 * 8 == kN1 * 4 * 8, "the whole cb table takes what UR had: the total shrinks by the two-factor table");
};

// FWD = false: the channelizer (above).  FWD = true: the same machinery as a plain forward transform of the block (no window,
// no inverse transform).  Stage 1 stops after the forward FFT-256 of a column: T[k2][n1] = A[k2] W_N^(n1 k2) / N, 512 KiB per block —
// twice what the G registers hold.  Rounds 2-5 kept the half k2 < 128 in G and sent the other half through 256 KiB of per-workgroup
// scratch: the counters (profiles/r06/pmc_summary_fwd.txt) say that trip is real traffic — WRITE 807 MB + FETCH 560 MB per 1024 blocks
// for 805 MB of work, at 5.5 TB/s: the kernel was bound by the memory system on bytes of which 39 % were its own scratch.
// Round 6 measured the alternative, two workgroups per block (each the forward FFT-256 of every column for half of the rows k2) and no scratch:
// it moves 805 MB instead of 1367 and is SLOWER, full band 0.2525 against 0.2405 ms per 1024 blocks, nothing written 0.2017 against 0.188
// (profiles/r06/fwd_ab.txt): its passes are a third of the channelizer's (no inverse transform), so the rows requested one pass ahead are not
// there when the pass starts, and it asks for every row twice.
// Stage 2 runs on G, then on the scratch half; its "slots" are the k1 of the spectrum: bins 256 c + k2 of the SHIFTED spectrum (the (-1)^n1
// of cbt moves k1 by 128 = fftshift).  This is what plans that need a spectrum in memory (mixed channel plans, the sinks, the debug port) use
// instead of two passes through a scratch of the whole batch.
// R4 = true: the channelizer at relinvovl = 4 (the reference's default overlap, grc/FDC_FrequencyDomainChannelizer.xml:61): three
// quarters of every inverse transform are kept, G is 192 rows x N1 columns.  The rows t >= 128 stay in the G registers
// as for R = 2; the rows 64 <= t < 128 take the route of the forward-transform variant: per-workgroup scratch (L2),
// read back for a third, 64-row run of stage 2.  Off the grid (OFF) the window phase counter runs: a constant j^p per block in cb.

// HALF = true: every channel half a slot higher (f = 256 slot + 128: a bank centred on multiples of 256 bins) WITHOUT the offset machinery.  The block
// modulated by exp(-2 pi i 128 n / N) = W_N^(128 n1) (-1)^n2: the (-1)^n2 moves every column's spectrum by half its length, which together with the
// ifftshift of the inverse is the identity — the value stays in its register, the tables are read at k2 ^ 128 (q ^ 8), W_N^(128 n1) is in cbt (the host
// builds it for r = 128 as for any offset).  No second twiddle table, no rotated exchange, both row sets: the on-grid rate, and relinvovl 4 too
// (128 mod 4 = 0: the window phase stays 0).
// TI: the input sample, float2 or complex integer (sc16 / sc8: fdc_iq.hpp); integer rows are loaded as they are (4 / 2 bytes a sample) and
// widened in registers at the top of the pass that transforms them, times iq_scale.  TO: the output sample, float2 or complex integer (sc16 / sc8:
// narrowed in the store, times oq_scale, oq_bits): one dword / one 16-bit store per sample at the same per-wave offsets, scaled to the narrow element
// SPREAD: the row loads of the next pass are issued in groups between the phases of a pass (ld_rows) instead of all sixteen at its top; plain loads
// only: a launch with streamed input loads (hints bit 1, a diagnostic) takes the form without it
template <int P, bool NT, bool OFF, bool FWD, bool R4 = false, bool HALF = false, class TI = float2, class TO = float2, bool SPREAD = false>
__global__ FDC_PLAIN_DS __launch_bounds__(512, (P == 2 && !OFF && !R4 && !FWD) ? 4 : 2) void k_blk256(const TI *__restrict__ in, size_t in_stride, TO *__restrict__ out,
                                                const float2 *__restrict__ tw256, const float2 *__restrict__ twq,
                                                const float2 *__restrict__ cbt, const float *__restrict__ shn,
                                                const long long *__restrict__ slot_off, long long out_base,
                                                long long nb_call, unsigned out_bytes, int nb, int hints,
                                                unsigned long long *__restrict__ dbg /* unused (null): keeps the kernarg layout */, int roff, long long first_block,
                                                float2 *__restrict__ fwd_scratch, const unsigned *__restrict__ keep,
                                                typename IqTail<TI, TO>::type gpow /* integer TI / TO: iq_scale / oq_scale */)
{
    constexpr bool kSrow = kBlkSrow<P, OFF, FWD, R4>;
    constexpr bool kOne = kBlkOneSet<P, SPREAD>;
    typedef BlkGeom<P, kSrow> GM;
    constexpr bool kIq = !std::is_same<TI, float2>::value, kOq = !std::is_same<TO, float2>::value;
    static_assert(!SPREAD || kBlkSpread<P, OFF, FWD, R4, TO>, "no spread form of this one");
    static_assert(!kIq || !FWD, "integer input: the channelizer forms (the forward transform takes widened input)");
    static_assert(!kOq || !FWD, "integer output: the channelizer forms");
    constexpr unsigned kEs = (unsigned)sizeof(TI);                              // bytes per input sample
    constexpr unsigned kOs = (unsigned)sizeof(TO);                              // bytes per output sample
    [[maybe_unused]] const float iq_scale = iq_tail_scale(gpow);
    [[maybe_unused]] const float oq_scale = oq_tail_scale(gpow);
    static_assert(!HALF || (!OFF && !FWD), "the half-slot form is a variant of the on-grid channelizer");
    constexpr int kN1 = GM::kN1, kLd = GM::kLd, kJT = GM::kJT, kJB = GM::kJB;
    float2 *scr = reinterpret_cast<float2 *>(fdc_smem_blk);                     // stage 1: 8 wave scratches; stage 2: the trip buffer
    float2 *wrow = reinterpret_cast<float2 *>(fdc_smem_blk + GM::kOffWrow);     // [b][p - 1 mod 16] = W256^(b p), rows of 18 (ld_row_sh)
    // The inter-pass twiddle times the window, W_N^(16 q (32 pass + c5)) shape[b + 16 q] / N, c5 = 4 wave + col, in two factors.
    // kSplit: LT[lane = col + 4 b][q] = W_N^(16 q col) shape[b + 16 q] / N cbt[col][b] depends on the lane and on nothing else;
    // UR[8 pass + wave][q] = W_N^(16 q (32 pass + 4 wave)) is the same for every lane of a wave (a broadcast read).  cbt[n1 = 32 pass + c5][b] =
    // (-1)^n1 W_N^(n1 (b + r)) factors the same way: cbt[col][b] is in LT, CB[pass][b] = cbt[32 pass][b] and CB[P + wave][b] =
    // cbt[4 wave][b] are read once per pass (the second is a constant of the lane, but there is no register to keep it in).
    // SROW: the row UR[8 pass + wave] is row 32 pass + 4 wave of twq as it lies in memory (HALF: its two halves swapped), the same for the whole wave:
    // read from there in four pieces of four entries through the scalar path, each entry the scalar operand of one multiplication; no UR in LDS, and in
    // its place CB[8 pass + wave][b] = cbt[32 pass + 4 wave][b] whole: one read per pass, no product.
    // P = 2: Bt[c5][q] = W_N^(16 c5 q) and SA[pass][b][q] = shape[b + 16 q] / N W_N^(512 pass q); cbt[n1][b] comes from memory a pass ahead.
    constexpr bool kSplit = GM::kSplit;
    float2 *LT = reinterpret_cast<float2 *>(fdc_smem_blk + GM::kOffLT);
    float2 *UR = reinterpret_cast<float2 *>(fdc_smem_blk + GM::kOffUR);
    float2 *CBL = reinterpret_cast<float2 *>(fdc_smem_blk + GM::kOffCbl);
    float2 *Bt = reinterpret_cast<float2 *>(fdc_smem_blk + GM::kOffB);
    float2 *SA = reinterpret_cast<float2 *>(fdc_smem_blk + GM::kOffSA);
    unsigned *soff = reinterpret_cast<unsigned *>(fdc_smem_blk + GM::kOffSoff);
    float2 *ctab = reinterpret_cast<float2 *>(fdc_smem_blk + GM::kOffCt);       // [c5][klo] = W_N1^(c5 klo): stage 2, after the DFT-P
    const int tid = threadIdx.x;
    // stage-1 roles
    const int w = tid >> 6, lane = tid & 63, col = lane & 3, b = lane >> 2, c5 = 4 * w + col;
    // stage-2 roles: writer = the stage-1 role (column c5, rows b + 16 j); reader: row = lane (+ 64 row half), klo = wave mod P
    // FWD with a plan that reads part of the spectrum only: which of this wave's 64-bin stores some channel reads at all
    // ([klo = wave mod P][k2 / 64], bit = register index of the slot); the others are dropped (offset beyond the descriptor's extent)
    unsigned mqs[4] = {~0u, ~0u, ~0u, ~0u};
    if (FWD && keep) {
        const int wu = __builtin_amdgcn_readfirstlane(w) % P;
#pragma unroll
        for (int q = 0; q < 4; q++) mqs[q] = keep[wu * 4 + q];
    }

    const int grid = gridDim.x, first = xcd_first_block();
    if (first >= nb) return;

    constexpr unsigned inbytes = (unsigned)GM::kN * kEs;
    constexpr unsigned kRowGrp = (unsigned)kN1 * 16u * kEs;       // 16 rows of kN1 columns, bytes (P = 8, float2: 32 KiB)
    const unsigned voff = (unsigned)(b * kN1 + c5) * kEs;         // row b, column c5 of pass 0; pass adds 32 samples, row group a 16 rows
    // one input sample: float2 as before; an integer sample's raw bits in .x (.y a constant the compiler drops), widened by iq_widen_bits
    [[maybe_unused]] auto ld_in = [&](__amdgpu_buffer_rsrc_t r, unsigned soff, auto aux) __attribute__((always_inline)) -> cf {
        constexpr int kAux = decltype(aux)::value;                // 0, or 2 = nt (hints bit 1)
        if constexpr (sizeof(TI) == 4) return mk(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, kAux)), 0.f);
        else return mk(__uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, kAux)), 0.f);
    };
    // the first block's rows are requested before the tables are built: their latency hides behind the table set-up
    // P = 2 only (kSplit reads cb from LDS): cbt[n1][b], n1 = 32 pass + c5, from memory, requested a pass ahead into cbA / cbB
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rcb = make_rsrc(cbt, (unsigned)kN1 * 16u * 8u);
    [[maybe_unused]] const unsigned voffc = (unsigned)(c5 * 16 + b) * 8u;
    // two row sets: a pass computes on one while the rows of the next pass arrive in the other (no register copies between passes); kBlkOneSet: LA
    // alone (LB / cbB are never touched there; declared inside the block loop they change the code of the P = 2 forms)
    [[maybe_unused]] cf LA[16], LB[16], cbA = mk(1.f, 0.f), cbB = cbA;   // (kSplit: cbA / cbB stay what they are here and are never read)
    {
        const __amdgpu_buffer_rsrc_t rin = make_rsrc(in + (size_t)first * in_stride, inbytes);
#pragma unroll
        for (int a = 0; a < 16; a++) {
            if constexpr (kIq) LA[a] = ld_in(rin, (unsigned)a * kRowGrp, std::integral_constant<int, 0>{});
            else LA[a] = bld2(rin, voff, (unsigned)a * kRowGrp);
        }
        if constexpr (!kSplit) cbA = bld2(rcb, voffc, 0);
    }
    // ---- tables (once per workgroup; the workgroup is persistent)
    // Offset plans (every channel at f = 256*slot + r, OFF): the block is modulated by exp(-2 pi i r n / N), n = n1 + N1 (16a + b),
    // without a single extra multiplication.  W_16^(r a) rotates the outputs of the first DFT-16 (index p reads Z[(p + r) mod 16]:
    // the exchange slot of register Z[p] becomes (p - r) mod 16), W_256^(r b) joins the forward twiddle (table wrowF), W_N^(r n1)
    // sits in cbt (host), and for odd r the window phase (-1)^block (phase_shifting_windowing_vcc_impl.cc:82, R = 2) in cb.
    float2 *wrowF = OFF ? reinterpret_cast<float2 *>(fdc_smem_blk + GM::kOffWrowF) : wrow;
    const int r16 = roff & 15;
    for (int i = tid; i < 256; i += 512) {
        // entry p of a row sits at index p - 1, entry 0 behind entry 15: the used entries are whole 16-byte pairs (ld_row_sh)
        const int ip = (i >> 4) * 18 + (((i & 15) - 1) & 15);
        wrow[ip] = tw256[((i >> 4) * (i & 15)) & 255];
        if (OFF)     // entry [b][p]: the twiddle of register Z[p], whose true index is pt = (p - r) mod 16: W_256^(b (pt + r))
            wrowF[ip] = tw256[((i >> 4) * ((((i & 15) - r16) & 15) + roff)) & 255];
    }
    for (int i = tid; i < kN1; i += 512) {
        const long long o = slot_off[i];                  // slot i = klo + P khi, khi = k0 + 2 k1, is entry [klo][16 k0 + rev16(k1)]
        soff[(i % P) * 32 + ((i / P) & 1) * 16 + rev16((i / P) >> 1)] = o >= 0 ? (unsigned)((o * nb_call + out_base) * kOs) : 0xFFFFFFFFu;
    }
    for (int i = tid; i < 32 * P; i += 512) ctab[i] = tw256[((i / P) * (i % P) * (8 / P)) & 255];     // [c5][klo] = W_N1^(c5 klo)
    if constexpr (kSplit) {
        for (int i = tid; i < 1024; i += 512) {
            const int ln = i >> 4, q = i & 15, qt = HALF ? q ^ 8 : q;            // HALF: the entries of q ^ 8
            const float2 t = twq[(ln & 3) * 16 + qt];                            // W_N^(16 col q)
            const float s = shn[(ln >> 2) + 16 * qt];
            const float2 e = make_float2(t.x * s, t.y * s), c = cbt[(ln & 3) * 16 + (ln >> 2)];
            LT[ln * 18 + q] = make_float2(e.x * c.x - e.y * c.y, e.x * c.y + e.y * c.x);
        }
        if constexpr (kSrow) {
            for (int i = tid; i < kN1 * 4; i += 512) CBL[i] = cbt[(i >> 4) * 64 + (i & 15)];   // row 4 (i >> 4) of cbt
        } else {
            for (int i = tid; i < kN1 * 4; i += 512) UR[i] = twq[(i >> 4) * 64 + (HALF ? (i & 15) ^ 8 : i & 15)];   // row 4 (i >> 4) of twq
            if (tid < (P + 8) * 16)                                                  // rows 32 pass, then rows 4 wave of cbt
                CBL[tid] = cbt[(tid < P * 16 ? (tid >> 4) * 512 : ((tid >> 4) - P) * 64) + (tid & 15)];
        }
    } else {
        Bt[(tid >> 4) * 18 + (tid & 15)] = twq[HALF ? tid ^ 8 : tid];            // c5 = tid >> 4 < 32, q = tid & 15 (HALF: the entry of q ^ 8)
        for (int i = tid; i < 256 * P; i += 512) {
            const int ps = i >> 8, bb = (i >> 4) & 15, q = i & 15, qt = HALF ? q ^ 8 : q;
            const float2 t = twq[(size_t)(32 * ps) * 16 + qt];                   // W_N^(16 * 32 ps * q)
            const float s = shn[bb + 16 * qt];
            SA[(ps * 16 + bb) * 18 + q] = make_float2(t.x * s, t.y * s);
        }
    }
    __syncthreads();

    float2 *const scrw = scr + w * kStripPts + lane;             // exchange write base: element p at + 68 p
    const float2 *const scrr = scr + w * kStripPts + col + 68 * b;   // exchange read base: element bb at + 4 bb
    const float2 *const wr = wrow + b * 18;
    const float2 *const wrf = wrowF + b * 18;
    // the two table rows of a pass: kSplit: UR row 8 pass + wave and the lane's LT row; P = 2: Bt row c5 and SA row 16 pass + b
    const float2 *const tr0 = kSplit ? UR + w * 16 : Bt + c5 * 18;  // kSplit: + 128 pass
    const float2 *const tr1 = kSplit ? LT + lane * 18 : SA + b * 18;   // P = 2: + 288 pass
    const float2 *const cblr = CBL + b + (kSrow ? 16 * w : 0);      // + 16 pass, + 16 (P + wave); SROW: + 128 pass
    // SROW: row 4 wave of twq as pieces of four entries, at an address the whole wave shares (scalar loads); + 128 pass, + piece
    [[maybe_unused]] const srow_piece *const srow = (const srow_piece *)(unsigned long long)(twq + (kSrow ? 64 * __builtin_amdgcn_readfirstlane(w) : 0));
    const __amdgpu_buffer_rsrc_t rout = make_rsrc(out, out_bytes);
    // FWD / R4: this workgroup's scratch, [pass][j][thread]
    constexpr bool kScr = FWD || R4;
    const __amdgpu_buffer_rsrc_t rscr = make_rsrc(kScr ? fwd_scratch + (size_t)blockIdx.x * 32768 : fwd_scratch, kScr ? 32768u * 8u : 0u);

    // Two waves share a SIMD (waves w and w + 4).  The older one wins the issue arbitration and finishes stage 1 ~10 k cycles
    // earlier; s_setprio (either half favoured, or alternating per pass) changes nothing about that (profiles/r02/NOTES.md).

    for (int m = first; m < nb; m += grid) {
        const int mnext = m + grid < nb ? m + grid : m;
        const float sgn = (OFF && !R4 && (roff & 1) && ((first_block + m) & 1)) ? -1.0f : 1.0f;
        // R = 4 off the grid: the window phase counter (phase_shifting_windowing_vcc_impl.cc:82) is (block * (f mod 4)) mod 4, and phase p of the window
        // table is the window times exp(2 pi i p / 4) = j^p: one constant per block
        cf phs = mk(1.f, 0.f);
        if constexpr (OFF && R4) {
            const int pc = (int)((((first_block + m) & 3) * (roff & 3)) & 3);
            phs = mk(pc == 0 ? 1.f : pc == 2 ? -1.f : 0.f, pc == 1 ? 1.f : pc == 3 ? -1.f : 0.f);
        }
        // G[j][pass]: row t' = b + 16 j, column 32 pass + c5.  One complex value = one 64-bit vector element (two floats packed
        // into an integer): the element index is the pass number at run time, and with 64-bit elements the compiler brackets
        // all sixteen moves of a pass with ONE s_set_gpr_idx_on / off pair (a pair per dword with 32-bit elements).  Integer,
        // not double, elements: bit-casting an extracted double to two floats read element 0 for every pass (seen in the ISA).
        typedef unsigned long long gvec __attribute__((ext_vector_type(P)));
        gvec G[8];
#define FDC_GGET(j, ps) unpack_cf(G[j][ps])
#define FDC_GPUT(j, ps, val) G[j][ps] = pack_cf(val)
        // ---------------- stage 1 ----------------
        // kBlkOneSet: the lane's twiddle row W_256^(b p), p = 1 ... 15, for every pass of this block
        [[maybe_unused]] cf twk[16];
        if constexpr (kOne) ld_row_sh<false>(twk, wr);
        // One pass per trip.  The 16 rows of this lane's column were requested a whole pass ago into L; the rows of the next
        // pass (of this block, or pass 0 of this workgroup's next block; after the last block: the same rows again, unused)
        // are requested first, unconditionally (a conditional request costs a second set of register copies).
        auto one_pass = [&](const int ps, cf (&cur)[16], const cf cbc, cf (&L)[16], cf &cbn) __attribute__((always_inline)) {
            const cf cbl = kSrow ? ld2(&cblr[128 * ps]) : kSplit ? cmul(ld2(&cblr[16 * ps]), ld2(&cblr[16 * (P + w)])) : cbc;
            const cf cb = (OFF && R4) ? cmul(cbl, phs) : OFF ? cbl * sgn : cbl;
            const int pn = ps < P - 1 ? ps + 1 : 0;
            const int mb = ps < P - 1 ? m : mnext;
            // the pass offset (32 columns) sits in the descriptor's base: every pass uses the same per-lane offset and the
            // same 16 scalar row offsets
            const __amdgpu_buffer_rsrc_t rin = make_rsrc(in + (size_t)mb * in_stride + 32 * pn, inbytes);
            // (the forms with a spread twin are launched with hints bit 1 set only; their plain arm stays so that every SPREAD = false form is
            // the code it was: without the branch the pass loop is scheduled and allocated otherwise, profiles/spread_loads/NOTES.md)
            if constexpr (!SPREAD) {
                if constexpr (kIq) {
                    if (hints & 2) {
#pragma unroll
                        for (int a = 0; a < 16; a++) L[a] = ld_in(rin, (unsigned)a * kRowGrp, std::integral_constant<int, 2>{});
                    } else {
#pragma unroll
                        for (int a = 0; a < 16; a++) L[a] = ld_in(rin, (unsigned)a * kRowGrp, std::integral_constant<int, 0>{});
                    }
                } else if (hints & 2) {
#pragma unroll
                    for (int a = 0; a < 16; a++) L[a] = bld2_nt(rin, voff, (unsigned)a * kRowGrp);
                } else {
#pragma unroll
                    for (int a = 0; a < 16; a++) L[a] = bld2(rin, voff, (unsigned)a * kRowGrp);
                }
                if constexpr (!kSplit) cbn = bld2(rcb, voffc, (unsigned)pn * 4096u);
            }
            // SPREAD: rows 4 g ... 4 g + 3 (and cbn at P = 2 with the last of them), behind the first dft16 (14 % of a pass), the middle dft16
            // (39 %), the first inverse dft16 (65 %) and the second exchange (84 %): profiles/spread_loads/NOTES.md.  L is dead from the previous
            // pass's first exchange write on, and this pass's rows are consumed by its first dft16: the waits at the top of a pass cover the
            // previous pass's loads only.  A full scheduling fence in front of a group holds it in its place.
            // kBlkOneSet: L is cur itself, whose rows are dead from this pass's first exchange write on: the first group goes behind that write
            // (22 %), the others are where they were.
            auto ld_rows = [&](auto group) __attribute__((always_inline)) {
                constexpr int g = decltype(group)::value;
                if constexpr (SPREAD) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int a = 4 * g; a < 4 * g + 4; a++) {
                        if constexpr (kIq) L[a] = ld_in(rin, (unsigned)a * kRowGrp, std::integral_constant<int, 0>{});
                        else L[a] = bld2(rin, voff, (unsigned)a * kRowGrp);
                    }
                    if constexpr (!kSplit && g == 3) cbn = bld2(rcb, voffc, (unsigned)pn * 4096u);
                }
            };
            const float2 *const r0 = tr0 + (kSplit ? 128 * ps : 0), *const r1 = tr1 + (kSplit ? 0 : 288 * ps);
            if constexpr (kIq) {
#pragma unroll
                for (int a = 0; a < 16; a++) cur[a] = iq_widen_bits(TI{}, __float_as_uint(cur[a].x), iq_scale);
            }
            // SROW: piece k = entries 4 k ... 4 k + 3 of the wave's row (HALF: of the row with its halves swapped).  Two pieces are requested here, behind
            // the first dft16, the other two into the same registers once the first two are used up: sixteen row SGPRs at most.  A scalar load shares
            // its counter with LDS and returns out of order, so every LDS wait behind a request waits for the pieces too: a request is placed where
            // LDS reads that have to be waited for anyway follow it (here: the forward twiddle row).  A fence in front of a request keeps it from moving
            // up, and from joining the pieces before it (32 row SGPRs live: spills, profiles/stage1_tables/NOTES.md).
            [[maybe_unused]] auto ld_piece = [&](int k) __attribute__((always_inline)) -> u32x8 {
                __builtin_amdgcn_sched_barrier(0);
                return srow[128 * ps + (HALF ? k ^ 2 : k)];
            };
            [[maybe_unused]] u32x8 pc[2];
            dft16<false>(cur);                                    // in place, over a: index p in cur[rev16(p)]
            if constexpr (!kOne) ld_rows(std::integral_constant<int, 0>{});
            if constexpr (kSrow) { pc[0] = ld_piece(0); pc[1] = ld_piece(1); }
            // kBlkOneSet: the twiddle row is the block's (twk, registers), for this use and for the inverse's below; no LDS read here, and the pieces
            // just requested are waited for with the exchange read
            cf tw[16];
            if constexpr (kOne) {
#pragma unroll
                for (int p = 1; p < 16; p++) tw[p] = twk[p];
            } else
                ld_row_sh<OFF>(tw, wrf);
            if constexpr (OFF) {
#pragma unroll
                for (int p = 0; p < 16; p++) st2(&scrw[68 * ((p - r16) & 15)], cmul(cur[rev16(p)], tw[p]));
            } else {
                st2(&scrw[0], cur[rev16(0)]);                     // W256^0 = 1
#pragma unroll
                for (int p = 1; p < 16; p++) st2(&scrw[68 * p], cmul(cur[rev16(p)], tw[p]));
            }
            if constexpr (kOne) ld_rows(std::integral_constant<int, 0>{});   // cur is dead: the next pass's rows 0 ... 3 into it
            __builtin_amdgcn_wave_barrier();                      // same wave, in-order LDS queue: no s_barrier
            cf v[16];
            strip_get(v, scrr);
            if constexpr (FWD) {
                // round-2..5 form: T[k2 = b + 16 q][n1] = A[k2] W_N^(n1 k2) / N.  The half q < 8 stays in the G registers, the half q >= 8 goes to this
                // workgroup's 256 KiB of scratch ([pass][j][thread]: 512-byte wave stores) and comes back for the second run of stage 2
                dft16<false>(v);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const float4 t0 = ld4(&r0[2 * i]), t1 = ld4(&r1[2 * i]);
                    const cf y0 = cmul(cmul(cmul(v[rev16(2 * i)], mk(t0.x, t0.y)), mk(t1.x, t1.y)), cb);
                    const cf y1 = cmul(cmul(cmul(v[rev16(2 * i + 1)], mk(t0.z, t0.w)), mk(t1.z, t1.w)), cb);
                    if (i < 4) { FDC_GPUT(2 * i, ps, y0); FDC_GPUT(2 * i + 1, ps, y1); }
                    else {
                        bst2(rscr, (unsigned)tid * 8u + (unsigned)(2 * i - 8) * 4096u, (unsigned)ps * 32768u, y0);
                        bst2(rscr, (unsigned)tid * 8u + (unsigned)(2 * i - 7) * 4096u, (unsigned)ps * 32768u, y1);
                    }
                }
            } else {
                dft16<false>(v);                                  // A[k2 = b + 16 q] in v[rev16(q)]
                ld_rows(std::integral_constant<int, 1>{});
                cf u[16];
                if constexpr (kSrow) {
                    // A half of the row at a time: its eight multiplications by the row entry (the scalar operand; no LDS), then, for the first half,
                    // the request of the other two pieces into the registers just used, then its eight multiplications by the lane-table entry.  The
                    // waits for the lane table's reads are the first behind the request and cover it: the pieces arrive while those reads do.
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        cf t[8];
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            const u32x8 pj = pc[j >> 2];
                            t[j] = cmul_s(v[rev16(8 * h + j)], mk(__uint_as_float(pj[2 * (j & 3)]), __uint_as_float(pj[2 * (j & 3) + 1])));
                        }
                        if (h == 0) { pc[0] = ld_piece(2); pc[1] = ld_piece(3); }
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const float4 t1 = ld4(&r1[8 * h + 2 * i]);
                            // window * inter-pass twiddle, placed at the ifftshifted position (k2 ^ 128 <=> q ^ 8)
                            u[HALF ? 8 * h + 2 * i : (8 * h + 2 * i) ^ 8] = cmul(t[2 * i], mk(t1.x, t1.y));
                            u[HALF ? 8 * h + 2 * i + 1 : (8 * h + 2 * i + 1) ^ 8] = cmul(t[2 * i + 1], mk(t1.z, t1.w));
                        }
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const float4 t0 = ld4(&r0[2 * i]), t1 = ld4(&r1[2 * i]);
                        // window * inter-pass twiddle, placed at the ifftshifted position (k2 ^ 128 <=> q ^ 8)
                        u[HALF ? 2 * i : (2 * i) ^ 8] = cmul(cmul(v[rev16(2 * i)], mk(t0.x, t0.y)), mk(t1.x, t1.y));
                        u[HALF ? 2 * i + 1 : (2 * i + 1) ^ 8] = cmul(cmul(v[rev16(2 * i + 1)], mk(t0.z, t0.w)), mk(t1.z, t1.w));
                    }
                }
                dft16<true>(u);
                ld_rows(std::integral_constant<int, 2>{});
                if constexpr (!kOne) ld_row_sh<false>(tw, wr);
                u[rev16(0)] = cmul(u[rev16(0)], cb);
#pragma unroll
                for (int p = 1; p < 16; p++) u[rev16(p)] = cmul(cmulc(u[rev16(p)], tw[p]), cb);
                strip_trip(u, scrw, scrr);
                ld_rows(std::integral_constant<int, 3>{});
                dft16<true>(u);                                       // y[t = b + 16 q] in u[rev16(q)]; keep q >= 8 (R = 2)
                // (without the branch that used to open a pass, two passes are one scheduling region: fenced, the G moves stay one s_set_gpr_idx pair)
                if constexpr (SPREAD) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 8; j++) FDC_GPUT(j, ps, u[rev16(8 + j)]);
                if constexpr (SPREAD) __builtin_amdgcn_sched_barrier(0);
                if constexpr (R4) {                                   // R = 4 keeps q >= 4: rows 64..127 go to the scratch, [pass][q - 4][thread]
#pragma unroll
                    for (int j = 0; j < 4; j++) bst2(rscr, (unsigned)tid * 8u + (unsigned)j * 4096u, (unsigned)ps * 16384u, u[rev16(4 + j)]);
                }
            }
        };
        // two passes per trip: the row sets swap roles (the pass count is even for every P).  The offset-plan variant at P = 8 has no
        // registers for the second set's live range (32 bytes of scratch): it copies the rows at the top of a pass as before.
        // kBlkOneSet: every pass computes on LA and loads the next pass's rows into it; the second set's registers hold the twiddle row, read here
        // once per block (not once per workgroup: stage 2 needs the registers — G 128, the prefetched rows 32, its 32 points 64)
        if constexpr (OFF && P == 8) {
#pragma nounroll
            for (int ps = 0; ps < P; ps++) {
                cf cur[16];
#pragma unroll
                for (int a = 0; a < 16; a++) cur[a] = LA[a];
                one_pass(ps, cur, cbA, LA, cbA);
            }
        } else if constexpr (kOne) {
#pragma nounroll
            for (int pp = 0; pp < P; pp += 2) {
                one_pass(pp, LA, cbA, LA, cbA);
                one_pass(pp + 1, LA, cbA, LA, cbA);
            }
        } else {
#pragma nounroll
            for (int pp = 0; pp < P; pp += 2) {
                one_pass(pp, LA, cbA, LB, cbB);
                one_pass(pp + 1, LB, cbB, LA, cbA);
            }
        }
        // ---------------- stage 2 ----------------
        // FFT-N1 over n1 = 32 pass + c5 of every row t' = b + 16 j.  The P passes of a column sit in ONE lane: a DFT-P over
        // the pass index needs no exchange at all (k1 = klo + P khi: W_N1^(n1 k1) = W_P^(pass klo) W_N1^(c5 klo) W_32^(c5 khi)).
        // What is left is a DFT-32 over c5 = 4 wave + col, i.e. across the whole workgroup: ONE trip through LDS per value
        // (trips of 16 kJT rows: [row][klo][c5], rows kLd apart), read back as whole 32-point runs by lane = row (+ 64 for the
        // upper row half when P < 8), klo = wave mod P, transformed in registers.  A wave's store is 64 consecutive samples of one
        // channel (512 B).
        // rowbase: first output row (sample index inside the block's lout rows, or bin offset 128 h of a forward transform) of the
        // run; njc: its number of 16-row groups (8 = the 128 rows in the G registers, 4 = a 64-row run from the scratch)
        auto stage2 = [&](auto get, const int rowbase, auto njc) __attribute__((always_inline)) {
            constexpr int kNJ = decltype(njc)::value;
            constexpr int kNTrip = (kNJ + kJT - 1) / kJT;
            __syncthreads();                                          // every wave is done with its stage-1 scratch
            // the stage-2 roles are worked out here, from a thread index the compiler cannot trace back: loop-invariant address
            // registers would otherwise stay live across stage 1, which has none to spare
            int t2 = tid;
            asm volatile("" : "+v"(t2));
            const int lane2 = t2 & 63, w2 = __builtin_amdgcn_readfirstlane(t2 >> 6), b_2 = lane2 >> 2, c5_2 = 4 * w2 + (lane2 & 3);
            const int klo2 = w2 % P, rh2 = w2 / P;                    // reader: klo, row half (0 for P = 8)
            float2 *const gw0 = scr + b_2 * kLd + c5_2;               // element (row b + 16 jj, klo) at + 16 jj * kLd + 32 klo
            // rows beyond 16 kJB are out of reach of the 16-bit ds offset from gw0: a second base, opaque to the constant folder (it
            // would otherwise materialise one address register per write)
            int rowjb = 16 * kJB * kLd;
            asm volatile("" : "+v"(rowjb));
            float2 *const gw1 = gw0 + rowjb;
            const float2 *const gr = scr + (64 * rh2 + lane2) * kLd + 32 * klo2;   // 32 consecutive points of one row
            const uint4 *const sow = reinterpret_cast<const uint4 *>(soff + 32 * klo2);
#pragma unroll
            for (int tr = 0; tr < kNTrip; tr++) {
                const int ja = kNJ - kJT * tr < kJT ? kNJ - kJT * tr : kJT;   // 16-row groups of this trip (compile time after unrolling)
                cf ct[P];                                             // W_N1^(c5 klo): read per trip, not held across the DFT-32 phase
                {
                    const float2 *ctr = reinterpret_cast<const float2 *>(fdc_smem_blk + GM::kOffCt) + c5_2 * P;
#pragma unroll
                    for (int i = 0; i < P / 2; i++) {
                        const float4 t = ld4(&ctr[2 * i]);
                        ct[2 * i] = mk(t.x, t.y); ct[2 * i + 1] = mk(t.z, t.w);
                    }
                }
                // the values of this trip: register reads, or (runs that come back from the scratch) all loads in flight at once
                cf src[kJT][P];
#pragma unroll
                for (int jj = 0; jj < kJT; jj++)
#pragma unroll
                    for (int ps = 0; ps < P; ps++) if (jj < ja) src[jj][ps] = get(kJT * tr + jj, ps);
#pragma unroll
                for (int jj = 0; jj < kJT; jj++) {
                    if (jj >= ja) continue;
                    cf a[P];
#pragma unroll
                    for (int ps = 0; ps < P; ps++) a[ps] = src[jj][ps];
                    pass_dft<P>(a);
                    float2 *const gw = (jj < kJB ? gw0 : gw1) + (jj % kJB) * 16 * kLd;
                    st2(&gw[0], a[0]);
#pragma unroll
                    for (int k = 1; k < P; k++) st2(&gw[32 * k], cmul(a[pass_idx<P>(k)], ct[k]));
                }
                __builtin_amdgcn_sched_barrier(0);                    // keep the next phase's arithmetic (and its registers) behind
                __syncthreads();                                      // the trip is in LDS
                const bool reads = P == 8 || 4 * rh2 < ja;            // P < 8: waves whose row half the trip does not have sit the phase out
                cf v[32];
                if (reads) {
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        const float4 t = ld4(&gr[2 * i]);
                        v[2 * i] = mk(t.x, t.y); v[2 * i + 1] = mk(t.z, t.w);
                    }
                }
                __syncthreads();                                      // every read of the trip is done: the region may be rewritten
                __builtin_amdgcn_sched_barrier(0);
                if (reads) {
                    dft32<false>(v);                                  // khi = k0 + 2 k1 in v[16 k0 + rev16(k1)]
                    // Stores: slot klo + P khi of row t' = 16 kJT tr + 64 rh + lane.  The 32 stream offsets are the same for the whole
                    // wave (table laid out [klo][register]).  Unused slots: the byte offset is pushed beyond the buffer's extent and the
                    // store is dropped by the range check of the descriptor (no branch per store).
                    // FWD: [block][N bins]
                    const int trow0 = 16 * kJT * tr + 64 * rh2, trow = trow0 + lane2;
                    const unsigned rb = (unsigned)(m * (FWD ? GM::kN : (R4 ? 192 : 128)) + rowbase + trow) * kOs;
                    unsigned mq = FWD ? mqs[((rowbase + trow0) >> 6) & 3] : ~0u;
                    if constexpr (FWD) asm volatile("" : "+s"(mq));   // the 32 scalar terms below are worked out here, not held from block to block
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const uint4 t = sow[q];
                        const unsigned so[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            // FWD: a store nobody reads gets the offset of an unused slot (all ones: a scalar term, one OR per store)
                            const unsigned o = FWD ? (so[e] | (((mq >> (4 * q + e)) & 1u) - 1u)) : so[e];
                            // (integer output: the unused-slot offset 0xFFFFFFF0 lies beyond any narrow extent, which is below 4 GiB too)
                            if constexpr (kOq) {
                                const unsigned u = oq_bits(TO{}, v[4 * q + e], oq_scale);
                                if constexpr (kOs == 4) __builtin_amdgcn_raw_buffer_store_b32(u, rout, (o == 0xFFFFFFFFu ? 0xFFFFFFF0u : o + rb), 0, NT ? 2 : 0);
                                else __builtin_amdgcn_raw_buffer_store_b16((unsigned short)u, rout, (o == 0xFFFFFFFFu ? 0xFFFFFFF0u : o + rb), 0, NT ? 2 : 0);
                            } else
                                bst2t<NT>(rout, (o == 0xFFFFFFFFu ? 0xFFFFFFF0u : o + rb), v[4 * q + e]);
                        }
                    }
                    if constexpr (FWD) {
                        // Power of every 16-bin group of the spectrum while it is in the registers (round 6: what the sinks' power cells are summed from —
                        // k_cell_power used to read the whole spectrum back, 444-472 MB per 1024 blocks).  This lane holds bins 256 slot + k2 of 32
                        // slots, its row of 16 lanes is one 16-bin group of each: 32 sums over 16 lanes as ONE transposed reduction — every step
                        // halves the registers and pairs the lanes of one bit (bits 3 and 2 of the lane: DPP row rotations / shifts whose bank mask
                        // picks which half of the lanes writes; bits 1 and 0: quad permutations) — 66 additions instead of 128, and lane j of the
                        // row ends with the sums of registers 2 j and 2 j + 1.
                        if (gpow) {
                            float t16[16];
#pragma unroll
                            for (int i = 0; i < 16; i++) {
                                const float s0 = __builtin_fmaf(v[i].y, v[i].y, v[i].x * v[i].x);
                                const float s1 = __builtin_fmaf(v[i + 16].y, v[i + 16].y, v[i + 16].x * v[i + 16].x);
                                // (s_nop 1: a DPP operand written by the VALU instruction just before needs two wait states; the compiler's hazard
                                // recogniser does not look into inline assembly)
                                asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                                    "v_add_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xc" : "=&v"(t16[i]) : "v"(s0), "v"(s1));
                            }
                            float t8[8];
#pragma unroll
                            for (int i = 0; i < 8; i++)
                                asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                                    "v_add_f32_dpp %0, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa" : "=&v"(t8[i]) : "v"(t16[i]), "v"(t16[i + 8]));
                            const bool b1 = (lane2 & 2) != 0, b0 = (lane2 & 1) != 0;
                            float t4[4], t2[2];
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                const float keepv = b1 ? t8[i + 4] : t8[i], send = b1 ? t8[i] : t8[i + 4];
                                t4[i] = keepv + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0x4E /* quad_perm [2,3,0,1] */, 0xF, 0xF, false));
                            }
#pragma unroll
                            for (int i = 0; i < 2; i++) {
                                const float keepv = b0 ? t4[i + 2] : t4[i], send = b0 ? t4[i] : t4[i + 2];
                                t2[i] = keepv + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, false));
                            }
                            // Lane (row g, j) now holds the sums of registers 2 j, 2 j + 1 over row g = group g of this trip's four.  Stored from there a
                            // wave's 128 values would be 128 separate 4-byte write requests (the four groups of a slot sit in four different rows of the
                            // wave; measured: + 31 us per 896 blocks, the request rate, not the bytes).  One hop through the LDS crossbar (ds_bpermute: no
                            // LDS memory) first: lane (rho, i) takes register R = 8 rho + (i >> 1), groups 2 (i & 1) and + 1, so that two NEIGHBOURING lanes
                            // write the 16 contiguous bytes of a slot's four groups: 32 requests per wave and trip.
                            const int i16 = lane2 & 15, rho = lane2 >> 4, gsrc = 2 * (i16 & 1);
                            const int a0 = (16 * gsrc + 4 * rho + (i16 >> 2)) * 4, a1 = a0 + 64;
                            const int z0 = __builtin_bit_cast(int, t2[0]), z1 = __builtin_bit_cast(int, t2[1]);
                            const int f0a = __builtin_amdgcn_ds_bpermute(a0, z0), f0b = __builtin_amdgcn_ds_bpermute(a0, z1);
                            const int f1a = __builtin_amdgcn_ds_bpermute(a1, z0), f1b = __builtin_amdgcn_ds_bpermute(a1, z1);
                            const bool odd = (i16 & 2) != 0;                      // R & 1: which of the source lane's two registers
                            float2 pr;
                            pr.x = __builtin_bit_cast(float, odd ? f0b : f0a);
                            pr.y = __builtin_bit_cast(float, odd ? f1b : f1a);
                            // register R -> slot (soff is laid out [klo][register]: register R is khi = (R >> 4) + 2 rev16(R & 15), slot klo + P khi);
                            // gpow is [block][slot][16 groups of the slot's 256 bins]
                            const int reg = 8 * rho + (i16 >> 1), slot = klo2 + P * ((reg >> 4) + 2 * (4 * (reg & 3) + ((reg & 15) >> 2)));
                            *reinterpret_cast<float2 *>(gpow + (size_t)m * (GM::kN / 16) + 16 * slot + (rowbase + trow0) / 16 + gsrc) = pr;
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        stage2([&](int j, int ps) { return FDC_GGET(j, ps); }, R4 ? 64 : 0, std::integral_constant<int, 8>{});
        if constexpr (FWD) {
            // second half of k2: the values stage 1 put aside are this lane's own stores; sc1 loads are served by the L2
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            stage2([&](int j, int ps) { return bld2_sc1(rscr, (unsigned)tid * 8u + (unsigned)(j * 4096 + ps * 32768), 0u); }, 128,
                   std::integral_constant<int, 8>{});
        }
        if constexpr (R4) {
            // rows 64..127 of the inverse transforms = output rows 0..63: this lane's own stores, served by the L2
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            stage2([&](int j, int ps) { return bld2_sc1(rscr, (unsigned)tid * 8u + (unsigned)(j * 4096 + ps * 16384), 0u); }, 0,
                   std::integral_constant<int, 4>{});
        }
        // the trip region (= stage-1 scratch) was last read before the barrier above: the next block starts without one
    }
}

// Which forms of k_blk256 exist, stated ONCE.  Integer output: streamed (nt) stores only — a handle with FDC_PIPE_PLAIN_STORES narrows behind the float form
// instead (half the instantiations) — and at P = 8 no R = 4 form on float input: the narrowing costs the 256-register kernel 2-3 spilled registers, so those
// plans narrow behind the float form too (fdc_enqueue.hip oq_fused).  The half-slot form is a variant of the on-grid channelizer; the forward transform is
// float2 to float2, on the grid, nothing else; a spread twin where kBlkSpread says so.
template <int P, bool NT, bool OFF, bool FWD, bool R4, bool HALF, class TI, class TO, bool SPREAD>
constexpr bool blk256_form()
{
    constexpr bool kIq = !std::is_same<TI, float2>::value, kOq = !std::is_same<TO, float2>::value;
    constexpr bool kOqR4Narrowed = P == 8 && R4 && !kIq && kOq;
    return (!kOq || NT) && !kOqR4Narrowed && !(HALF && OFF) && (!FWD || !(kIq || kOq || OFF || R4 || HALF)) && (!SPREAD || kBlkSpread<P, OFF, FWD, R4, TO>);
}

// f(kernel, LDS bytes, TI{}, TO{}) for the forms that match (fdc_forms.hpp; kEvery: every value of that argument).  spread = 1: the spread twin of a form
// that has one, the form itself otherwise; 0: the form with all sixteen row loads at the top of a pass
template <class F>
static void for_blk256_forms(int p, int nt, int off, int fwd, int r4, int half, int ifmt, int ofmt, int spread, F &&f)
{
    auto form = [&](auto P, auto NT, auto OFF, auto FWD, auto R4, auto HALF, auto ti, auto to) {
        using TI = decltype(ti);
        using TO = decltype(to);
        constexpr bool kNt = NT() != 0, kOff = OFF() != 0, kFwd = FWD() != 0, kR4 = R4() != 0, kHalf = HALF() != 0;
        constexpr bool kSrow = kBlkSrow<P(), kOff, kFwd, kR4>;      // (never an offset plan)
        constexpr int kLds = kOff ? BlkGeom<P()>::kLdsOff : BlkGeom<P(), kSrow>::kLds;
        if constexpr (blk256_form<P(), kNt, kOff, kFwd, kR4, kHalf, TI, TO, false>()) {
            constexpr bool kTwin = blk256_form<P(), kNt, kOff, kFwd, kR4, kHalf, TI, TO, true>();
            if (spread != 1 || !kTwin) f(k_blk256<P(), kNt, kOff, kFwd, kR4, kHalf, TI, TO, false>, kLds, ti, to);
            if constexpr (kTwin)
                if (spread != 0) f(k_blk256<P(), kNt, kOff, kFwd, kR4, kHalf, TI, TO, true>, kLds, ti, to);
        }
    };
    for_values<2, 4, 8>(p, [&](auto P) { for_values<1, 0>(nt, [&](auto NT) { for_values<0, 1>(off, [&](auto OFF) { for_values<0, 1>(fwd, [&](auto FWD) {
        for_values<0, 1>(r4, [&](auto R4) { for_values<0, 1>(half, [&](auto HALF) {
            for_samples(ifmt, [&](auto ti) { for_samples(ofmt, [&](auto to) { form(P, NT, OFF, FWD, R4, HALF, ti, to); }); });
        }); });
    }); }); }); });
}

hipError_t init_block_kernels()
{
    hipError_t e = hipSuccess;
    for_blk256_forms(kEvery, kEvery, kEvery, kEvery, kEvery, kEvery, kEvery, kEvery, kEvery, [&](auto k, int lds, auto, auto) {
        if (e == hipSuccess) e = set_block_lds(reinterpret_cast<const void *>(k), lds);
    });
    return e;
}

bool poly_block_supports(int N) { return N == 16384 || N == 32768 || N == 65536; }

hipError_t launch_poly_block(const BlockLaunch &b)
{
    if (b.nb_chunk <= 0) return hipSuccess;
    const bool r4 = b.R == 4, halfslot = b.half();         // half a slot: the on-grid kernel with its tables moved (HALF), R = 2 and 4
    if (b.L != 256 || b.r < 0 || b.r >= 256 || !poly_block_supports(b.N) || (b.R != 2 && !r4) || (r4 && !b.scratch)) return hipErrorInvalidValue;
    if (b.ifmt == kEvery || b.ofmt == kEvery) return hipErrorInvalidValue;      // a launch names one form
    // one 512-thread workgroup per CU (LDS: up to 159.5 KiB each).  N = 16384 on the grid at R = 2: 126 registers and 79.75 KiB of LDS per
    // workgroup: two workgroups per CU, one's stage 2 beside the other's stage 1
    const int grid = b.grid(b.N == 16384 && b.R == 2 && (!b.r || halfslot) ? 2 : 1);
    // output samples are written once and never read back here: streamed (nt) stores, measured 0.186 -> 0.172 ms (hints bit 0)
    // ev_start / ev_stop (timing): the dispatch packet's own begin / end time stamps (hipExtLaunchKernel) — no barrier packet
    // in front of or behind the kernel, unlike hipEventRecord (measured 7-17 us per bracketed launch)
    // R = 4: three quarters of every inverse transform kept: 192 rows per block, 64 of them via the scratch
    // streamed input loads (hints bit 1, a diagnostic): the forms with all sixteen row loads at the top of a pass
    hipError_t e = hipErrorInvalidValue;                        // stays if no form matches
    for_blk256_forms(b.N / 8192, b.hints & 1, !halfslot && b.r, 0, r4, halfslot, b.ifmt, b.ofmt, !(b.hints & 2), [&](auto k, int lds, auto ti, auto to) {
        using TI = decltype(ti);
        using TO = decltype(to);
        hipExtLaunchKernelGGL(k, dim3((unsigned)grid), dim3(512), lds, b.s, b.ev_start, b.ev_stop, 0u, static_cast<const TI *>(b.in), b.in_stride,
                              static_cast<TO *>(b.out), b.tw256, b.twq, b.cbt, b.shn, b.slot_off, (long long)b.mbase * (r4 ? 192 : 128), (long long)b.nb_call,
                              b.out_bytes, b.nb_chunk, b.hints, (unsigned long long *)nullptr, halfslot ? 0 : b.r, b.first_block,
                              r4 ? b.scratch : (float2 *)nullptr, (const unsigned *)nullptr, iq_tail<TI, TO>(nullptr, b.iscale, b.oscale));
        e = hipGetLastError();
    });
    return e;
}

// Forward transform of nitems blocks of 65536 samples (item m at in + m*in_stride) into the shifted, 1/N-scaled spectrum
// out[m][N] with the block kernel (N = 16384 / 32768 / 65536: k_blk256<P, ..., FWD>).  slot_off[c] = 256 c, c < N / 256; shn1[k2] = 1/N; cbt0 = the r = 0 table.
// ev: null or 3 events: start and end of the kernel (dispatch stamps), and an event recorded behind it (the 3-event protocol
// of the two-pass transform: its second interval is empty here).
hipError_t launch_block_fft(int N, const float2 *in, size_t in_stride, float2 *out, int nitems, const float2 *tw256,
                            const float2 *twq, const float2 *cbt0, const float *shn1, const long long *slot_off,
                            float2 *scratch /* ncu x 32768 points */, int ncu, int hints, hipStream_t s, hipEvent_t *ev,
                            const unsigned *keep, float *gpow /* null, or nitems x N/16 floats: the power of every 16-bin group of the spectrum */)
{
    if (!poly_block_supports(N)) return hipErrorInvalidValue;
    const int per = (int)(((size_t)1 << 28) / (size_t)N);  // 32-bit byte offsets inside one launch: at most 2 GiB of spectrum (N = 65536: 4096 blocks)
    for (int m0 = 0; m0 < nitems; m0 += per) {
        const int nb = nitems - m0 < per ? nitems - m0 : per;
        int grid = ncu > 0 ? ncu : 256;
        if (grid > nb) grid = nb;
        hipEvent_t e0 = ev && m0 == 0 ? ev[0] : nullptr, e2 = ev && m0 + nb >= nitems ? ev[1] : nullptr;
        hipError_t e = hipErrorInvalidValue;
        for_blk256_forms(N / 8192, hints & 1, 0, 1, 0, 0, kIqFloat, kIqFloat, 0, [&](auto k, int lds, auto ti, auto to) {
            if constexpr (std::is_same<decltype(ti), float2>::value && std::is_same<decltype(to), float2>::value) {
                hipExtLaunchKernelGGL(k, dim3((unsigned)grid), dim3(512), lds, s, e0, e2, 0u, in + (size_t)m0 * in_stride, in_stride, out + (size_t)m0 * (size_t)N,
                                      tw256, twq, cbt0, shn1, slot_off, 0ll, 1ll, (unsigned)((size_t)nb * (size_t)N * 8), nb, hints,
                                      (unsigned long long *)nullptr, 0, 0ll, scratch, keep, gpow ? gpow + (size_t)m0 * (size_t)(N / 16) : (float *)nullptr);
                e = hipGetLastError();
            }
        });
        if (e != hipSuccess) return e;
    }
    if (ev) { hipError_t e = hipEventRecord(ev[2], s); if (e != hipSuccess) return e; }
    return hipGetLastError();
}

}  // namespace fdc
