// fdc_pipeline_create in four steps (round 5; it was one 530-line function): validate -> channel records -> classify_plan (which kernels
// run the plan: banks, remainder, or the spectrum path; the cost rule and nothing else decides) -> device tables and scratch.
#include "fdc_pipeline.hpp"

#include <map>
#include <tuple>

namespace fdc { namespace pipe {

// ---- step 1: the arguments (the reference constructors' predicates among them)
int validate_cfg(const fdc_pipeline_cfg *cfg)
{
    const int N = cfg->blocklen, R = cfg->relinvovl;
    if (!ispow2(N) || N < 2) return set_error(FDC_ERR_INVALID_ARGUMENT, "blocklen %d must be a power of two >= 2", N);
    if (!ispow2(R) || R < 2 || R > N) return set_error(FDC_ERR_INVALID_ARGUMENT, "relinvovl %d must be a power of two in [2, blocklen]", R);
    if (N > (1 << 24)) return set_error(FDC_ERR_UNSUPPORTED, "blocklen %d above 2^24", N);
    if (cfg->nchannels < 0 || (cfg->nchannels > 0 && !cfg->channels)) return set_error(FDC_ERR_INVALID_ARGUMENT, "bad channel list");
    if (cfg->max_blocks < 1) return set_error(FDC_ERR_INVALID_ARGUMENT, "max_blocks must be >= 1");
    for (int c = 0; c < cfg->nchannels; c++) {
        const fdc_channel &ch = cfg->channels[c];
        if (!ispow2(ch.l) || ch.l > N) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel %d: l=%d must be a power of two <= blocklen", c, ch.l);
        if (ch.f < 0 || ch.f + ch.l > N) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel %d: slice [%d,%d) outside the spectrum", c, ch.f, ch.f + ch.l);
        // predicates of phase_shifting_windowing_vcc_impl ctor (lib/phase_shifting_windowing_vcc_impl.cc:46-53)
        if (ch.passbw <= 0.0f) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel %d: PassBw must not be <= 0", c);
        if (ch.stopbw <= 0.0f) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel %d: StopBw must not be <= 0", c);
        if (ch.stopbw < ch.passbw) return set_error(FDC_ERR_INVALID_ARGUMENT, "channel %d: StopBw must not be < PassBw", c);
    }
    // several kernels address a call's output with 32-bit byte offsets (buffer descriptors; offsets from 0xFFFFFFF0 up mean "no store"):
    // one call produces less than 4 GiB.  A stream is cut into more calls, not bigger ones.
    int64_t per_block = 0;
    for (int c = 0; c < cfg->nchannels; c++) per_block += cfg->channels[c].l - cfg->channels[c].l / R;
    if (per_block * 8 * (int64_t)cfg->max_blocks > 0xFFFFF000ll)
        return set_error(FDC_ERR_INVALID_ARGUMENT, "max_blocks %d x %lld output samples per block is more than the 4 GiB one call may produce (at most %lld blocks per call for this plan)",
                    cfg->max_blocks, (long long)per_block, (long long)(0xFFFFF000ll / (per_block * 8)));
    return FDC_OK;
}

// ---- step 2: channel records, de-duplicated window tables, the channels by width
void group_by_width(const fdc_pipeline *p, const std::vector<int> *ids, std::vector<std::pair<int, std::vector<int32_t>>> &groups,
                    std::vector<size_t> &off, std::vector<char> &al, std::vector<char> &oal, std::vector<int32_t> &flat)
{
    std::map<int, std::vector<int32_t>> bylen;
    if (ids) for (int c : *ids) bylen[p->chans[(size_t)c].l].push_back(c);
    else for (int c = 0; c < p->C; c++) bylen[p->chans[(size_t)c].l].push_back(c);
    for (auto &kv : bylen) {
        bool a = true, o = true;
        for (int c : kv.second) {
            if (p->chans[(size_t)c].f & 1) a = false;
            if ((p->chans[(size_t)c].out_off & 1) || (p->chans[(size_t)c].lout & 1)) o = false;
        }
        al.push_back(a); oal.push_back(o);
        off.push_back(flat.size());
        groups.emplace_back(kv.first, kv.second);
        flat.insert(flat.end(), kv.second.begin(), kv.second.end());
    }
}

void build_channel_records(fdc_pipeline *p, const fdc_pipeline_cfg *cfg, std::vector<std::complex<float>> &pool)
{
    std::map<std::tuple<int, float, float>, int> winmap;
    int64_t off = 0;
    for (int c = 0; c < p->C; c++) {
        const fdc_channel &ch = cfg->channels[c];
        fdc::ChanDev d{};
        d.f = ch.f; d.l = ch.l; d.lout = ch.l - ch.l / p->R;
        d.shift = ((ch.f % p->R) + p->R) % p->R;
        d.out_off = off; off += d.lout;
        auto key = std::make_tuple(ch.l, ch.passbw, ch.stopbw);
        auto it = winmap.find(key);
        if (it == winmap.end()) {
            const int o = (int)pool.size();
            pool.resize(pool.size() + (size_t)p->R * ch.l);
            fdc::window_table(cfg->windowtype, ch.l, ch.passbw, ch.stopbw, p->R, 1, false, pool.data() + o);
            it = winmap.emplace(key, o).first;
        }
        d.win_off = it->second;
        p->chans.push_back(d);
    }
    p->sum_lout = off;
}

// ---- step 3: which kernels run the plan
// the block kernel that takes a bank of l-bin channels at f = l slot + r, if there is one for this block length and overlap
static bool bank_has_block_kernel(int N, int R, int L, int r, int flags)
{
    if ((flags & FDC_PIPE_NO_BLOCK) || (R != 2 && R != 4)) return false;
    switch (L) {
    case 256: return fdc::poly_block_supports(N);                                    // k_blk256: N = 16384 / 32768 / 65536, any r
    case 512: return fdc::poly_block512_supports(N, R) && (r == 0 || r == L / 2);   // k_blk512<P>: N = 16384 / 32768 / 65536; on the grid or half a channel off it
    case 1024: return fdc::poly_block1024_supports(N, R) && (r == 0 || r == L / 2); // k_blk1024<P>: the same
    case 128: case 64: return fdc::poly_block_narrow_supports(N, L, R) && r % (L / 4) == 0;   // k_blknar: quarters of a channel
    default: return false;
    }
}

// N = 4096: the whole plan as ONE launch (fdc_fused4096.hip) when every channel is 16 ... 1024 bins wide.  A workgroup takes T blocks (T = 1 where no channel
// is wider than 256 bins, else 2); its rows — (block of the workgroup, channel) — go to its 4 T waves, one width per wave: two rows of 1024 bins, four of 512,
// eight of 256 or less; their exchange areas must fit the T tiles the spectra leave behind.  Always true for plans of 256-bin and wider channels of up to 4096
// bins in total; plans of channels that overlap to more (or of more than 32 narrow channels) stay on the spectrum path.
struct F4Class { int l, cls, per_wave, pitch; };
constexpr F4Class kF4Classes[] = {{1024, 4, 2, 1056}, {512, 3, 4, 513}, {128, 5, 8, 136}, {64, 6, 8, 68}, {32, 7, 8, 34}, {16, 8, 8, 17}};   // (256: below; pitches: rows of a half-wave on different banks)
static bool plan_fused4096(fdc_pipeline *p, const fdc_pipeline_cfg *cfg, int flags)
{
    for (auto &w : p->f4_wave) w.clear();
    p->f4_cls = 0;
    p->f4_teams = 2;
    if (p->N != 4096 || p->C == 0 || p->cfg_generic || (flags & (FDC_PIPE_NO_POLY | FDC_PIPE_NO_FUSED))) return false;
    long long bins = 0;
    bool wide = false;
    for (int c = 0; c < p->C; c++) {
        const int l = cfg->channels[c].l;
        if (l < 16 || l > 1024 || (l & (l - 1)) || l % p->R) return false;
        bins += l;
        wide = wide || l >= 512;
    }
    // ONE 256-bin channel: the two launches are as fast or a little faster (0.060 - 0.063 against 0.064 ms per 8192 blocks; four such channels: 0.075 / 0.064;
    // everything wider: 1.3 - 2.8 x for this form, profiles/r06/plan_choice_4096.txt) — the forward transform alone is what both cost
    if (bins < 512 && !(flags & FDC_PIPE_WIDE_UNIFORM)) return false;
    // the schedule for T blocks per workgroup (4 T waves, T tiles): rows by width, the blocks' rows of a channel side by side
    auto schedule = [&](int T) {
        for (auto &w : p->f4_wave) w.clear();
        std::map<int, std::vector<int>> by;
        for (int c = 0; c < p->C; c++) for (int k = 0; k < T; k++) by[cfg->channels[c].l].push_back(2 * c + k);
        int w = 0;
        unsigned cls = 0;
        long long pts = 272ll * (long long)by[256].size();
        for (const F4Class &k : kF4Classes) {
            const std::vector<int> &rows = by[k.l];
            pts += (long long)k.pitch * (long long)rows.size();
            for (size_t i = 0; i < rows.size(); i += (size_t)k.per_wave, w++) {
                if (w >= 4 * T) return false;
                for (size_t j = i; j < std::min(i + (size_t)k.per_wave, rows.size()); j++) p->f4_wave[w].push_back(rows[j]);
                cls |= (unsigned)k.cls << (4 * w);
            }
        }
        const int avail = 4 * T - w, n256 = (int)by[256].size();
        if (n256 > 8 * avail || pts > (long long)T * fdc::fused4096_tile_points()) return false;
        if (n256) {
            // as few waves as one set of four rows each allows (a wave's instructions cost the same for one row as for four); two sets where that is not enough
            const int nw = n256 <= 4 * avail ? (n256 + 3) / 4 : avail;
            for (int i = 0; i < n256; i++) p->f4_wave[w + i % nw].push_back(by[256][(size_t)i]);
            for (int k = 0; k < nw; k++) cls |= (p->f4_wave[w + k].size() > 4 ? 2u : 1u) << (4 * (w + k));
        }
        p->f4_cls = cls;
        p->f4_teams = T;
        return true;
    };
    // one block per workgroup (four independent workgroups on a unit) where no row is wide; else, or where that does not fit, a pair of blocks
    static const int teams_env = [] { const char *e = fdc::debug_env("FDC_F4_TEAMS"); return e ? atoi(e) : 0; }();
    if ((!wide || teams_env == 1) && teams_env != 2 && schedule(1)) return true;
    if (schedule(2)) return true;
    for (auto &w : p->f4_wave) w.clear();
    p->f4_cls = 0;
    return false;
}

void classify_plan(fdc_pipeline *p, const fdc_pipeline_cfg *cfg, int flags)
{
    const int N = p->N, R = p->R, C = p->C;
    // the spectrum path's forward transform is the block kernel at N = 16384 / 32768 / 65536 (fdc_pipeline_path() = 1; decided here so that
    // fdc_pipeline_plan_preview says what create does)
    p->fwd_block = fdc::poly_block_supports(N) && !p->cfg_generic && !(flags & FDC_PIPE_NO_BLOCK);
    p->banks.clear(); p->bank_alias.clear(); p->rem.clear();
    p->poly_ok = p->poly_block = p->split = false;
    p->fused = plan_fused4096(p, cfg, flags);
    if (p->fused) return;
    if (C == 0 || p->cfg_generic || (flags & FDC_PIPE_NO_POLY) || N > (1 << 20) || R > 16) return;
    auto same_window = [&](const fdc_pipeline::Bank &b, const fdc_channel &ch) { return b.passbw == ch.passbw && b.stopbw == ch.stopbw; };

    // (a) every channel whose width has a block kernel at its offset joins the bank of its (width, offset, window); a slice that is
    //     already in its bank (the reference's parameter derivation clamps a wrapped channel onto its neighbour's place) is computed
    //     once and copied; everything else is the remainder
    std::vector<fdc_pipeline::Bank> banks;
    std::vector<std::vector<char>> used;
    std::vector<std::pair<int, int>> alias;
    std::vector<int> rem;
    for (int c = 0; c < C; c++) {
        const fdc_channel &ch = cfg->channels[c];
        const int L = ch.l, r = ch.f % L;
        if (!bank_has_block_kernel(N, R, L, r, flags)) { rem.push_back(c); continue; }
        size_t k = 0;
        for (; k < banks.size(); k++) if (banks[k].L == L && banks[k].r == r && same_window(banks[k], ch)) break;
        if (k == banks.size()) {
            fdc_pipeline::Bank b;
            b.L = L; b.r = r; b.passbw = ch.passbw; b.stopbw = ch.stopbw;
            banks.push_back(std::move(b));
            used.emplace_back((size_t)(N / L) + 1, 0);
        }
        if (used[k][(size_t)(ch.f / L)]) {
            int first = -1;
            for (int c0 : banks[k].chan) if (cfg->channels[c0].f == ch.f) { first = c0; break; }
            alias.emplace_back(c, first);
            continue;
        }
        used[k][(size_t)(ch.f / L)] = 1;
        banks[k].chan.push_back(c);
    }

    // (b) no block kernel anywhere (another block length or overlap, FDC_PIPE_NO_BLOCK): the two-launch forms take a plan that is ONE
    //     bank on its grid, every slot at most once.  l = 256: k_p1 + k_p2 / k_p2k / k_p2g (4096 <= N <= 2^20); other widths on the generic
    //     LDS core, which measured faster than the spectrum path for l = 128 only (profiles/r04/NOTES.md section 6) — FDC_PIPE_WIDE_UNIFORM
    //     takes it for every width
    if (banks.empty()) {
        const int L = cfg->channels[0].l;
        const bool fits = L == 256 ? N >= 4096
                                   : (L >= 64 && L <= 4096 && L / R >= 1 && N / L >= 16 && N / L <= 4096 && (L == 128 || (flags & FDC_PIPE_WIDE_UNIFORM)));
        if (!fits) return;
        fdc_pipeline::Bank b;
        b.L = L; b.r = 0; b.passbw = cfg->channels[0].passbw; b.stopbw = cfg->channels[0].stopbw;
        std::vector<char> u((size_t)(N / L) + 1, 0);
        for (int c = 0; c < C; c++) {
            const fdc_channel &ch = cfg->channels[c];
            if (ch.l != L || ch.f % L || !same_window(b, ch) || u[(size_t)(ch.f / L)]) return;
            u[(size_t)(ch.f / L)] = 1;
            b.chan.push_back(c);
        }
        p->banks.push_back(std::move(b));
        p->poly_ok = true;
        return;
    }

    // (c) the cost rule (fdc_plan_cost.hpp; the numbers are measured at N = 65536, where the remainder of a split plan has its forward
    //     kernel).  Banks go back to the remainder, cheapest plan first, while that lowers the sum; then the sum must beat the whole plan on
    //     the spectrum path.  Other block lengths (banks of 256-bin channels only): no remainder, no more than kMaxBanks launches.
    // (round 5: the forward variant of the block kernel exists at N = 16384 / 32768 too; per block everything costs N / 65536 of the table's
    // numbers there, on both sides of every comparison)
    const bool may_split = p->fwd_block;
    auto band = [&](const std::vector<int> &ids) { double b = 0; for (int c : ids) b += cfg->channels[c].l; return b / double(N); };
    auto move_to_rem = [&](size_t k) {
        rem.insert(rem.end(), banks[k].chan.begin(), banks[k].chan.end());
        for (size_t i = 0; i < alias.size();) {                   // copies of a channel that is no longer computed by a bank are channels again
            if (std::find(banks[k].chan.begin(), banks[k].chan.end(), alias[i].second) != banks[k].chan.end()) {
                rem.push_back(alias[i].first);
                alias.erase(alias.begin() + (long)i);
            } else i++;
        }
        banks.erase(banks.begin() + (long)k);
    };
    if (!may_split) {
        if (!rem.empty() || (int)banks.size() > fdc::cost::kMaxBanks) return;
    } else {
        auto total = [&](const std::vector<fdc_pipeline::Bank> &bs, double remband) {
            double t = fdc::cost::spectrum_path(remband);
            for (const auto &b : bs) t += fdc::cost::bank_launch(b.L);
            return t;
        };
        const bool forced = (flags & FDC_PIPE_WIDE_UNIFORM) != 0;              // every bank keeps its block kernel, whatever the rule says (A/B, tests)
        for (;;) {
            if (banks.empty()) break;
            const bool too_many = (int)banks.size() > fdc::cost::kMaxBanks;
            if (forced && !too_many) break;
            const double now = total(banks, band(rem));
            size_t best = banks.size();
            double best_t = too_many ? 1e30 : now;
            for (size_t k = 0; k < banks.size(); k++) {
                std::vector<int> r2(rem);
                r2.insert(r2.end(), banks[k].chan.begin(), banks[k].chan.end());
                for (const auto &al : alias) if (std::find(banks[k].chan.begin(), banks[k].chan.end(), al.second) != banks[k].chan.end()) r2.push_back(al.first);
                double t = fdc::cost::spectrum_path(band(r2));
                for (size_t j = 0; j < banks.size(); j++) if (j != k) t += fdc::cost::bank_launch(banks[j].L);
                if (t < best_t) { best_t = t; best = k; }
            }
            if (best == banks.size()) break;
            move_to_rem(best);
        }
        if (banks.empty()) return;                                            // the spectrum path
        if (!forced) {
            std::vector<int> all(C);
            for (int c = 0; c < C; c++) all[(size_t)c] = c;
            if (total(banks, band(rem)) >= fdc::cost::spectrum_path(band(all))) return;
        }
    }
    // the biggest bank first (what the timing events and the description call bank 1)
    std::stable_sort(banks.begin(), banks.end(), [](const fdc_pipeline::Bank &x, const fdc_pipeline::Bank &y) { return x.chan.size() > y.chan.size(); });
    std::sort(rem.begin(), rem.end());
    p->banks = std::move(banks);
    p->bank_alias = std::move(alias);
    p->rem = std::move(rem);
    p->split = !p->rem.empty();
    p->poly_ok = p->poly_block = true;
}

// ---- step 4a: the tables of one bank (window, slot table, per-column constants of its width's kernel)
static int build_bank_tables(fdc_pipeline *p, const fdc_pipeline_cfg *cfg, fdc_pipeline::Bank &bk)
{
    const int N = p->N, L = bk.L, N1 = N / L, rb = bk.r;
    std::vector<std::complex<float>> shape((size_t)L);
    fdc::window_table(cfg->windowtype, L, bk.passbw, bk.stopbw, 1, 0, true, shape.data());     // plateau 1: the chain's * l is in it
    std::vector<float> sn((size_t)L);
    for (int k2 = 0; k2 < L; k2++) sn[(size_t)k2] = float(double(shape[(size_t)k2].real()) / double(N));
    std::vector<long long> so((size_t)N1, -1);
    for (int c : bk.chan) so[(size_t)(p->chans[(size_t)c].f / L)] = p->chans[(size_t)c].out_off;
    CHK_DEV(bk.d_slot_off.upload(so));
    std::vector<float2> cb;
    if (L == 256) {
        // (-1)^n1 W_N^(n1 (b + r)): an offset tiling is the on-grid plan of the block modulated by exp(-2 pi i r n / N)
        cb.resize((size_t)N1 * 16);
        for (int n1 = 0; n1 < N1; n1++)
            for (int j = 0; j < 16; j++) {
                const float2 w = unit(double(((long long)n1 * (j + rb)) % N) / double(N));
                const float sg = (n1 & 1) ? -1.0f : 1.0f;
                cb[(size_t)n1 * 16 + j] = make_float2(sg * w.x, sg * w.y);
            }
    } else if ((L == 512 || L == 1024) && p->poly_block) {
        // (-1)^n1 W_N^(n1 (b + 256 i)) at [n1][b + 16 i], i = half (512: two) or quarter (1024: four) of k2.  Half a channel off the grid: the lane
        // of part i holds part i ^ (parts / 2) of the modulated column, whose constant W_N^((l/2) n1) joins the table, and the kernels read the window
        // with its halves swapped
        const bool half = rb == L / 2;
        const int parts = L / 256;
        if (half) {
            std::vector<float> snd(sn);
            for (int k2 = 0; k2 < L; k2++) sn[(size_t)k2] = snd[(size_t)(k2 ^ (L / 2))];
        }
        cb.resize((size_t)N1 * 16 * parts);
        for (int n1 = 0; n1 < N1; n1++)
            for (int e = 0; e < 16 * parts; e++) {
                const int i = half ? (e >> 4) ^ (parts / 2) : e >> 4;
                const float2 w = unit(double(((long long)n1 * ((e & 15) + 256 * i + (half ? L / 2 : 0))) % N) / double(N));
                const float sg = (n1 & 1) ? -1.0f : 1.0f;
                cb[(size_t)n1 * 16 * parts + e] = make_float2(sg * w.x, sg * w.y);
            }
    } else if (p->poly_block) {
        // the narrow-channel block kernel (fdc_blocknarrow.hip): its LDS image, and W_N^(S V (b + r)) at [V][b], S = 256 / l
        const bool half = rb == L / 2;
        const int S = 256 / L;
        std::vector<float2> img((size_t)fdc::poly_block_narrow_table_points(L, N));
        fdc::poly_block_narrow_tables(L, N, sn.data(), img.data(), half, half ? 0 : rb);
        CHK_DEV(bk.d_tab.upload(img));
        const int NV = N / 256;                                      // virtual columns
        cb.resize((size_t)NV * 16);
        for (int V = 0; V < NV; V++)
            for (int b = 0; b < 16; b++) cb[(size_t)V * 16 + b] = unit(double(((long long)S * V * (b + rb)) % N) / double(N));
    }
    CHK_DEV(bk.d_shn.upload(sn));
    if (!cb.empty()) CHK_DEV(bk.d_cbt.upload(cb));
    return FDC_OK;
}

// ---- step 4b: what the banks of one width share, and the generic two-launch form's tile table
static int build_shared_bank_tables(fdc_pipeline *p)
{
    const int N = p->N;
    auto has = [&](int L) { for (const auto &b : p->banks) if (b.L == L) return true; return false; };
    auto twq_table = [&](int N1) {                      // W_N^(16 n1 q)
        std::vector<float2> tq((size_t)N1 * 16);
        for (int n1 = 0; n1 < N1; n1++)
            for (int q = 0; q < 16; q++) tq[(size_t)n1 * 16 + q] = unit(double((16ll * n1 * q) % N) / double(N));
        return tq;
    };
    if (has(256)) {
        CHK_DEV(p->d_twq.upload(twq_table(N / 256)));
        if (N / 256 == 1024) CHK_DEV(p->d_tw1024.upload(make_twiddles(1024)));
    }
    if (has(512) && p->poly_block) {
        std::vector<float2> t5(256);
        for (int k = 0; k < 256; k++) t5[(size_t)k] = unit(double(k) / 512.0);
        CHK_DEV(p->d_tw512.upload(t5));
        CHK_DEV(p->d_twq512.upload(twq_table(N / 512)));
    }
    if (has(1024) && p->poly_block) {
        CHK_DEV(p->d_tw1k.upload(make_twiddles(1024)));
        CHK_DEV(p->d_twq1k.upload(twq_table(N / 1024)));
    }
    // ONE on-grid bank of another width: its two-launch form (the whole plan where no block kernel applies; launch groups shorter than
    // block_min otherwise) wants the tile-local factor of the inter-pass twiddle in the tile's own order: t2[k2][t] = W_N^(t k2)
    if (p->banks.size() == 1 && p->banks[0].L != 256 && p->banks[0].r == 0 && p->bank_alias.empty()) {
        const int L = p->banks[0].L, TCg = fdc::poly_stage1_generic_tile_columns(N, L);
        std::vector<float2> t2v((size_t)L * TCg);
        for (int k2 = 0; k2 < L; k2++)
            for (int t = 0; t < TCg; t++) t2v[(size_t)k2 * TCg + t] = unit(double(((long long)t * k2) % N) / double(N));
        CHK_DEV(p->d_t2g.upload(t2v));
    }
    return FDC_OK;
}

// ---- step 4c: the block kernel as a forward transform (N = 65536: the spectrum path, the remainder of a split plan, the sinks)
static int build_forward_tables(fdc_pipeline *p)
{
    // twq / cbt as for a bank of 256-bin channels with r = 0, a flat "window" 1/N, and the slots of stage 2 mapped to the bins 256 c (+ k2) of
    // the shifted spectrum
    const int N = p->N, N1 = N / 256;
    std::vector<float2> tq((size_t)N1 * 16), cb((size_t)N1 * 16);
    for (int n1 = 0; n1 < N1; n1++)
        for (int j = 0; j < 16; j++) {
            tq[(size_t)n1 * 16 + j] = unit(double((16ll * n1 * j) % N) / double(N));
            const float2 w = unit(double(((long long)n1 * j) % N) / double(N));
            const float sg = (n1 & 1) ? -1.0f : 1.0f;
            cb[(size_t)n1 * 16 + j] = make_float2(sg * w.x, sg * w.y);
        }
    std::vector<float> sn(256, float(1.0 / double(N)));
    std::vector<long long> so((size_t)N1);
    for (int c = 0; c < N1; c++) so[(size_t)c] = 256ll * c;
    CHK_DEV(p->d_ftwq.upload(tq));
    CHK_DEV(p->d_fcbt.upload(cb));
    CHK_DEV(p->d_fshn.upload(sn));
    CHK_DEV(p->d_fslot.upload(so));
    return FDC_OK;
}

// ---- step 4d: plans that read part of the band: the 64-bin groups of the shifted spectrum some channel reads (a split plan's internal
// spectrum serves its remainder only); the forward kernels that store whole 64-bin runs per wave leave the other groups unwritten
static int build_keep_map(fdc_pipeline *p)
{
    const int N = p->N;
    std::vector<char> g64((size_t)N / 64, 0);
    bool all = true;
    for (int c = 0; c < p->C; c++) {
        if (p->split && !std::binary_search(p->rem.begin(), p->rem.end(), c)) continue;
        const auto &ch = p->chans[(size_t)c];
        for (int b = ch.f / 64; b <= (ch.f + ch.l - 1) / 64 && b < N / 64; b++) g64[(size_t)b] = 1;
    }
    for (char v : g64) all = all && v;
    if (all) return FDC_OK;
    if (N == 4096) {
        p->keep4096 = 0;
        for (int b = 0; b < 64; b++) if (g64[(size_t)b]) p->keep4096 |= 1ull << b;
        return FDC_OK;
    }
    // the block kernel's wave klo stores, per 64-row chunk q, the bins 256 c + 64 q .. + 63 of the slots c = klo + P khi (P = N / 8192 passes); slot
    // khi = k0 + 2 k1 sits in register 16 k0 + rev16(k1) (fdc_block256.hip, soff)
    const int P = N / 8192;
    std::vector<unsigned> kw((size_t)P * 4, 0u);
    for (int klo = 0; klo < P; klo++)
        for (int q = 0; q < 4; q++)
            for (int r = 0; r < 32; r++) {
                const int k0 = r >> 4, k1 = 4 * (r & 3) + ((r & 15) >> 2), c = klo + P * (k0 + 2 * k1);
                if (g64[(size_t)(4 * c + q)]) kw[(size_t)(klo * 4 + q)] |= 1u << r;
            }
    CHK_DEV(p->d_keep.upload(kw));
    return FDC_OK;
}


// ---- step 4: everything on the device
int build_device_state(fdc_pipeline *p, const fdc_pipeline_cfg *cfg, const std::vector<std::complex<float>> &pool,
                       const std::vector<int32_t> &flat, const std::vector<int32_t> &rflat)
{
    const int N = p->N, R = p->R, flags = p->cfg.flags, chunk = p->chunk;
    CHK_DEV(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    p->ntab = N;
    CHK_DEV(p->d_tw.upload(make_twiddles(N)));
    if (p->C > 0) {
        CHK_DEV(p->d_wins.alloc(pool.size()));
        CHK_DEV(hipMemcpy(p->d_wins, pool.data(), sizeof(float2) * pool.size(), hipMemcpyHostToDevice));
        CHK_DEV(p->d_chans.upload(p->chans));
        CHK_DEV(p->d_groups.upload(flat));
        if (!rflat.empty()) CHK_DEV(p->d_rgroups.upload(rflat));
    }
    CHK_DEV(p->d_tw256.upload(make_twiddles(256)));
    if (N > fdc::kMaxLdsFft) {
        // inter-pass twiddles of the two-pass transform, laid out like pass A's output: [k2][n1] = W_N^(n1*k2)
        const fdc::BigGeom bg = fdc::big_geom(N);
        std::vector<float2> tf((size_t)N);
        for (int k2 = 0; k2 < bg.N2; k2++)
            for (int n1 = 0; n1 < bg.N1; n1++) tf[(size_t)k2 * bg.N1 + n1] = unit(double((long long)n1 * k2) / double(N));
        CHK_DEV(p->d_twf.upload(tf));
    }
    for (auto &bk : p->banks) { const int rc = build_bank_tables(p, cfg, bk); if (rc != FDC_OK) return rc; }
    if (p->fused) {
        std::vector<fdc::F4Row> rows(64);
        int xch = 0;
        for (int w = 0; w < 4 * p->f4_teams; w++) {
            const unsigned cls = (p->f4_cls >> (4 * w)) & 0xfu;
            const int L = cls == 4 ? 1024 : cls == 3 ? 512 : cls >= 5 ? 16 << (8 - (int)cls) : 256, pitch = cls == 4 ? 1056 : cls == 3 ? 513 : cls >= 5 ? L + L / 16 : 272;
            for (int k = 0; k < 8; k++) {
                fdc::F4Row &r = rows[(size_t)(8 * w + k)];
                r = fdc::F4Row{0, 0, 0, 0, L - L / R, 0, 0};
                if (k >= (int)p->f4_wave[w].size()) continue;
                const int code = p->f4_wave[w][(size_t)k];
                const fdc::ChanDev &ch = p->chans[(size_t)(code >> 1)];
                r = fdc::F4Row{ch.f, ch.win_off, ch.shift, xch, ch.lout, 1 + (code & 1), (long long)ch.out_off};
                xch += pitch;
            }
        }
        CHK_DEV(p->d_f4rows.upload(rows));
    }
    { const int rc = build_shared_bank_tables(p); if (rc != FDC_OK) return rc; }
    p->fwd_block = fdc::poly_block_supports(N) && !p->cfg_generic && !(flags & FDC_PIPE_NO_BLOCK);      // N = 16384 / 32768 / 65536 (round 5: the forward variant has the pass-count template too)
    if (p->fwd_block) { const int rc = build_forward_tables(p); if (rc != FDC_OK) return rc; }
    {
        hipDeviceProp_t prop;
        CHK_DEV(hipGetDeviceProperties(&prop, cfg->device_id));
        p->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    // per-workgroup scratch of the block kernels: the forward-transform variant's second half of T, the R = 4 channelizers' rows 64..127
    if (p->fwd_block || (p->poly_block && R == 4)) CHK_DEV(p->d_fscr.alloc(32768 * (size_t)p->ncu));
    if (p->C > 0 && !(flags & FDC_PIPE_FULL_SPECTRUM) && (N == 4096 || p->fwd_block)) {
        const int rc = build_keep_map(p);
        if (rc != FDC_OK) return rc;
    }
    if (two_launch_possible(p)) {
        // G scratch of the two-launch form.  With block kernels only launch groups shorter than block_min take it
        const int L = p->banks[0].L, gblocks = p->poly_block ? std::min(chunk, p->block_min) : chunk;
        CHK_DEV(p->d_g.alloc((size_t)gblocks * (size_t)(L - L / R) * (size_t)(N / L)));
    }
    {
        // widest "channels x width" of a group above 4096 bins: a piece of the launch group is as many blocks as fit 32 Mi points
        size_t widest = 0;
        for (const auto &gr : p->groups) if (gr.first > 4096) { widest = std::max(widest, gr.second.size() * (size_t)gr.first); p->big_l = std::max(p->big_l, gr.first); }
        if (widest) {
            p->big_pts = std::max<size_t>(widest, std::min<size_t>((size_t)32 << 20, widest * (size_t)chunk));
            CHK_DEV(p->d_big.alloc(p->big_pts));
            CHK_DEV(p->d_wtasks.alloc(p->big_pts / 8192 + (size_t)p->C + 1));   // a piece: at most big_pts / l tasks, l >= 8192
        }
    }
    // two-pass scratch; with the block kernel only launch groups shorter than block_min take the two-pass kernels
    if (N > fdc::kMaxLdsFft) CHK_DEV(p->d_tmp.alloc((size_t)(p->fwd_block ? std::min(chunk, p->block_min) : chunk) * N));
    CHK_DEV(p->d_spec.alloc((size_t)chunk * N));
    return FDC_OK;
}

// fdc_pipeline_cfg.flags as create AND plan_preview read them: under FDC_DEBUG_ENV=1 the debugging variables override the fields (one place, so
// that what the preview describes is what create builds)
int effective_flags(int flags)
{
    auto on = [](const char *n) { const char *v = fdc::debug_env(n); return v && v[0] == '1'; };
    if (on("FDC_FORCE_GENERIC")) flags |= FDC_PIPE_FORCE_GENERIC;
    if (on("FDC_NO_POLY")) flags |= FDC_PIPE_NO_POLY;
    if (on("FDC_NO_BLOCK")) flags |= FDC_PIPE_NO_BLOCK;
    if (on("FDC_NO_FUSED")) flags |= FDC_PIPE_NO_FUSED;
    if (const char *bh = fdc::debug_env("FDC_BLOCK_HINTS")) {
        flags &= ~(FDC_PIPE_PLAIN_STORES | FDC_PIPE_NT_LOADS);
        if (!(atoi(bh) & 1)) flags |= FDC_PIPE_PLAIN_STORES;
        if (atoi(bh) & 2) flags |= FDC_PIPE_NT_LOADS;
    }
    return flags;
}

} }  // namespace fdc::pipe
