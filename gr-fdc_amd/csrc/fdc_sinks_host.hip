// Host engine of a sink bank (see fdc_sinks.hip for which engine a bank gets): the work() loops of PowerActivationChannel,
// activity_detection_channelizer_vcm and SegmentDetection as state machines on the host, between two GPU phases that cover
// a whole batch of blocks:
//     GPU power cells -> D2H -> host state machines (one pass over the batch, emits an extraction task list and PDU
//     records that reference tasks) -> GPU extractions -> D2H -> payload assembly.
// The decisions are inherently sequential over blocks and tiny (a few hundred floats per block); channels and segments do not
// interact, so a large bank is cut into ranges that worker threads take through the batch on their own, and their lists are
// merged afterwards (merge_worker_lists).  Behaviour follows lib/PowerActivationChannel_impl.cc and
// lib/activity_detection_channelizer_vcm_impl.cc; line references are given at each decision.
// The file exports one function, fdc::sinks::host_work_device (fdc_sinks_state.hpp).
#include "fdc_sinks_state.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>

using namespace fdc::sinks;

namespace {

// Where the decisions of one batch are collected: the handle's own lists, or the private lists of a worker thread that
// runs a range of PowerActivationChannels on its own (they do not interact; the lists are merged afterwards).
struct Emit {
    std::vector<fdc::ExtractTask> *tasks;
    std::vector<int> *task_w, *task_skip;
    int64_t *ext_used;
    std::vector<PduRec> *pdus;
    int64_t blockcount;             // the block counter while the current block is processed
    int64_t key;                    // order key of a PDU emitted now
};

int64_t add_task(Emit &e, int slot, int start, int w, int skip, int win_off)
{
    fdc::ExtractTask t{};
    t.slot = slot; t.start = start; t.win_off = win_off; t.out_off = *e.ext_used;
    *e.ext_used += w - skip;
    e.tasks->push_back(t);
    e.task_w->push_back(w); e.task_skip->push_back(skip);
    return (int64_t)e.tasks->size() - 1;
}

// ---------------------------------------------------------------- PowerActivationChannel
void pac_process(const fdc_sinks *s, Emit &e, Pac &p, int slot)            // process_channel, …_impl.cc:260-284
{
    BlockRef b;
    b.task = add_task(e, slot, p.extract_start, p.extract_width, p.ovl_offset, p.win_off + p.phase * p.extract_width);
    p.blocks.push_back(std::move(b));
    p.count++;
    p.phase = (p.phase + p.deltaphase) % s->R;
}

void pac_emit(const fdc_sinks *s, Emit &e, Pac &p, bool fin)               // emit_data, :212-258
{
    PduRec r;
    r.key = e.key;
    r.meta.kind = 0; r.meta.source = p.ID; r.meta.chan_id = p.id_at_activation;
    r.meta.finalized = fin; r.meta.part = p.part; r.meta.has_part = 1;
    r.meta.rel_cfreq = (double)(p.extract_start + p.extract_stop) / 2.0 / (double)s->N;
    r.meta.rel_bw = (double)p.extract_width / (double)s->N;
    r.meta.blockstart = e.blockcount - p.count; r.meta.blockend = e.blockcount;
    r.meta.vectorstart = p.extract_start; r.meta.vectorend = p.extract_stop;
    std::snprintf(r.meta.id, sizeof r.meta.id, "%s", p.msg_id.c_str());
    r.blocklen = p.output_len;
    r.blocks = std::move(p.blocks);                                        // the whole list changes hands: no per-block move
    p.blocks.clear();
    p.blocks.reserve(r.blocks.size() + 2);
    if (s->cfg.verbose)                                                    // :246-253
        sink_log(s, pac_logfile(p), p.msg_id + (fin ? std::string(".fin") : ".parted." + std::to_string(p.part)) + ": start=" +
                 std::to_string(p.extract_start) + ", stop=" + std::to_string(p.extract_stop) + ", blockstart=" +
                 std::to_string((long long)r.meta.blockstart) + ", blockend=" + std::to_string((long long)r.meta.blockend));
    e.pdus->push_back(std::move(r));
    p.part++;
}

void pac_step(const fdc_sinks *s, Emit &e, Pac &p, float pwr, int slot)    // one item of work(), :146-170
{
    if (pwr == 0.0f) pwr = FLT_MIN;                                        // :293-294
    bool changed = false;
    if (!p.active && pwr / p.lastpower >= s->pac_thr) changed = true;      // :296-302
    else if (p.active && p.lastpower / pwr >= s->pac_thr) changed = true;
    p.lastpower = pwr;
    if (changed) {
        if (!p.active) {                                                   // activate(), :198-210
            p.part = 0; p.count = 0; p.active = true; p.phase = 0; p.blocks.clear();
            p.id_at_activation = p.finished;
            p.msg_id = current_time_string() + ".PowActChan." + std::to_string(p.ID) + "." + std::to_string(p.finished);
            pac_process(s, e, p, slot - 1);                                // previous block (slot 0 = saved history)
            pac_process(s, e, p, slot);
        } else {
            pac_process(s, e, p, slot);
            p.active = false;                                              // deactivate(), :189-196
            pac_emit(s, e, p, true);
            p.finished++;
        }
    } else if (p.active) {
        pac_process(s, e, p, slot);
        const int mb = s->cfg.pac_maxblocks;
        if (mb == 0 || (mb > 0 && p.count % mb == 0)) pac_emit(s, e, p, false);
    }
}

// ---------------------------------------------------------------- activity_detection_channelizer_vcm
void det_process(fdc_sinks *s, Emit &e, DetChan &c, int slot)        // process_channel, …vcm_impl.cc:373-397
{
    BlockRef b;
    b.task = add_task(e, slot, c.extract_start, c.extract_width, c.ovlskip,
                      s->det_win_off[c.wclass] + c.phase * c.extract_width);
    c.data.push_back(std::move(b));
    c.count++;
    c.phase = (c.phase + c.phaseincrement) % s->R;
}

void det_emit(fdc_sinks *s, Emit &e, Segment &g, DetChan &c, bool fin, size_t nblk)   // :406-452 / :454-510
{
    PduRec r;
    r.key = e.key++;
    // the number the ID string carries (activate()): SegmentDetection's own ID where the bank was given one — as the device engine reports it
    r.meta.kind = 1; r.meta.chan_id = c.ID;
    r.meta.source = (s->cfg.det_variant == 1 && s->cfg.det_id >= 0 && s->segs.size() == 1) ? s->cfg.det_id : g.ID;
    r.meta.finalized = fin; r.meta.part = c.part; r.meta.has_part = fin ? (c.part > 0) : 1;
    r.meta.rel_bw = (double)c.extract_width / (double)s->N;
    r.meta.rel_cfreq = (double)(c.extract_start + c.extract_stop) / 2.0 / (double)s->N;
    // the vcm block counts from 1 (…vcm_impl.cc:188), SegmentDetection from 0 (SegmentDetection_impl.cc:118)
    const int64_t bc = e.blockcount - (s->cfg.det_variant == 1 ? 1 : 0);
    // blockcount - count in the counter's own type: the vcm block's is `unsigned int` (…vcm_impl.h:142), so a channel activated in
    // the very first item (count 2 with the zero history, counter 1) publishes 4294967295, not -1; SegmentDetection's size_t
    // difference comes out of pmt::from_long(long) as the signed value (SegmentDetection_impl.h:96)
    r.meta.blockstart = s->cfg.det_variant == 1 ? bc - c.count : (int64_t)(uint32_t)(bc - c.count); r.meta.blockend = bc;
    r.meta.vectorstart = c.extract_start; r.meta.vectorend = c.extract_stop;
    std::snprintf(r.meta.id, sizeof r.meta.id, "%s", c.msg_id.c_str());
    r.blocklen = c.outputsamples;
    for (size_t i = 0; i < nblk; i++) { r.blocks.push_back(std::move(c.data.front())); c.data.pop_front(); }
    if (s->cfg.verbose)                                                        // …vcm_impl.cc:441-450, :498-508
        sink_log(s, s->det_logfile, c.msg_id + (fin ? std::string(".fin: ") : ".parted." + std::to_string(c.part) + ": ") + "start=" +
                 std::to_string(c.extract_start) + ", stop=" + std::to_string(c.extract_stop) + ", blockstart=" +
                 std::to_string((long long)r.meta.blockstart) + ", blockend=" + std::to_string((long long)r.meta.blockend));
    e.pdus->push_back(std::move(r));
}

void seg_detect(fdc_sinks *s, Segment &g, const float *P)   // detect_channels, :617-628
{
    const int n = g.ncell, dec = s->dec;
    // get_active_channels, :694-739
    struct Edge { float r; int pos; };
    std::vector<Edge> rise;
    std::vector<int> fall;
    const float inv = 1.0f / s->det_thr;
    const bool sd = s->cfg.det_variant == 1;
    for (int i = 1; i < n; i++) {
        // vcm guards a zero denominator (:703-706); SegmentDetection divides as is (volk_32f_x2_divide_32f, :206)
        const float pd = (!sd && P[i - 1] == 0.0f) ? P[i] / FLT_MIN : P[i] / P[i - 1];
        if (pd > s->det_thr) rise.push_back({pd, (i - 1) * dec + g.start});
        else if (sd) { if (pd < inv) fall.push_back(i * dec + g.start); }        // if / else if (:209-210)
        if (!sd && pd < inv) fall.push_back(i * dec + g.start);                  // two independent ifs (:708-709)
    }
    std::stable_sort(rise.begin(), rise.end(), [](const Edge &a, const Edge &b) { return a.r > b.r; });   // :713
    std::vector<std::pair<int, int>> cand;
    for (const Edge &e : rise) {
        int ne = -1;
        for (int f : fall) if (f > e.pos) { ne = f; break; }                   // get_next_int, :678-692
        if (ne <= e.pos) continue;
        bool clash = false;
        for (auto &a : cand) if (e.pos < a.second && ne >= a.first) { clash = true; break; }   // :727-734
        if (!clash) cand.emplace_back(e.pos, ne);
    }
    // match_active_channels, :741-783
    if (cand.empty()) {
        for (auto &c : g.chans) c.inactive += 1;
        return;
    }
    for (auto &c : g.chans) {
        bool idle = true;
        for (size_t i = 0; i < cand.size();) {
            if (cand[i].first < c.detect_stop && cand[i].second >= c.detect_start) {
                c.inactive = 0; idle = false;
                cand.erase(cand.begin() + i);
            } else i++;
        }
        if (idle) c.inactive += 1;
    }
    for (auto &pc : cand) {                                                    // activate, :785-841
        const int dw = pc.second - pc.first, mid = pc.first + dw / 2;
        const int ew = pow2ceil((int)std::ceil((double)dw * (1.0 + 2.0 * s->cfg.window_flank_puffer)));
        if (ew > s->N) continue;                                               // logged and skipped in the reference
        if (s->det_win_off[(size_t)std::lround(std::log2((double)ew))] < 0) continue;   // no window table for this width (see create)
        int es = mid - ew / 2, ee = mid + ew / 2;
        if (es < 0) { es = 0; ee = ew; }
        if (ee > s->N) { ee = s->N; es = s->N - ew; }
        DetChan c{};
        c.ID = g.counter++;
        c.detect_start = pc.first; c.detect_stop = pc.second; c.extract_start = es; c.extract_stop = ee;
        c.extract_width = ew; c.wclass = (int)std::log2((double)ew);
        c.ovlskip = ew / s->R; c.outputsamples = ew - c.ovlskip;
        c.count = 0; c.phase = 0; c.phaseincrement = es % s->R; c.inactive = -1; c.part = 0;
        const int segname = (s->cfg.det_variant == 1 && s->cfg.det_id >= 0 && s->segs.size() == 1) ? s->cfg.det_id : g.ID;
        c.msg_id = current_time_string() + ".DETECTED." + std::to_string(segname) + "." + std::to_string(c.ID);
        g.chans.push_back(std::move(c));
    }
}

void seg_extract(fdc_sinks *s, Emit &e, Segment &g, int slot)        // extract_channels_in_segments_singlethread, :306-337
{
    const int mb = s->cfg.det_maxblocks, delay = s->cfg.det_deactivation_delay;
    for (auto &c : g.chans) {
        if (c.inactive < 0) { det_process(s, e, c, slot - 1); det_process(s, e, c, slot); c.inactive = 0; }   // :399-403
        else if (c.inactive > delay) det_emit(s, e, g, c, true, c.data.size());
        else det_process(s, e, c, slot);
        if (s->cfg.det_variant == 0 && mb >= 0 && (int)c.data.size() >= mb) {  // :317-318, :454-470
            const size_t ntx = mb == 0 ? c.data.size() : (size_t)mb;
            if (ntx > 0) { det_emit(s, e, g, c, false, ntx); c.part++; }
        }
    }
    if (s->cfg.det_variant == 1 && mb >= 0)                                     // SegmentDetection: separate pass, :359-362
        for (auto &c : g.chans)
            if ((int)c.data.size() >= mb) {
                const size_t ntx = mb == 0 ? c.data.size() : (size_t)mb;
                if (ntx > 0) { det_emit(s, e, g, c, false, ntx); c.part++; }
            }
    for (size_t i = 0; i < g.chans.size();)                                     // clear_inactive_channels, :512-524
        if (g.chans[i].inactive > delay) g.chans.erase(g.chans.begin() + i); else i++;
}

// The workers' lists join the handle's: the tasks of worker t land behind the tasks in front of them (base b0), so every task
// index the worker handed out moves up by b0 — in its PDUs' blocks here, in the blocks its live owners still hold through
// shift_live(t, b0) (the one thing the two phases differ in).  Every worker moves its own lists into place; the PDUs are
// appended in worker order (the caller's stable_sort by order key restores the emission order).  Returns the pool's status.
template <class ShiftLive>
bool merge_worker_lists(fdc_sinks *s, int nw, ShiftLive shift_live)
{
    std::vector<int64_t> base((size_t)nw + 1, (int64_t)s->tasks.size());
    for (int t = 0; t < nw; t++) {
        base[(size_t)t + 1] = base[(size_t)t] + (int64_t)s->wl[(size_t)t]->tasks.size();
        s->ext_used += s->wl[(size_t)t]->used;
    }
    s->tasks.resize((size_t)base[(size_t)nw]); s->task_w.resize((size_t)base[(size_t)nw]); s->task_skip.resize((size_t)base[(size_t)nw]);
    const bool ok = s->pool.run(nw, [&](int t) {
        WorkerLists &L = *s->wl[(size_t)t];
        const int64_t b0 = base[(size_t)t];
        std::copy(L.tasks.begin(), L.tasks.end(), s->tasks.begin() + b0);
        std::copy(L.w.begin(), L.w.end(), s->task_w.begin() + b0);
        std::copy(L.skip.begin(), L.skip.end(), s->task_skip.begin() + b0);
        if (b0) {
            for (auto &r : L.pdus) for (auto &bk : r.blocks) if (bk.task >= 0) bk.task += b0;
            shift_live(t, b0);
        }
    });
    for (int t = 0; t < nw; t++)
        for (auto &r : s->wl[(size_t)t]->pdus) s->pdus.push_back(std::move(r));
    return ok;
}

}  // namespace

namespace fdc { namespace sinks {

int host_work_device(fdc_sinks *s, int nblocks)
{
    static const bool trace = fdc::debug_env("FDC_SINKS_TRACE") != nullptr;      // phase times on stderr (diagnostics)
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t0 = now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        const auto t1 = now();
        std::fprintf(stderr, "[fdc_sinks] %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    };
    s->pdus.clear();
    lap("previous PDUs released");
    bool pool_ok = true;
    const int N = s->N, ncells = (int)s->cells.size();
    // phase 1: power of every cell of every block
    bool have_power = false;
    { const int rb = batch_begin(s, nblocks, &have_power); if (rb != FDC_OK) return rb; }
    if (ncells) {
        if (!have_power) HIPCHK(fdc::launch_cell_power(s->d_spec + N, N, s->d_cells, ncells, nblocks, s->d_power, s->stream));
        s->h_power.resize((size_t)ncells * nblocks);
        HIPCHK(hipMemcpyAsync(s->h_power.data(), s->d_power, sizeof(float) * s->h_power.size(), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    lap("cell power + D2H");
    // phase 2: decisions (work() loops of both reference blocks).  Every block: the PowerActivationChannels in order, then the
    // detection segments.  PowerActivationChannel instances do not interact, so a large bank is cut into ranges that worker
    // threads run over the whole batch on their own; the PDUs carry an order key (block, then instance) and are put back
    // into the order the sequential loop emits them in.
    s->tasks.clear(); s->task_w.clear(); s->task_skip.clear(); s->ext_used = 0;
    const int64_t bc0 = s->blockcount;
    const int npac = (int)s->pacs.size();
    int nthr = 1;
    if (npac >= 32 && (int64_t)npac * nblocks >= 16384 && s->cfg.verbose == 0) {
        const unsigned hc = std::thread::hardware_concurrency();
        nthr = (int)std::min<unsigned>(8, std::max<unsigned>(1, hc / 2));
        if (s->host_threads > 0) nthr = s->host_threads;
        nthr = std::min(nthr, npac / 8);
    }
    auto run_pacs = [&](int a, int b, Emit e) {
        for (int m = 0; m < nblocks; m++) {
            const float *P = s->h_power.data() + (size_t)m * ncells;
            e.blockcount = bc0 + m;
            for (int i = a; i < b; i++) {
                e.key = ((int64_t)m << kKeyShiftHost) | i;
                pac_step(s, e, s->pacs[(size_t)i], P[s->pacs[(size_t)i].cell], m + 1);
            }
        }
    };
    // the workers' form: one channel at a time over the whole batch (its state stays in registers, its tasks are appended in
    // one run); the PDUs find their place through the order key, the tasks through the landing layout
    auto run_pacs_by_channel = [&](int a, int b, Emit e) {
        const float *P0 = s->h_power.data();
        for (int i = a; i < b; i++) {
            Pac &p = s->pacs[(size_t)i];
            const float *P = P0 + p.cell;
            for (int m = 0; m < nblocks; m++) {
                e.blockcount = bc0 + m;
                e.key = ((int64_t)m << kKeyShiftHost) | i;
                pac_step(s, e, p, P[(size_t)m * ncells], m + 1);
            }
        }
    };
    Emit em{&s->tasks, &s->task_w, &s->task_skip, &s->ext_used, &s->pdus, bc0, 0};
    if (nthr > 1) {
        while ((int)s->wl.size() < nthr) s->wl.emplace_back(new WorkerLists());
        std::vector<int> lo((size_t)nthr + 1);
        for (int t = 0; t <= nthr; t++) lo[(size_t)t] = (int)((int64_t)npac * t / nthr);
        std::vector<double> tms((size_t)nthr, 0.0);
        pool_ok = s->pool.run(nthr, [&](int t) {
            const auto a0 = now();
            WorkerLists &L = *s->wl[(size_t)t];
            L.clear();
            run_pacs_by_channel(lo[(size_t)t], lo[(size_t)t + 1], Emit{&L.tasks, &L.w, &L.skip, &L.used, &L.pdus, bc0, 0});
            tms[(size_t)t] = std::chrono::duration<double, std::milli>(now() - a0).count();
        });
        if (trace) { std::fprintf(stderr, "[fdc_sinks]     worker ms:"); for (double v : tms) std::fprintf(stderr, " %.3f", v); std::fprintf(stderr, "\n"); }
        lap("  PAC state machines (threads)");
        pool_ok = merge_worker_lists(s, nthr, [&](int t, int64_t b0) {
            for (int i = lo[(size_t)t]; i < lo[(size_t)t + 1]; i++)
                for (auto &bk : s->pacs[(size_t)i].blocks) if (bk.task >= 0) bk.task += b0;
        });
    } else if (npac) {
        run_pacs(0, npac, em);
    }
    lap("  PAC total incl. merge");
    const int nseg = (int)s->segs.size();
    const int nthr_s = (nseg >= 2 && (int64_t)nseg * nblocks >= 256 && s->cfg.verbose == 0) ? std::min(nseg, 8) : 1;
    if (nthr_s > 1) {
        // The segments of a detection block do not interact either (…vcm_impl.cc:558-562 loops over them per item): a worker
        // takes whole segments through the batch; the order key (block, then segment, then emission) restores the reference's order.
        while ((int)s->wl.size() < nthr_s) s->wl.emplace_back(new WorkerLists());
        pool_ok = s->pool.run(nthr_s, [&](int t) {
            WorkerLists &L = *s->wl[(size_t)t];
            L.clear();
            Emit e{&L.tasks, &L.w, &L.skip, &L.used, &L.pdus, bc0, 0};
            for (int gi = t; gi < nseg; gi += nthr_s) {
                Segment &g = s->segs[(size_t)gi];
                for (int m = 0; m < nblocks; m++) {
                    e.blockcount = bc0 + m;
                    e.key = ((int64_t)m << kKeyShiftHost) | kKeyDetBitHost | ((int64_t)gi << kKeySegShiftHost);
                    seg_detect(s, g, s->h_power.data() + (size_t)m * ncells + g.cell0);
                    seg_extract(s, e, g, m + 1);
                }
            }
        });
        pool_ok = merge_worker_lists(s, nthr_s, [&](int t, int64_t b0) {
            for (int gi = t; gi < nseg; gi += nthr_s)
                for (auto &c : s->segs[(size_t)gi].chans) for (auto &bk : c.data) if (bk.task >= 0) bk.task += b0;
        });
    } else if (nseg)
        for (int m = 0; m < nblocks; m++) {
            const float *P = s->h_power.data() + (size_t)m * ncells;
            em.blockcount = bc0 + m;
            em.key = ((int64_t)m << kKeyShiftHost) | kKeyDetBitHost;
            for (auto &g : s->segs) seg_detect(s, g, P + g.cell0);                  // …vcm_impl.cc:558
            for (auto &g : s->segs) seg_extract(s, em, g, m + 1);                   // :562
        }
    s->blockcount = bc0 + nblocks;
    if (!pool_ok) return fdc::set_error(FDC_ERR_NOMEM, "a decision worker failed (out of memory?): the batch is lost");
    if ((npac && (nthr > 1 || nseg)) || nthr_s > 1)
        std::stable_sort(s->pdus.begin(), s->pdus.end(), [](const PduRec &a, const PduRec &b) { return a.key < b.key; });
    lap("decisions (host)");
    // Landing layout: the blocks of every PDU emitted in this call sit one behind the other (PDU order, block order),
    // so a PDU whose blocks all come from this call needs no assembly — its payload IS a run of the landing buffer;
    // blocks that stay buffered in live channels follow.
    {
        std::vector<int64_t> noff(s->tasks.size(), -1);
        int64_t pos = 0;
        for (auto &r : s->pdus)
            for (auto &b : r.blocks)
                if (b.task >= 0) { noff[(size_t)b.task] = pos; pos += r.blocklen; }
        for (size_t i = 0; i < s->tasks.size(); i++)
            if (noff[i] < 0) { noff[i] = pos; pos += s->task_w[i] - s->task_skip[i]; }
        for (size_t i = 0; i < s->tasks.size(); i++) s->tasks[i].out_off = noff[i];
    }
    // phase 3: extractions, one launch per width class
    const size_t nt = s->tasks.size();
    if (nt) {
        // tasks grouped by width: a counting sort over the (at most 25) power-of-two classes, order inside a class kept;
        // nothing to do when every task has the same width (a PowerActivationChannel bank of equal channels)
        size_t cnt[32] = {0}, first[32];
        for (size_t i = 0; i < nt; i++) cnt[31 - __builtin_clz((unsigned)s->task_w[i])]++;
        size_t acc = 0;
        int nclasses = 0;
        for (int k = 0; k < 32; k++) { first[k] = acc; acc += cnt[k]; nclasses += cnt[k] != 0; }
        const fdc::ExtractTask *upload = s->tasks.data();
        if (nclasses > 1) {
            s->sorted.resize(nt);
            size_t pos[32];
            std::copy(first, first + 32, pos);
            for (size_t i = 0; i < nt; i++) s->sorted[pos[31 - __builtin_clz((unsigned)s->task_w[i])]++] = s->tasks[i];
            upload = s->sorted.data();
        }
        const size_t used = (size_t)s->ext_used;
        HIPCHK(s->d_tasks.reserve(nt, nt * 2));
        HIPCHK(s->h_ext.reserve(used, used * 2));
        HIPCHK(s->d_ext.reserve(used, used * 2));
        lap("  task grouping + buffers");
        HIPCHK(hipMemcpyAsync(s->d_tasks, upload, sizeof(fdc::ExtractTask) * nt, hipMemcpyHostToDevice, s->stream));
        {
            const int rce = run_extractions(s, s->d_tasks, first, cnt, s->d_ext, trace);
            if (rce != FDC_OK) return rce;
        }
        if (trace) { HIPCHK(hipStreamSynchronize(s->stream)); lap("  task upload + extraction kernels"); }
        HIPCHK(hipMemcpyAsync(s->h_ext, s->d_ext, sizeof(float2) * (size_t)s->ext_used, hipMemcpyDeviceToHost, s->stream));
    }
    // history <- last block of this call (save_hist, PowerActivationChannel_impl.cc:173; …vcm_impl.cc:571)
    { const int rh = batch_end_history(s, nblocks, s->stream); if (rh != FDC_OK) return rh; }
    HIPCHK(hipStreamSynchronize(s->stream));
    { const int rh = batch_end_swap(s, nullptr); if (rh != FDC_OK) return rh; }
    lap("extractions + D2H");
    // phase 4: payloads; blocks still buffered in live channels become host copies
    auto resolve = [&](BlockRef &b, int len) {
        if (b.task >= 0) {
            const cfl *src = s->h_ext + s->tasks[(size_t)b.task].out_off;
            b.owned.assign(src, src + len);
            b.task = -1;
        }
    };
    auto finish_pdu = [&](PduRec &r) {
        bool all_here = !r.blocks.empty();
        for (auto &b : r.blocks) if (b.task < 0) { all_here = false; break; }
        if (all_here) {                     // contiguous in the landing buffer by construction (layout above)
            r.meta.nsamples = (int64_t)r.blocks.size() * r.blocklen;
            r.meta.samples = s->h_ext + s->tasks[(size_t)r.blocks.front().task].out_off;
        } else {                            // some blocks were kept from an earlier call: assemble
            r.payload.reserve(r.blocks.size() * (size_t)r.blocklen);
            for (auto &b : r.blocks) {
                const cfl *src = b.task >= 0 ? s->h_ext + s->tasks[(size_t)b.task].out_off : b.owned.data();
                r.payload.insert(r.payload.end(), src, src + r.blocklen);
            }
            r.meta.nsamples = (int64_t)r.payload.size();
            r.meta.samples = r.payload.data();
        }
        r.blocks.clear();
    };
    // PDUs and live channels are independent of each other: a large bank is finished by the worker threads
    const int npdu = (int)s->pdus.size();
    const int nasm = std::max(nthr, nthr_s);
    if (nasm > 1 && (npdu >= 64 || npac >= 64)) {
        pool_ok = s->pool.run(nasm, [&](int t) {
            for (int i = (int)((int64_t)npdu * t / nasm), e = (int)((int64_t)npdu * (t + 1) / nasm); i < e; i++) finish_pdu(s->pdus[(size_t)i]);
            for (int i = (int)((int64_t)npac * t / nasm), e = (int)((int64_t)npac * (t + 1) / nasm); i < e; i++)
                for (auto &b : s->pacs[(size_t)i].blocks) resolve(b, s->pacs[(size_t)i].output_len);
        });
    } else {
        for (auto &r : s->pdus) finish_pdu(r);
        for (auto &p : s->pacs) for (auto &b : p.blocks) resolve(b, p.output_len);
    }
    for (auto &g : s->segs) for (auto &c : g.chans) for (auto &b : c.data) resolve(b, c.outputsamples);
    if (!pool_ok) return fdc::set_error(FDC_ERR_NOMEM, "a payload worker failed (out of memory?): the batch is lost");
    lap("payload assembly");
    if (trace) std::fprintf(stderr, "[fdc_sinks] %zu tasks, %lld samples extracted, %zu PDUs\n", nt, (long long)s->ext_used, s->pdus.size());
    return nblocks;
}

}}  // namespace fdc::sinks
