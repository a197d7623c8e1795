// The sink bank's handle and what its two engines share (private to csrc): fdc_sinks.hip holds construction, the C entries, the
// shared batch helpers and the device engine's host side; fdc_sinks_host.hip holds the host engine.  See fdc_sinks.hip for which
// engine a bank gets.
#pragma once
#include "../../include/fdc_amd.h"
#include "fdc_buffers.hpp"
#include "fdc_iq.hpp"
#include "fdc_kernels.h"
#include "fdc_sinks_dev.h"

#include <cfloat>
#include <cmath>
#include <complex>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace fdc { int set_error(int code, const char *fmt, ...); int pick_device(int device_id); const char *debug_env(const char *name); }

#define HIPCHK(expr)                                                                                              \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess) return fdc::set_error(FDC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// The record types are named (not in an anonymous namespace): struct fdc_sinks has members of them and is seen by two translation units.
namespace fdc { namespace sinks {

using cfl = std::complex<float>;

// A buffered output block of a channel: either still on the device as the result of a task of the current call, or a
// host copy carried over from an earlier call.
struct BlockRef {
    int64_t task = -1;
    std::vector<cfl> owned;
};

struct PduRec {
    int64_t key = 0;                // emission order inside a call (layout: fdc_sinks_dev.h, kKeyShiftHost / kKeyShiftDev)
    fdc_pdu meta{};
    std::vector<BlockRef> blocks;
    int blocklen = 0;               // samples per block
    std::vector<cfl> payload;
};

struct Pac {
    int ID = 0, extract_start = 0, extract_stop = 0, extract_width = 0, output_len = 0, ovl_offset = 0;
    int measure_start = 0, measure_stop = 0, deltaphase = 0, win_off = 0, cell = 0;
    bool active = false;
    float lastpower = FLT_MAX;
    int count = 0, phase = 0, part = 0, finished = 0, id_at_activation = 0;
    std::string msg_id;                  // create_ID() at activation, :308-312
    std::vector<BlockRef> blocks;        // handed to the PDU as a whole when it is emitted
};

struct DetChan {
    int ID, detect_start, detect_stop, extract_start, extract_stop, extract_width, wclass, ovlskip, outputsamples;
    int count, phase, phaseincrement, inactive, part;
    std::string msg_id;                  // get_ID_for_msg() at activation, …vcm_impl.cc:526-530
    std::deque<BlockRef> data;
};

struct Segment {
    int ID = 0, start = 0, stop = 0, width = 0, ncell = 0, cell0 = 0, counter = 0;
    std::deque<DetChan> chans;
};

// What a worker thread collects while it runs its range of PowerActivationChannels over a batch.  Kept from call to call:
// the lists keep their capacity (no page faults on fresh heap memory in every call).
struct WorkerLists {
    std::vector<fdc::ExtractTask> tasks;
    std::vector<int> w, skip;
    int64_t used = 0;
    std::vector<PduRec> pdus;
    void clear() { tasks.clear(); w.clear(); skip.clear(); used = 0; pdus.clear(); }
};

// Fork-join pool of the handle (threads are made once; a batch costs two condition-variable round trips instead of a
// thread creation per worker).
class WorkerPool {
public:
    ~WorkerPool() { stop(); }
    // false: a job threw (std::bad_alloc from a growing list, normally): the batch is lost, the process is not
    bool run(int n, const std::function<void(int)> &fn)
    {
        if ((int)th_.size() < n) grow(n);
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = &fn; njob_ = n; pending_ = n; gen_++; failed_ = false;
        }
        cv_.notify_all();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&] { return pending_ == 0; });
        job_ = nullptr;
        return !failed_;
    }
    void stop()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
        th_.clear();
    }
private:
    void grow(int n)
    {
        for (int i = (int)th_.size(); i < n; i++)
            th_.emplace_back([this, i] {
                uint64_t seen = 0;
                for (;;) {
                    const std::function<void(int)> *fn = nullptr;
                    {
                        std::unique_lock<std::mutex> lk(m_);
                        cv_.wait(lk, [&] { return quit_ || (gen_ != seen && i < njob_); });
                        if (quit_) return;
                        seen = gen_; fn = job_;
                    }
                    bool ok = true;
                    try { (*fn)(i); } catch (...) { ok = false; }     // nothing may unwind out of a worker thread
                    {
                        std::lock_guard<std::mutex> g(m_);
                        if (!ok) failed_ = true;
                        pending_--;
                    }
                    done_.notify_one();
                }
            });
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)> *job_ = nullptr;
    int njob_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
    bool quit_ = false, failed_ = false;
};

}}  // namespace fdc::sinks

struct fdc_sinks {
    template <typename T> using DevBuf = fdc::DevBuf<T>;
    template <typename T> using PinBuf = fdc::PinBuf<T>;
    using cfl = fdc::sinks::cfl;
    // ================================================================ common to both engines
    fdc_sinks_cfg cfg{};
    int N = 0, R = 0, dec = 1;
    float pac_thr = 0.f, det_thr = 0.f;
    std::vector<fdc::sinks::Pac> pacs;       // geometry (both engines) and state (host engine)
    std::vector<fdc::sinks::Segment> segs;
    std::vector<int> det_win_off;            // per width class
    std::vector<fdc::PowerCell> cells;
    int64_t blockcount = 1;                  // both reference blocks start counting at 1 (hist is block 0)
    // A work / submit / flush call that fails after it has begun to advance the bank's state (block counter, channel state on the
    // device, buffered blocks, the two-deep pipeline) cannot be undone or repeated: the handle is dead from then on and every
    // later call says so (include/fdc_amd.h, "Failure").
    bool poisoned = false;
    std::string poison_why;
    hipStream_t stream = nullptr;
    DevBuf<float2> d_spec;                   // (max_blocks + 1) * N: slot 0 = history block.  The buffer the NEXT batch is read from
    DevBuf<float2> d_wins, d_tw, d_tw256;    // window pool, exp(-2 pi i k/N), exp(-2 pi i j/256)
    DevBuf<fdc::PowerCell> d_cells;
    DevBuf<float> d_power;                   // power cells of the batch in d_spec
    // FDC_SINKS_LOOKAHEAD: a second spectrum / power buffer and a stream of its own for their producer, so that the forward transform
    // (and the power cells) of batch n + 1 run on the device beside the decision kernels of batch n — one wave per channel or a
    // workgroup per segment: latency-bound kernels that leave the machine idle (fdc_sinks_spectrum_ahead, fdc_sinks_prepare_ahead).
    // d_spec / d_power always name the buffers of the batch the next submit reads; the pair swaps when a batch's extractions are enqueued.
    DevBuf<float2> d_spec_ahead;
    DevBuf<float> d_power_ahead;
    // Two, not three: with two, the forward transform of batch n + 2 waits for the extractions of batch n to release their buffer, and a batch's whole
    // chain (transform, cells, decisions, the host's look at the summary, task placement, extractions: 0.65 ms at configs[2]) runs two deep: 0.34 ms per
    // step for 0.29 ms of fill-stream work (profiles/r06/timeline_cfg3_shipped.txt).  With a third buffer (round 6, measured and removed) the transform
    // does run beside the extractions — and both slow down: they are the two bandwidth-heavy kernels of the step (configs[2] 0.340 -> 0.335 ms, forward
    // kernel 0.25 -> 0.28; configs[4] 0.49 -> 0.53, forward kernel 0.40 beside k_det_track and the extractions; profiles/r06/sched_three_buffers.txt).
    // The step is the memory system's, not the schedule's.
    // round 6: the power of every 16-bin group of the spectra in d_spec (slot 1 on) / d_spec_ahead, written by the producer's forward kernel
    // (fdc_pipeline_process_device_power) beside the spectrum: fdc_sinks_prepare_from_groups sums the cells from it instead of reading the spectrum back
    DevBuf<float> d_gpow, d_gpow_ahead;
    hipStream_t s_fill = nullptr;
    hipEvent_t ev_fill = nullptr;
    // ... and two side streams: the width classes above 4096 points are two small launches each (a few hundred transforms); side by side
    // they fill the device, one after the other they do not (configs[4]: 3 x (42 + 20) us).  Only with the flag: with the payload copy to the
    // host running, more streams than hardware queues put a class behind the copy (profiles/r03/NOTES.md).
    hipStream_t s_side[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    // ... and the extraction kernels of a batch on a stream of their own (s_x), so that the NEXT batch's decision chain — enqueued on the bank's
    // stream by the next submit — starts beside them instead of behind them (two deep as before: that submit hands out this batch's PDUs).
    // Placement of the tasks and the buffered blocks' move stay on the bank's stream (they read what the next chain overwrites).
    hipStream_t s_x = nullptr;
    hipEvent_t ev_tasks = nullptr;
    hipEvent_t ev_ready = nullptr, ev_ready_ahead = nullptr;   // recorded on s_fill behind the power cells of the batch in d_spec / d_spec_ahead (fdc_sinks_prepare)
    int prepared = -1, prepared_ahead = -1;  // blocks whose power cells are already (being) computed in d_power / d_power_ahead on s_fill; -1 = none
    DevBuf<float2> d_wide;                   // scratch of extractions wider than 4096 points (between the two passes), in points (run_extractions)
    std::vector<fdc::sinks::PduRec> pdus;    // the PDUs of the last finished batch
    // fdc_sinks_set_payload_format: what fdc_pdu.samples holds (fdc::IqFormat = FDC_OQ_*), and the route the last finished batch took to it
    int pay_fmt = fdc::kIqFloat;
    float pay_scale = 1.0f;
    int pay_route = 0;
    bool pay_all256 = false;                 // the bank holds 256-bin PowerActivationChannels and nothing else: every extraction it can ever make is k_x256's
    // ================================================================ host engine only (fdc_sinks_host.hip): dev.on == false
    DevBuf<fdc::ExtractTask> d_tasks;
    DevBuf<float2> d_ext;
    PinBuf<cfl> h_ext;                       // pinned landing buffer of the extractions
    std::vector<fdc::ExtractTask> sorted;    // tasks grouped by width class
    std::vector<float> h_power;
    // per-call scratch
    std::vector<fdc::ExtractTask> tasks;
    std::vector<int> task_w, task_skip;
    int64_t ext_used = 0;
    std::vector<std::unique_ptr<fdc::sinks::WorkerLists>> wl;    // one per worker thread (separate heap objects: no shared cache lines)
    fdc::sinks::WorkerPool pool;
    std::string det_logfile;                 // verbose == 2: …vcm_impl.cc:94 / SegmentDetection_impl.cc:51
    int host_threads = 0;                    // cfg.threads, 0 = from the bank's size
    // ================================================================ device engine only (fdc_sinks_dev.hip): decisions, layout and buffered blocks stay on the device
    struct Dev {
        bool on = false;
        int nlist = 0, npw = 0;
        long long max_list = 0;              // longest task list (grid of the scatter kernel)
        std::vector<int64_t> task_base, pdu_base, owner_base, cand_base;
        DevBuf<int64_t> d_task_base, d_pdu_base, d_owner_base, d_cand_base;
        DevBuf<int32_t> d_ntask, d_npdu, d_nowner, d_error, d_class_fill;
        DevBuf<int32_t> d_ncand, d_winoff, d_live, d_live2;
        DevBuf<fdc::DetCh> d_detch;          // tracker scratch: one life record per entry of the owner table
        DevBuf<int64_t> d_live_off;
        DevBuf<int2> d_cand;
        DevBuf<fdc::PacGeom> d_pgeom; DevBuf<fdc::PacState> d_pstate;
        DevBuf<fdc::DetGeom> d_dgeom; DevBuf<fdc::DetSegState> d_sst;
        DevBuf<fdc::SinkTask> d_tasks; DevBuf<fdc::SinkPdu> d_pdus, d_pdus_out; DevBuf<fdc::SinkOwner> d_owners;
        DevBuf<fdc::ExtractTask> d_sorted;
        DevBuf<fdc::SinkSummary> d_sum; PinBuf<fdc::SinkSummary> h_sum;
        PinBuf<fdc::SinkPdu> h_pdus;         // pinned: the first kEagerPdus records travel with the summary
        DevBuf<float2> d_land[2];            // landing buffers (emitted runs, then buffered rests)
        PinBuf<cfl> h_land[2];               // pinned copies of the emitted runs
        // sc16 / sc8 payloads: the emitted runs [0, used_a) once more, narrow, at the same SAMPLE offsets (capacities in bytes); the buffered rests
        // stay float in d_land
        DevBuf<unsigned char> d_nland[2];
        PinBuf<unsigned char> h_nland[2];
        int fmt_of[2] = {0, 0}, route_of[2] = {0, 0};                             // payload format and route (fdc_sinks_payload_route) of the batch in buffer b
        hipStream_t s_copy = nullptr;
        int carry_width = 0;                 // streams that can hold blocks from the call before: every PowerActivationChannel, or a
                                             // segment's live channels (disjoint detect ranges: at most one per power cell)
        hipEvent_t ev_decide = nullptr, ev_extract[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
        std::vector<fdc::SinkPdu> recs[2];
        std::vector<std::pair<int64_t, uint32_t>> order;     // emission order of a batch's records (scratch of dev_build)
        fdc::SinkSummary sum[2];
        int64_t bc0[2] = {0, 0};              // block counter at the start of the batch in landing buffer b
        int nb_of[2] = {0, 0};
        bool pend[2] = {false, false};        // batch in landing buffer b is enqueued and not yet handed out
        int cur = 1;                          // landing buffer of the newest batch
        bool inflight = false;                // some batch is pending
        bool any = false;                     // a batch has run: d_land[cur] holds buffered blocks
        int eager_n = 0;                      // look-ahead: the decision chain of the NEXT batch (prepared, this many blocks) is already enqueued
    } dev;
};

namespace fdc { namespace sinks {

// item index of the order key: from this bit up (fdc_sinks_dev.h)
inline int item_shift(const fdc_sinks *s) { return s->dev.on ? kKeyShiftDev : kKeyShiftHost; }

inline int pow2ceil(int k) { return (int)std::pow(2.0, std::ceil(std::log2((double)k))); }
inline std::string pac_logfile(const Pac &p) { return "gr-FDC.PowActChan." + std::to_string(p.ID) + ".log"; }

// ---- shared by the two engines, defined in fdc_sinks.hip
const std::string &current_time_string();
void sink_log(const fdc_sinks *s, const std::string &file, const std::string &line);
int batch_begin(fdc_sinks *s, int nblocks, bool *have_power);
int batch_end_history(fdc_sinks *s, int nblocks, hipStream_t q);
int batch_end_swap(fdc_sinks *s, hipEvent_t done);
int run_extractions(fdc_sinks *s, const fdc::ExtractTask *d_tasks, const size_t *first, const size_t *cnt, float2 *d_out, bool trace,
                    hipStream_t q0 = nullptr, void *narrow = nullptr, long long used_a = 0);

// ---- the host engine (fdc_sinks_host.hip): one synchronous batch of nblocks blocks from d_spec; the PDUs are in s->pdus when it returns
int host_work_device(fdc_sinks *s, int nblocks);

}}  // namespace fdc::sinks
