// TEST INFRASTRUCTURE. C-ABI driver around the reference's OWN three sink blocks (PowerActivationChannel,
// activity_detection_channelizer_vcm, SegmentDetection), the sibling of ref_windows_driver.cpp.
// The reference's *_impl.cc files are compiled unmodified from where they lie (oracle/Makefile, target `ref`) against the
// functional stand-ins of oracle/ref_standins/; nothing of them is copied into this repository.  This file only calls the
// blocks' public make(...) and work(...), and flattens the PDUs they publish into the fdco_pdu layout of fdc_oracle.h, so
// that one Python comparison serves oracle, reference and device.  File output off, verbose 0, message output on.
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <FDC/PowerActivationChannel.h>
#include <FDC/SegmentDetection.h>
#include <FDC/activity_detection_channelizer_vcm.h>

#include "fdc_oracle.h"

namespace {
struct handle {
    boost::shared_ptr<gr::sync_block> blk;
    int kind;          // 0 = PowerActivationChannel, 1 = the two detection blocks
    int blocklen;
};
thread_local std::string g_error;

template <class F> handle *guarded(F make, int kind, int blocklen)
{
    try {
        boost::shared_ptr<gr::sync_block> blk = make();     // may throw: nothing is held yet
        handle *h = new handle;
        h->blk = blk;
        h->kind = kind;
        h->blocklen = blocklen;
        return h;
    } catch (const std::exception &e) {                 // the reference's constructors throw std::invalid_argument
        g_error = e.what();
        return 0;
    }
}

long get_long(const pmt::pmt_t &dict, const char *key, long absent)
{
    const pmt::pmt_t k = pmt::intern(key);
    return pmt::dict_has_key(dict, k) ? pmt::to_long(pmt::dict_ref(dict, k, pmt::pmt_t())) : absent;
}
}  // namespace

// the list Python drains: fdco_pdu_list, then the untouched ID string of every PDU
struct ref_pdu_list { fdco_pdu *pdu; int n, cap; char **ids; };

extern "C" {
const char *ref_sinks_last_error(void) { return g_error.c_str(); }

void *ref_pac_create(int blocklen, float cfreq, float bw, int relinvovl, float thresh_db, int maxblocks, int deactivation_delay, int ID)
{
    return guarded([&] { return gr::FDC::PowerActivationChannel::make(blocklen, cfreq, bw, relinvovl, thresh_db, maxblocks, deactivation_delay,
                                                                      true, false, std::string(""), 0, ID); }, 0, blocklen);
}

void *ref_vcm_create(int blocklen, int nseg, const float *segs, float thresh_db, int relinvovl, int maxblocks, float minchandist,
                     int deactivation_delay, double window_flank_puffer, int threads)
{
    std::vector<std::vector<float> > s;
    for (int i = 0; i < nseg; i++) s.push_back(std::vector<float>(segs + 2 * i, segs + 2 * i + 2));
    return guarded([&] { return gr::FDC::activity_detection_channelizer_vcm::make(blocklen, s, thresh_db, relinvovl, maxblocks, true, false,
                                                                                  std::string(""), threads != 0, minchandist,
                                                                                  deactivation_delay, window_flank_puffer, 0); }, 1, blocklen);
}

void *ref_sd_create(int ID, int blocklen, int relinvovl, float seg_start, float seg_stop, float thresh_db, float minchandist,
                    float window_flank_puffer, int maxblocks, int deactivation_delay, int threads)
{
    return guarded([&] { return gr::FDC::SegmentDetection::make(ID, blocklen, relinvovl, seg_start, seg_stop, thresh_db, minchandist,
                                                                window_flank_puffer, maxblocks, deactivation_delay, true, false,
                                                                std::string(""), threads != 0, 0); }, 1, blocklen);
}

void ref_sinks_destroy(void *hv) { delete (handle *)hv; }

// work() over `nitems` spectrum items, `per_call` items per call (<= 0: all in one call); returns the items consumed or -1
int ref_sinks_work(void *hv, const float *items, int nitems, int per_call)
{
    handle *h = (handle *)hv;
    if (per_call <= 0) per_call = nitems;
    try {
        int done = 0;
        while (done < nitems) {
            const int n = nitems - done < per_call ? nitems - done : per_call;
            gr_vector_const_void_star in(1, (const void *)(items + 2 * (size_t)done * (size_t)h->blocklen));
            gr_vector_void_star out(1, (void *)0);      // no output stream; one null entry, since one block names output_items[0]
            const int rc = h->blk->work(n, in, out);
            if (rc != n) throw std::runtime_error("work() did not consume its items");
            done += n;
        }
        return done;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -1;
    }
}

void ref_sinks_list_clear(ref_pdu_list *L)
{
    for (int i = 0; i < L->n; i++) { free(L->pdu[i].samples); free(L->ids[i]); }
    free(L->pdu); free(L->ids);
    L->pdu = 0; L->ids = 0; L->n = 0; L->cap = 0;
}

// everything published since the last drain, in publication order; returns the count or -1
int ref_sinks_drain(void *hv, ref_pdu_list *L)
{
    handle *h = (handle *)hv;
    L->pdu = 0; L->ids = 0; L->n = 0; L->cap = 0;
    try {
        const std::vector<std::pair<pmt::pmt_t, pmt::pmt_t> > msgs = h->blk->standin_drain();
        const int n = (int)msgs.size();
        L->pdu = (fdco_pdu *)calloc((size_t)(n > 0 ? n : 1), sizeof(fdco_pdu));
        L->ids = (char **)calloc((size_t)(n > 0 ? n : 1), sizeof(char *));
        L->cap = n;
        for (int i = 0; i < n; i++) {
            if (pmt::symbol_to_string(msgs[(size_t)i].first) != "msgout") throw std::runtime_error("message on an unexpected port");
            const pmt::pmt_t dict = pmt::car(msgs[(size_t)i].second), vec = pmt::cdr(msgs[(size_t)i].second);
            fdco_pdu *p = &L->pdu[i];
            const std::string id = pmt::symbol_to_string(pmt::dict_ref(dict, pmt::intern("ID"), pmt::pmt_t()));
            L->ids[i] = strdup(id.c_str());
            p->kind = h->kind;
            p->source = -1; p->chan_id = -1;            // both are part of the ID string; oracle.py reads them from there
            p->finalized = pmt::to_bool(pmt::dict_ref(dict, pmt::intern("finalized"), pmt::pmt_t())) ? 1 : 0;
            p->has_part = pmt::dict_has_key(dict, pmt::intern("part")) ? 1 : 0;
            p->part = (int)get_long(dict, "part", 0);
            p->rel_bw = pmt::to_double(pmt::dict_ref(dict, pmt::intern("rel_bw"), pmt::pmt_t()));
            p->rel_cfreq = pmt::to_double(pmt::dict_ref(dict, pmt::intern("rel_cfreq"), pmt::pmt_t()));
            p->blockstart = get_long(dict, "blockstart", -1);
            p->blockend = get_long(dict, "blockend", -1);
            p->vectorstart = get_long(dict, "vectorstart", -1);      // -1: the dictionary has no such key (PowerActivationChannel)
            p->vectorend = get_long(dict, "vectorend", -1);
            size_t len = 0;
            const std::complex<float> *d = pmt::c32vector_elements(vec, len);
            p->nsamples = (long)len;
            p->samples = (float *)malloc(sizeof(float) * 2 * (len > 0 ? len : 1));
            if (len > 0) memcpy(p->samples, d, sizeof(float) * 2 * len);
            L->n = i + 1;
        }
        return n;
    } catch (const std::exception &e) {
        g_error = e.what();
        ref_sinks_list_clear(L);
        return -1;
    }
}
}  // extern "C"
