// TEST INFRASTRUCTURE. C-ABI driver around the reference's OWN three throughput-chain blocks (overlap_save, vector_cut_vxx,
// phase_shifting_windowing_vcc), the sibling of ref_sinks_driver.cpp.  The reference's *_impl.cc files are compiled unmodified
// from where they lie (oracle/Makefile, target `ref`) against the stand-ins of oracle/ref_standins/; nothing of them is copied
// into this repository.  This file only calls the blocks' public make(...) and work(...): one create per block, one work
// (noutput_items and raw pointers, handed to the block's own work() as they are) and one destroy for all of them.
#include <stdexcept>
#include <string>

#include <FDC/overlap_save.h>
#include <FDC/phase_shifting_windowing_vcc.h>
#include <FDC/vector_cut_vxx.h>

namespace {
struct handle { boost::shared_ptr<gr::sync_block> blk; };
thread_local std::string g_error;

template <class F> void *guarded(F make)
{
    try {
        boost::shared_ptr<gr::sync_block> blk = make();     // may throw: nothing is held yet
        handle *h = new handle;
        h->blk = blk;
        return h;
    } catch (const std::exception &e) {                 // the phase window's constructor throws std::invalid_argument
        g_error = e.what();
        return 0;
    }
}
}  // namespace

extern "C" {
const char *ref_chain_last_error(void) { return g_error.c_str(); }

void *ref_overlap_save_create(int itemsize, int outputlen, int overlaplen)
{
    return guarded([&] { return gr::FDC::overlap_save::make(itemsize, outputlen, overlaplen); });
}

void *ref_vector_cut_create(int itemsize, int veclen, int offset, int blocklen)
{
    return guarded([&] { return gr::FDC::vector_cut_vxx::make(itemsize, veclen, offset, blocklen); });
}

void *ref_phase_window_create(int blocklen, int numphasestates, int shifts, float passbw, float stopbw, int windowtype)
{
    return guarded([&] { return gr::FDC::phase_shifting_windowing_vcc::make(blocklen, numphasestates, shifts, passbw, stopbw, windowtype); });
}

void ref_chain_destroy(void *hv) { delete (handle *)hv; }

// one work() call of the block: returns what it returns, or -1 with ref_chain_last_error() set
int ref_chain_work(void *hv, int noutput_items, const void *in, void *out)
{
    handle *h = (handle *)hv;
    try {
        gr_vector_const_void_star ins(1, in);
        gr_vector_void_star outs(1, out);
        return h->blk->work(noutput_items, ins, outs);
    } catch (const std::exception &e) {
        g_error = e.what();
        return -1;
    }
}
}  // extern "C"
