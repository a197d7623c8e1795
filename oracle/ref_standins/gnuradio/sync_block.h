// functional stand-in (see ../README.md): gnuradio/sync_block.h — a block without a scheduler.  It keeps its name and
// signatures, records the message ports it registers and appends every published message to a list the driver drains.
#pragma once
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include <gnuradio/io_signature.h>
#include <pmt/pmt.h>
namespace gr {
class basic_block {
    std::string d_name;
    io_signature::sptr d_in, d_out;
    std::vector<pmt::pmt_t> d_ports;
    std::vector<std::pair<pmt::pmt_t, pmt::pmt_t> > d_published;
    std::mutex d_mutex;      // the reference's threaded paths publish from several threads
public:
    virtual ~basic_block();
    std::string name() const { return d_name; }
    io_signature::sptr input_signature() const { return d_in; }
    io_signature::sptr output_signature() const { return d_out; }
    void message_port_register_out(pmt::pmt_t port_id);
    void message_port_pub(pmt::pmt_t port_id, pmt::pmt_t msg);   // throws for a port that was never registered
    // driver side (not GNU Radio's interface)
    std::vector<std::pair<pmt::pmt_t, pmt::pmt_t> > standin_drain();
protected:
    basic_block() {}     // for the virtual inheritance of the block faces, as in GNU Radio
    basic_block(const std::string &name, io_signature::sptr in, io_signature::sptr out) : d_name(name), d_in(in), d_out(out) {}
};
class block : public basic_block {
protected:
    block() {}
    block(const std::string &name, io_signature::sptr in, io_signature::sptr out) : basic_block(name, in, out) {}
};
class sync_block : public block {
protected:
    sync_block() {}
    sync_block(const std::string &name, io_signature::sptr in, io_signature::sptr out) : block(name, in, out) {}
public:
    virtual int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items) = 0;
};
}  // namespace gr
namespace gnuradio {
template <class T> boost::shared_ptr<T> get_initial_sptr(T *p) { return boost::shared_ptr<T>(p); }
}  // namespace gnuradio
