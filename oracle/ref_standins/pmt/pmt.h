// functional stand-in (see ../README.md): pmt/pmt.h — a small reference-counted variant with the constructors the sink
// blocks call and the accessors the driver needs.  A dictionary is an ordered list of (key, value) pairs; dict_add returns
// a new dictionary and replaces the value of a key that is already there, as pmt does.
#pragma once
#include <complex>
#include <string>
#include <utility>
#include <vector>
#include <boost/shared_ptr.hpp>
namespace pmt {
class pmt_base {
public:
    enum kind_t { SYMBOL, BOOL, LONG, DOUBLE, PAIR, DICT, C32VECTOR };
    kind_t kind;
    std::string sym;
    bool b;
    long l;
    double d;
    boost::shared_ptr<pmt_base> car, cdr;
    std::vector<std::pair<boost::shared_ptr<pmt_base>, boost::shared_ptr<pmt_base> > > items;
    std::vector<std::complex<float> > c32;
    explicit pmt_base(kind_t k) : kind(k), b(false), l(0), d(0.0) {}
};
typedef boost::shared_ptr<pmt_base> pmt_t;
pmt_t intern(const std::string &s);
pmt_t from_bool(bool val);
pmt_t from_long(long x);
pmt_t from_double(double x);
pmt_t make_dict();
pmt_t dict_add(const pmt_t &dict, const pmt_t &key, const pmt_t &value);
pmt_t cons(const pmt_t &x, const pmt_t &y);
pmt_t init_c32vector(size_t k, const std::complex<float> *data);
pmt_t init_c32vector(size_t k, const std::vector<std::complex<float> > &data);
// accessors (each throws std::runtime_error on the wrong kind, like pmt::wrong_type)
bool is_symbol(const pmt_t &x);
bool eqv(const pmt_t &x, const pmt_t &y);
std::string symbol_to_string(const pmt_t &x);
bool to_bool(const pmt_t &x);
long to_long(const pmt_t &x);
double to_double(const pmt_t &x);
pmt_t car(const pmt_t &x);
pmt_t cdr(const pmt_t &x);
bool dict_has_key(const pmt_t &dict, const pmt_t &key);
pmt_t dict_ref(const pmt_t &dict, const pmt_t &key, const pmt_t &not_found);
const std::complex<float> *c32vector_elements(const pmt_t &x, size_t &len);
}  // namespace pmt
