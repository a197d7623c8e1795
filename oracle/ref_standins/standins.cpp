// Functional stand-ins for the part of GNU Radio 3.7, pmt, VOLK and boost that the reference's three sink blocks use
// (see README.md).  Written from those libraries' public interfaces.  TEST INFRASTRUCTURE — not product code.
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <gnuradio/fft/fft.h>
#include <gnuradio/sync_block.h>
#include <pmt/pmt.h>
#include <volk/volk.h>

// ---------------------------------------------------------------- gr::basic_block
namespace gr {
basic_block::~basic_block() {}

void basic_block::message_port_register_out(pmt::pmt_t port_id)
{
    if (!pmt::is_symbol(port_id)) throw std::runtime_error("message_port_register_out: port id is not a symbol");
    d_ports.push_back(port_id);
}

void basic_block::message_port_pub(pmt::pmt_t port_id, pmt::pmt_t msg)
{
    std::lock_guard<std::mutex> lock(d_mutex);
    bool known = false;
    for (size_t i = 0; i < d_ports.size(); i++) known = known || pmt::eqv(d_ports[i], port_id);
    if (!known) throw std::runtime_error("message_port_pub: port was not registered");
    d_published.push_back(std::make_pair(port_id, msg));
}

std::vector<std::pair<pmt::pmt_t, pmt::pmt_t> > basic_block::standin_drain()
{
    std::lock_guard<std::mutex> lock(d_mutex);
    std::vector<std::pair<pmt::pmt_t, pmt::pmt_t> > out;
    out.swap(d_published);
    return out;
}
}  // namespace gr

// ---------------------------------------------------------------- pmt
namespace pmt {
static void want(const pmt_t &x, pmt_base::kind_t k, const char *what)
{
    if (!x || x->kind != k) throw std::runtime_error(std::string("pmt: wrong type, expected ") + what);
}
pmt_t intern(const std::string &s) { pmt_t p(new pmt_base(pmt_base::SYMBOL)); p->sym = s; return p; }
pmt_t from_bool(bool val) { pmt_t p(new pmt_base(pmt_base::BOOL)); p->b = val; return p; }
pmt_t from_long(long x) { pmt_t p(new pmt_base(pmt_base::LONG)); p->l = x; return p; }
pmt_t from_double(double x) { pmt_t p(new pmt_base(pmt_base::DOUBLE)); p->d = x; return p; }
pmt_t make_dict() { return pmt_t(new pmt_base(pmt_base::DICT)); }
pmt_t cons(const pmt_t &x, const pmt_t &y) { pmt_t p(new pmt_base(pmt_base::PAIR)); p->car = x; p->cdr = y; return p; }
pmt_t init_c32vector(size_t k, const std::complex<float> *data)
{
    pmt_t p(new pmt_base(pmt_base::C32VECTOR));
    p->c32.assign(data, data + k);
    return p;
}
pmt_t init_c32vector(size_t k, const std::vector<std::complex<float> > &data)
{
    if (k > data.size()) throw std::runtime_error("pmt: init_c32vector longer than its data");
    return init_c32vector(k, data.data());
}
bool is_symbol(const pmt_t &x) { return x && x->kind == pmt_base::SYMBOL; }
bool eqv(const pmt_t &x, const pmt_t &y)
{
    if (x == y) return true;
    if (!x || !y || x->kind != y->kind) return false;
    switch (x->kind) {
    case pmt_base::SYMBOL: return x->sym == y->sym;      // interned symbols of equal spelling are one object in pmt
    case pmt_base::BOOL: return x->b == y->b;
    case pmt_base::LONG: return x->l == y->l;
    case pmt_base::DOUBLE: return x->d == y->d;
    default: return false;
    }
}
pmt_t dict_add(const pmt_t &dict, const pmt_t &key, const pmt_t &value)
{
    want(dict, pmt_base::DICT, "dict");
    pmt_t p(new pmt_base(pmt_base::DICT));
    p->items = dict->items;
    for (size_t i = 0; i < p->items.size(); i++)
        if (eqv(p->items[i].first, key)) { p->items[i].second = value; return p; }
    p->items.push_back(std::make_pair(key, value));
    return p;
}
std::string symbol_to_string(const pmt_t &x) { want(x, pmt_base::SYMBOL, "symbol"); return x->sym; }
bool to_bool(const pmt_t &x) { want(x, pmt_base::BOOL, "bool"); return x->b; }
long to_long(const pmt_t &x) { want(x, pmt_base::LONG, "long"); return x->l; }
double to_double(const pmt_t &x) { want(x, pmt_base::DOUBLE, "double"); return x->d; }
pmt_t car(const pmt_t &x) { want(x, pmt_base::PAIR, "pair"); return x->car; }
pmt_t cdr(const pmt_t &x) { want(x, pmt_base::PAIR, "pair"); return x->cdr; }
bool dict_has_key(const pmt_t &dict, const pmt_t &key)
{
    want(dict, pmt_base::DICT, "dict");
    for (size_t i = 0; i < dict->items.size(); i++) if (eqv(dict->items[i].first, key)) return true;
    return false;
}
pmt_t dict_ref(const pmt_t &dict, const pmt_t &key, const pmt_t &not_found)
{
    want(dict, pmt_base::DICT, "dict");
    for (size_t i = 0; i < dict->items.size(); i++) if (eqv(dict->items[i].first, key)) return dict->items[i].second;
    return not_found;
}
const std::complex<float> *c32vector_elements(const pmt_t &x, size_t &len)
{
    want(x, pmt_base::C32VECTOR, "c32vector");
    len = x->c32.size();
    return x->c32.data();
}
}  // namespace pmt

// ---------------------------------------------------------------- gr::fft::fft_complex
namespace gr {
namespace fft {
fft_complex::fft_complex(int fft_size, bool forward, int) : d_n(fft_size), d_forward(forward)
{
    if (fft_size < 1 || (fft_size & (fft_size - 1))) throw std::invalid_argument("fft_complex stand-in: size must be a power of two");
    d_in.assign((size_t)d_n, gr_complex(0.0f, 0.0f));
    d_out.assign((size_t)d_n, gr_complex(0.0f, 0.0f));
    d_work.resize((size_t)d_n);
    d_tw.resize((size_t)(d_n / 2 > 0 ? d_n / 2 : 1));
    const double sign = forward ? -1.0 : 1.0;
    for (int k = 0; k < d_n / 2; k++) {
        const double a = sign * 2.0 * M_PI * (double)k / (double)d_n;
        d_tw[(size_t)k] = std::complex<double>(std::cos(a), std::sin(a));
        if (4 * k == d_n) d_tw[(size_t)k] = std::complex<double>(0.0, sign);      // the quarter turn exactly: cos(pi / 2) is not 0 in double,
                                                                                  // and a payload that cancels to zero must come out as zero
    }
}

fft_complex::~fft_complex() {}

void fft_complex::execute()     // iterative radix-2, decimation in time, double precision throughout
{
    const int n = d_n;
    int bits = 0;
    while ((1 << bits) < n) bits++;
    for (int i = 0; i < n; i++) {
        int r = 0;
        for (int b = 0; b < bits; b++) if (i & (1 << b)) r |= 1 << (bits - 1 - b);
        d_work[(size_t)r] = std::complex<double>((double)d_in[(size_t)i].real(), (double)d_in[(size_t)i].imag());
    }
    for (int len = 2; len <= n; len <<= 1) {
        const int half = len / 2, step = n / len;
        for (int base = 0; base < n; base += len)
            for (int k = 0; k < half; k++) {
                const std::complex<double> w = d_tw[(size_t)(k * step)], lo = d_work[(size_t)(base + k)], hi = d_work[(size_t)(base + k + half)];
                const std::complex<double> t(w.real() * hi.real() - w.imag() * hi.imag(), w.real() * hi.imag() + w.imag() * hi.real());
                d_work[(size_t)(base + k)] = lo + t;
                d_work[(size_t)(base + k + half)] = lo - t;
            }
    }
    for (int i = 0; i < n; i++) d_out[(size_t)i] = gr_complex((float)d_work[(size_t)i].real(), (float)d_work[(size_t)i].imag());
}
}  // namespace fft
}  // namespace gr

// ---------------------------------------------------------------- VOLK, generic kernels
size_t volk_get_alignment(void) { return 64; }

void *volk_malloc(size_t size, size_t alignment)
{
    void *p = 0;
    if (alignment < sizeof(void *)) alignment = sizeof(void *);
    if (posix_memalign(&p, alignment, size ? size : 1) != 0) return 0;
    return p;
}

void volk_free(void *aptr) { free(aptr); }

void volk_32fc_x2_multiply_32fc(lv_32fc_t *c, const lv_32fc_t *a, const lv_32fc_t *b, unsigned int num_points)
{
    for (unsigned int i = 0; i < num_points; i++) {      // (ar br - ai bi) + i (ar bi + ai br), each product rounded on its own
        const float ar = a[i].real(), ai = a[i].imag(), br = b[i].real(), bi = b[i].imag();
        c[i] = lv_32fc_t(ar * br - ai * bi, ar * bi + ai * br);
    }
}

void volk_32fc_magnitude_squared_32f(float *m, const lv_32fc_t *x, unsigned int num_points)
{
    for (unsigned int i = 0; i < num_points; i++) {
        const float re = x[i].real(), im = x[i].imag();
        m[i] = re * re + im * im;
    }
}

void volk_32f_x2_divide_32f(float *c, const float *a, const float *b, unsigned int num_points)
{
    for (unsigned int i = 0; i < num_points; i++) c[i] = a[i] / b[i];
}

void volk_32f_s32f_multiply_32f(float *c, const float *a, const float scalar, unsigned int num_points)
{
    for (unsigned int i = 0; i < num_points; i++) c[i] = a[i] * scalar;
}

void volk_32f_accumulator_s32f(float *result, const float *in, unsigned int num_points)
{
    float acc = 0.0f;                                     // index order, one float32 accumulator
    for (unsigned int i = 0; i < num_points; i++) acc += in[i];
    *result = acc;
}
