// functional stand-in (see ../../README.md): gnuradio/fft/fft.h — gr::fft::fft_complex as an unnormalised DFT of a power-of-two
// length, sign by `forward`.  The transform runs in DOUBLE and is rounded to float once: a run through these stand-ins gives
// the high-precision answer, not a third float32 FFT with an error of its own.
#pragma once
#include <complex>
#include <vector>
typedef std::complex<float> gr_complex;
namespace gr {
namespace fft {
class fft_complex {
    int d_n;
    bool d_forward;
    std::vector<gr_complex> d_in, d_out;
    std::vector<std::complex<double> > d_tw, d_work;
public:
    fft_complex(int fft_size, bool forward = true, int nthreads = 1);
    virtual ~fft_complex();
    gr_complex *get_inbuf() { return d_in.data(); }
    gr_complex *get_outbuf() { return d_out.data(); }
    void execute();
};
}  // namespace fft
}  // namespace gr
