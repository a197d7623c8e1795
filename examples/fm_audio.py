#!/usr/bin/env python3
"""The narrow-band receive chain of a whole band on the device, down to the audio: 16 FM carriers, each modulated by a tone of its own, a few bins of
N off their slice centres and at different strengths.  Per call: an AFC set from the lag-1 correlation (examples/afc.py) pulls every carrier to DC,
an AGC set from the levels (examples/agc.py) brings every channel to one power, the discriminator demodulates (Pipeline.set_demod("fm")), and the
audio filter behind it (Pipeline.set_audio: a low-pass from lowpass_taps, decimation 8, int16 out) leaves 128 / 8 = 16 samples of 2 bytes per block and
channel to cross the link, where the complex ports were 128 samples of 8 bytes.
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/fm_audio.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_fdc_amd as G  # noqa: E402

N, R, C, nblocks, calls, D = 16384, 2, 16, 16, 8, 8
H, l = N - N // R, 256
plan = [(1024 * c + 256, l, 0.88, 1.0) for c in range(C)]            # 256-bin slices: lout = 128 output samples per block
pipe = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nblocks)
lout = pipe.lout[0]

# one FM carrier per channel: off[c] bins of N above the slice centre, amplitude amp[c], deviation dev bins of N, modulated by a tone of fm[c] cycles
# per OUTPUT sample (inside the audio filter's passband: below 0.5 / D)
rng = np.random.default_rng(5)
off, fm, amp, dev = rng.uniform(-6.0, 6.0, C), rng.uniform(0.01, 0.04, C), 10.0 ** rng.uniform(-2.0, 0.0, C), 10.0
t = np.arange(calls * nblocks * H, dtype=np.float64)
x = 1e-4 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
for c, (f, _l, _p, _s) in enumerate(plan):
    f_in = fm[c] * l / N                                              # the modulating tone in cycles per input sample
    phase = ((f + l / 2 + off[c]) / N - 0.5) * t - dev / N / (2 * np.pi * f_in) * np.cos(2 * np.pi * f_in * t)
    x += amp[c] * np.exp(2j * np.pi * phase)                          # instantaneous frequency: carrier + (dev / N) sin(2 pi f_in t)
x = x.astype(np.complex64)

MU, TARGET = 0.7, 1.0
nu, gains = np.zeros(C), np.ones(C)
pipe.set_lag1(True)                                                   # the AFC's measurement
pipe.set_levels(True)                                                 # the AGC's
pipe.set_demod("fm", 1.0 / (2.0 * np.pi))                             # cycles per output sample
SCALE = 32767.0 / (2.0 * dev / l)                                     # full scale at twice the deviation sent
pipe.set_audio(D, G.lowpass_taps(D, 64), "s16", SCALE)                # the ports are int16 at an eighth of the channel rate from here on
audio = [[] for _ in range(C)]
print("call   bytes to the host   largest |mean of the audio| (cycles per output sample: what is left of the carrier offsets)   gains (min .. max)")
for k in range(calls):
    outs = pipe.work(x[k * nblocks * H:(k + 1) * nblocks * H])
    print("%4d   %17d   %.6f   %.2f .. %.2f" % (k, sum(o.nbytes for o in outs), max(abs(float(o.mean())) for o in outs) / SCALE, gains.min(), gains.max()))
    for c, o in enumerate(outs):
        audio[c].append(o)
    nu += MU * G.lag1_frequency(pipe.lag1().mean(axis=0))
    pipe.set_fine_tuning(nu)
    power = pipe.levels()[:, :, 0].mean(axis=0) / lout                # mean power per sample of the gained samples
    gains *= np.sqrt(TARGET / np.maximum(power, 1e-30)) ** MU
    pipe.set_gains(gains)

# the last two calls of every channel: the strongest line of the audio spectrum against the modulating tone (in cycles per CHANNEL sample), the peak
print("channel   modulating tone   strongest audio line   peak deviation (bins of N; sent: %.1f)" % dev)
for c in range(C):
    a = np.concatenate(audio[c][-2:]).astype(np.float64) / SCALE
    a -= a.mean()
    spec = np.abs(np.fft.rfft(a * np.hanning(a.size)))
    print("%7d   %15.5f   %20.5f   %14.2f" % (c, fm[c], np.argmax(spec) / a.size / D, np.percentile(np.abs(a), 99.0) * l))
print(pipe.describe())
