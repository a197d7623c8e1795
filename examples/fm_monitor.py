#!/usr/bin/env python3
"""A band of narrow-band FM carriers demodulated on the device: 16 channels, each carrier frequency-modulated by a tone of its own and sitting a few
bins of N off its slice centre.  An AFC set from the lag-1 correlation (examples/afc.py) pulls every carrier to DC, and the discriminator's output
(Pipeline.set_demod("fm", 1 / (2 pi)): cycles per output sample, 4 bytes per sample over the link instead of 8) is each channel's audio: a tone at
its modulation frequency, riding on what the AFC has left of the carrier offset.
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/fm_monitor.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_fdc_amd as G  # noqa: E402

N, R, C, nblocks, calls = 16384, 2, 16, 16, 6
H, l = N - N // R, 256
plan = [(1024 * c + 256, l, 0.88, 1.0) for c in range(C)]            # 256-bin slices: lout = 128 output samples per block
pipe = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nblocks)
lout = pipe.lout[0]

# one FM carrier per channel: off[c] bins of N above the slice centre, deviation dev bins of N, modulated by a tone of fm[c] cycles per OUTPUT sample
rng = np.random.default_rng(5)
off, fm, dev = rng.uniform(-6.0, 6.0, C), rng.uniform(0.01, 0.05, C), 10.0
t = np.arange(calls * nblocks * H, dtype=np.float64)
x = 0.01 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
for c, (f, _l, _p, _s) in enumerate(plan):
    f_in = fm[c] * l / N                                              # the modulating tone in cycles per input sample
    phase = ((f + l / 2 + off[c]) / N - 0.5) * t - dev / N / (2 * np.pi * f_in) * np.cos(2 * np.pi * f_in * t)
    x += np.exp(2j * np.pi * phase)                                   # instantaneous frequency: carrier + (dev / N) sin(2 pi f_in t)
x = x.astype(np.complex64)

MU = 0.7
nu = np.zeros(C)
pipe.set_lag1(True)                                                   # the AFC's measurement, of the complex samples in front of the discriminator
pipe.set_demod("fm", 1.0 / (2.0 * np.pi))                             # the ports are float32 from here on
audio = [[] for _ in range(C)]
print("call   largest |mean of the discriminator's output| over the channels (cycles per output sample: what is left of the carrier offsets)")
for k in range(calls):
    outs = pipe.work(x[k * nblocks * H:(k + 1) * nblocks * H])
    print("%4d   %.6f" % (k, max(abs(float(o.mean())) for o in outs)))
    for c, o in enumerate(outs):
        audio[c].append(o)
    nu += MU * G.lag1_frequency(pipe.lag1().mean(axis=0))
    pipe.set_fine_tuning(nu)

# the last two calls of every channel: the strongest line of the audio spectrum against the modulating tone, and the peak deviation
print("channel   modulating tone   strongest audio line   peak deviation (bins of N; sent: %.1f)" % dev)
for c in range(C):
    a = np.concatenate(audio[c][-2:]).astype(np.float64)
    a -= a.mean()
    spec = np.abs(np.fft.rfft(a * np.hanning(a.size)))
    # (the 99th percentile, not the maximum: a new nu turns the phase of every later sample at once, which the discriminator shows as one spike at
    # the first sample of the call)
    print("%7d   %15.5f   %20.5f   %14.2f" % (c, fm[c], np.argmax(spec) / a.size, np.percentile(np.abs(a), 99.0) * l))
print(pipe.describe())
