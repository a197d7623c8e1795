#!/usr/bin/env python3
"""A band to 48 kHz int16: 16 FM carriers in 256-bin channels of a 16384-point plan at fs = 1.6 MHz, so the channel rate is fs l / N = 25 kHz, from
which no integer decimation reaches a standard audio rate.  The audio resampler (Pipeline.set_audio_resampler) takes every demodulated port to
48 kHz on the device: audio_resample_ratio(25000, 48000) is 48 / 25, resampler_taps designs the low-pass, and work() returns the valid samples of
every call, whose counts vary from call to call (48 / 25 of 128 samples is 245.76 per block) and add up to the rate exactly.
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/fm_audio_48k.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_fdc_amd as G  # noqa: E402

FS, N, R, C, nblocks, calls = 1.6e6, 16384, 2, 16, 10, 5
H, l = N - N // R, 256
plan = [(1024 * c + 256, l, 0.88, 1.0) for c in range(C)]            # 256-bin slices: lout = 128 output samples per block
pipe = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nblocks)
rate_in = FS * l / N                                                  # 25 kHz
up, down = G.audio_resample_ratio(rate_in, 48000)                    # (48, 25), exact and reduced
print("channel rate %.0f Hz -> 48000 Hz: up %d, down %d" % (rate_in, up, down))

rng = np.random.default_rng(7)
tone = rng.uniform(300.0, 3000.0, C)                                  # the audio tone every carrier is modulated with, Hz
dev = 2500.0                                                          # peak deviation, Hz
t = np.arange(calls * nblocks * H, dtype=np.float64) / FS
x = 1e-3 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
for c in range(C):
    fc = ((plan[c][0] + l / 2) / N - 0.5) * FS
    x += 0.1 * np.exp(2j * np.pi * (fc * t - dev / (2 * np.pi * tone[c]) * np.cos(2 * np.pi * tone[c] * t)))
x = x.astype(np.complex64)

pipe.set_demod("fm", rate_in / (2.0 * np.pi))                         # the discriminator in Hz of deviation
pipe.set_audio_resampler(up, down, G.resampler_taps(up, down), "s16", 32767.0 / (2.0 * dev))
audio = [[] for _ in range(C)]
for k in range(calls):
    outs = pipe.work(x[k * nblocks * H:(k + 1) * nblocks * H])        # one int16 array per channel: the valid 48 kHz samples of this call
    print("call %d: blocks %d .. %d gave %s samples per channel" % (k, k * nblocks, (k + 1) * nblocks - 1, sorted(set(o.size for o in outs))))
    for c, o in enumerate(outs):
        audio[c].append(o)
audio = [np.concatenate(a) for a in audio]
sent = calls * nblocks * H / FS
print("%.4f s of band gave %d samples per channel: %.1f Hz" % (sent, audio[0].size, audio[0].size / sent))
print("channel   tone sent (Hz)   tone found at 48 kHz (Hz)   peak (int16)")
for c in range(C):
    a = audio[c][2000:].astype(np.float64)                            # (behind the filter's start)
    spec = np.abs(np.fft.rfft(a * np.hanning(a.size)))
    print("%7d   %14.1f   %25.1f   %12d" % (c, tone[c], (np.argmax(spec[1:]) + 1) * 48000.0 / a.size, np.abs(audio[c]).max()))
print(pipe.describe())
