#!/usr/bin/env python3
"""A band monitor with a tone squelch: the band of examples/fm_squelch.py (16 channels of 25 kHz, FM demodulation on the device), two keyed carriers,
each with a different CTCSS tone under its modulation, the other channels noise.  The tone bank (Pipeline.set_tones) measures all 50 standard tones
in every channel on the device, over frames of 32 blocks (0.16 s); what comes home per frame is 50 complex numbers a channel, not the demodulated
ports.  The decision stays on the host: a channel carries a tone when the strongest of the 50 has at least RATIO times the median tone's power, and
the speaker opens only for the channel that carries the WANTED tone.
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/fm_ctcss.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_fdc_amd as G  # noqa: E402

N, R, C, nblocks, calls = 16384, 2, 16, 16, 8
H, l = N - N // R, 256
FS = 1.6e6                                                            # input rate: 256-bin slices give lout = 128 samples per block, 25 kHz a channel
plan = [(1024 * c + 256, l, 0.88, 1.0) for c in range(C)]
pipe = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nblocks)
lout = pipe.lout[0]
RATE = FS * lout / H
GROUP, FRAME, RATIO, WANTED = 16, 32, 30.0, 100.0

# two keyed carriers over the whole stream: channel -> (CTCSS tone in Hz, its deviation in Hz); speech is a slow sine of 2.5 kHz deviation
tones = G.ctcss_tones()
keyed = {5: (100.0, 500.0), 12: (151.4, 500.0)}
rng = np.random.default_rng(5)
t = np.arange(calls * nblocks * H, dtype=np.float64)
x = 1e-3 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
for c, (f_tone, dev_tone) in keyed.items():
    f_speech, dev_speech = rng.uniform(400.0, 900.0), 2500.0
    phase = ((plan[c][0] + l / 2) / N - 0.5) * t
    for f_mod, dev in ((f_speech, dev_speech), (f_tone, dev_tone)):
        phase -= dev / f_mod / (2 * np.pi) * np.cos(2 * np.pi * f_mod * t / FS)       # the integral of dev sin(2 pi f_mod t / FS) / FS, in cycles
    x += 0.3 * np.exp(2j * np.pi * phase)
x = x.astype(np.complex64)

pipe.set_demod("fm", 1.0 / (2.0 * np.pi))                             # cycles per channel sample: a deviation of d Hz is an amplitude of d / RATE
pipe.set_tones(G.tone_increments(tones, RATE, GROUP), GROUP, FRAME)   # the same 50 tones in every channel
print("frame   channel: detected tone (amplitude as deviation in Hz)                  speaker")
frame = 0
for k in range(calls):
    pipe.work(x[k * nblocks * H:(k + 1) * nblocks * H])
    for Z in pipe.tones():                                            # complex64 [C, 50] per completed frame; most calls complete none or one
        power = np.abs(Z.astype(np.complex128)) ** 2
        best = power.argmax(axis=1)
        found = power[np.arange(C), best] >= RATIO * np.median(power, axis=1)
        amp = G.tone_amplitude(Z[np.arange(C), best], FRAME * lout, tones[best], RATE, GROUP) * RATE
        seen = ", ".join("%d: %.1f Hz (%.0f)" % (c, tones[best[c]], amp[c]) for c in range(C) if found[c])
        speaker = [c for c in range(C) if found[c] and tones[best[c]] == WANTED]
        print("%5d   %-70s %s" % (frame, seen or "none", ", ".join("channel %d" % c for c in speaker) or "closed"))
        frame += 1
print("keyed: " + ", ".join("channel %d with %.1f Hz" % (c, f) for c, (f, _d) in keyed.items()) + "; wanted: %.1f Hz" % WANTED)
print(pipe.describe())
