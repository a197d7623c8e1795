#!/usr/bin/env python3
"""A band monitor with a tone squelch ON THE DEVICE: the chain of examples/fm_ctcss.py (16 channels of 25 kHz, FM demodulation, two carriers with a
different CTCSS tone each, the other channels noise), but the decision no longer comes home.  Pipeline.set_tone_squelch puts thresholds on the frame
rows of the wanted tone; the decision of every completed frame gates the carrier squelch's mask from the next frame on, and with the audio packing on
only the audio of the channel that carries the WANTED tone crosses the link: the carrier with the other tone opens the carrier squelch and sends
nothing.  The latency is one frame (here 32 blocks, 0.16 s) by construction: a call of 16 blocks completes a frame every second time.
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/fm_tone_squelch.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_fdc_amd as G  # noqa: E402

N, R, C, nblocks, calls = 16384, 2, 16, 16, 12
H, l = N - N // R, 256
FS = 1.6e6                                                            # input rate: 256-bin slices give lout = 128 samples per block, 25 kHz a channel
plan = [(1024 * c + 256, l, 0.88, 1.0) for c in range(C)]
pipe = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nblocks)
lout = pipe.lout[0]
RATE = FS * lout / H
GROUP, FRAME, DECIM, WANTED = 16, 32, 4, 100.0

# two carriers over the whole stream: channel -> (CTCSS tone in Hz, its deviation in Hz); speech is a slow sine of 2.5 kHz deviation
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

pipe.set_levels(True)
pipe.set_demod("fm", 1.0 / (2.0 * np.pi))                             # cycles per channel sample: a deviation of d Hz is an amplitude of d / RATE
pipe.set_audio(DECIM, G.lowpass_taps(DECIM, 64))
pipe.set_squelch(*G.squelch_thresholds(pipe.lout, -30.0, -36.0), hang=2)               # the carrier squelch: both carriers open it, the noise does not
pipe.set_audio_packing(True)
pipe.set_tones(G.tone_increments(tones, RATE, GROUP), GROUP, FRAME)   # the same 50 tones in every channel
sel = int(np.argmin(np.abs(tones - WANTED)))
# open at half the wanted tone's nominal deviation, close at a quarter; the tone must also have 4 times the power of any tone 3 or more places away
thr_open = G.tone_squelch_thresholds(250.0 / RATE, lout, FRAME, GROUP, WANTED, RATE)
thr_close = G.tone_squelch_thresholds(125.0 / RATE, lout, FRAME, GROUP, WANTED, RATE)
pipe.set_tone_squelch(sel, thr_open, thr_close, ratio=4.0, guard=2, hang=1)
print("call   frames decided open (channel: frames)        open cells by channel (carrier AND tone)      audio samples home")
total = 0
for k in range(calls):
    audio = pipe.work(x[k * nblocks * H:(k + 1) * nblocks * H])       # per channel the audio of its open blocks only
    dec, mask = pipe.tone_squelch(), pipe.squelch()
    frames = ", ".join("%d: %d of %d" % (c, dec[:, c].sum(), dec.shape[0]) for c in range(C) if dec[:, c].any())
    cells = ", ".join("%d: %d" % (c, mask[:, c].sum()) for c in range(C) if mask[:, c].any())
    n = sum(a.size for a in audio)
    total += n
    print("%4d   %-45s %-45s %d" % (k, frames or "none", cells or "none", n))
print("carriers: " + ", ".join("channel %d with %.1f Hz" % (c, f) for c, (f, _d) in keyed.items()) + "; wanted: %.1f Hz" % WANTED)
print("audio samples home: %d of the %d an ungated monitor would fetch" % (total, calls * nblocks * C * lout // DECIM))
print(pipe.describe())
