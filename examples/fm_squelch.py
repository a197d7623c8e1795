#!/usr/bin/env python3
"""A band monitor with a squelch in front of every speaker: the band of examples/fm_audio.py (16 FM carriers, AGC, FM demodulation, audio filter, all
on the device), but only a few of the carriers are keyed, each for a stretch of its own, and the others are noise.  The squelch
(Pipeline.set_squelch) decides per block and channel on the levels the device has already summed: a channel opens when its mean power in front of
the gain reaches OPEN_DB, stays open while it reaches CLOSE_DB and closes HANG + 1 blocks after it last did.  The audio of closed blocks is zero and
is not filtered; Pipeline.squelch() says which blocks were open.
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/fm_squelch.py
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
OPEN_DB, CLOSE_DB, HANG = -30.0, -36.0, 2                             # dB of mean power per output sample, blocks

# four keyed carriers: channel -> (first block, last block) of the stream in which it transmits; the amplitude differs from carrier to carrier
rng = np.random.default_rng(5)
keyed = {2: (10, 40), 5: (0, 127), 9: (50, 60), 12: (90, 120)}
amp = {c: 10.0 ** rng.uniform(-1.2, -0.2) for c in keyed}
fm, dev = {c: rng.uniform(0.01, 0.04) for c in keyed}, 10.0
t = np.arange(calls * nblocks * H, dtype=np.float64)
x = 1e-3 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
for c, (b0, b1) in keyed.items():
    f = plan[c][0]
    f_in = fm[c] * l / N
    phase = ((f + l / 2) / N - 0.5) * t - dev / N / (2 * np.pi * f_in) * np.cos(2 * np.pi * f_in * t)
    gate = (t >= b0 * H) & (t < (b1 + 1) * H)
    x += gate * amp[c] * np.exp(2j * np.pi * phase)
x = x.astype(np.complex64)

MU, TARGET = 0.7, 1.0
gains = np.ones(C)
pipe.set_levels(True)                                                 # the AGC's measurement, and the squelch's
pipe.set_demod("fm", 1.0 / (2.0 * np.pi))
SCALE = 32767.0 / (2.0 * dev / l)
pipe.set_audio(D, G.lowpass_taps(D, 64), "s16", SCALE)
pipe.set_squelch(*G.squelch_thresholds(pipe.lout, OPEN_DB, CLOSE_DB), hang=HANG)
masks = []
print("call   open channels (blocks open of %d)                     audio samples that are not zero" % nblocks)
for k in range(calls):
    outs = pipe.work(x[k * nblocks * H:(k + 1) * nblocks * H])
    mask = pipe.squelch()                                             # uint8 [nblocks, C]
    masks.append(mask)
    opened = ", ".join("%d (%d)" % (c, n) for c, n in enumerate(mask.sum(axis=0)) if n)
    print("%4d   %-60s %d of %d" % (k, opened or "-", sum(int(np.count_nonzero(o)) for o in outs), sum(o.size for o in outs)))
    # the AGC of examples/agc.py: the thresholds refer to the power in front of the gain, so it does not move them
    power = pipe.levels()[:, :, 0].mean(axis=0) / lout
    gains *= np.sqrt(TARGET / np.maximum(power, 1e-30)) ** MU
    pipe.set_gains(np.clip(gains, 1e-3, 1e3))
    gains = np.clip(gains, 1e-3, 1e3)

mask = np.concatenate(masks)
print("channel   keyed in blocks   open in blocks")
for c in range(C):
    on = np.flatnonzero(mask[:, c])
    runs = np.split(on, np.flatnonzero(np.diff(on) > 1) + 1) if on.size else []
    print("%7d   %-15s   %s" % (c, "%d .. %d" % keyed[c] if c in keyed else "-", ", ".join("%d .. %d" % (r[0], r[-1]) for r in runs) or "-"))
print(pipe.describe())
