#!/usr/bin/env python3
"""A band recorder: the band of examples/fm_squelch.py (16 channels, a few FM carriers keyed each for a stretch of its own, the others noise) with AFC,
AGC, FM demodulation, the audio filter and the squelch on the device, and the audio PACKED (Pipeline.set_audio_packing): only the audio of open
(block, channel) cells crosses the link.  work() hands every channel the audio of its open blocks of the call, which is appended to that channel's own
recording; Pipeline.squelch() says which blocks they were.  Per call the bytes the call copies home are printed, packed and as the whole matrix.
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/fm_record.py
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

rng = np.random.default_rng(5)
keyed = {2: (10, 40), 5: (0, 127), 9: (50, 60), 12: (90, 120)}       # channel -> (first block, last block) in which it transmits
amp = {c: 10.0 ** rng.uniform(-1.2, -0.2) for c in keyed}
off = {c: rng.uniform(-0.5, 0.5) for c in keyed}                     # carrier offsets in bins of N, which the AFC finds
fm, dev = {c: rng.uniform(0.01, 0.04) for c in keyed}, 10.0
t = np.arange(calls * nblocks * H, dtype=np.float64)
x = 1e-3 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
for c, (b0, b1) in keyed.items():
    f_in = fm[c] * l / N
    phase = ((plan[c][0] + l / 2 + off[c]) / N - 0.5) * t - dev / N / (2 * np.pi * f_in) * np.cos(2 * np.pi * f_in * t)
    x += ((t >= b0 * H) & (t < (b1 + 1) * H)) * amp[c] * np.exp(2j * np.pi * phase)
x = x.astype(np.complex64)

MU, TARGET = 0.7, 1.0
gains, nu = np.ones(C), np.zeros(C)
pipe.set_levels(True)                                                 # the AGC's measurement, and the squelch's
pipe.set_lag1(True)                                                   # the AFC's
pipe.set_demod("fm", 1.0 / (2.0 * np.pi))
SCALE = 32767.0 / (2.0 * dev / l)
pipe.set_audio(D, G.lowpass_taps(D, 64), "s16", SCALE)
pipe.set_squelch(*G.squelch_thresholds(pipe.lout, OPEN_DB, CLOSE_DB), hang=HANG)
pipe.set_audio_packing(True)
npb = [lo // D for lo in pipe.lout]                                   # audio samples per block of every channel
recordings = [[] for _ in range(C)]
matrix_bytes = 2 * nblocks * sum(npb)                                 # what the unpacked call copies home as audio (int16)
print("call   openings appended to the recordings (channel: blocks)       audio bytes over the link: packed / unpacked")
for k in range(calls):
    outs = pipe.work(x[k * nblocks * H:(k + 1) * nblocks * H])        # one int16 array per channel: its open blocks of this call
    mask = pipe.squelch()                                             # uint8 [nblocks, C]: which blocks they were
    for c, o in enumerate(outs):
        if o.size:
            recordings[c].append(o)
    opened = ", ".join("%d: %d" % (c, n) for c, n in enumerate(mask.sum(axis=0)) if n)
    print("%4d   %-60s %7d / %d" % (k, opened or "-", sum(o.nbytes for o in outs), matrix_bytes))
    # the AGC of examples/agc.py and the AFC of examples/afc.py, on open channels only: a closed channel's measurements are of noise
    heard = mask.any(axis=0)
    power = pipe.levels()[:, :, 0].mean(axis=0) / lout
    gains = np.clip(np.where(heard, gains * np.sqrt(TARGET / np.maximum(power, 1e-30)) ** MU, gains), 1e-3, 1e3)
    pipe.set_gains(gains)
    lag = np.where(mask != 0, pipe.lag1(), 0).sum(axis=0)
    nu += np.where(heard, MU * G.lag1_frequency(np.where(heard, lag, 1.0)), 0.0)
    pipe.set_fine_tuning(nu)

print("channel   keyed in blocks   recorded samples (blocks)   carrier offset found / sent (bins of N)")
for c in range(C):
    n = sum(o.size for o in recordings[c])
    print("%7d   %-15s   %8d (%3d)              %s" % (c, "%d .. %d" % keyed[c] if c in keyed else "-", n, n // npb[c],
                                                        "%+.3f / %+.3f" % (nu[c] * l, off[c]) if c in keyed else "-"))
print(pipe.describe())
