#!/usr/bin/env python3
"""A per-channel AGC in three calls: 256 channels of one band whose levels differ by 40 dB, handed out as sc8 (one byte per component).  With the one
scale of set_output_format either the strong channels clip or the weak ones keep a bit or two; with a gain per channel (Pipeline.set_gains) every
channel uses the range.  The loop never pulls the float streams over the link: levels() -> gains -> set_gains().
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/agc.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_fdc_amd as G  # noqa: E402

N, R, C, nblocks = 65536, 2, 256, 32
H = N - N // R
plan = [(256 * c, 256, 0.88, 1.0) for c in range(C)]                 # the 256-bin grid: one block kernel per step
pipe = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nblocks)

# a band whose channels fall by 40 dB from one edge to the other: white noise shaped in the frequency domain
rng = np.random.default_rng(2)
n = 3 * nblocks * H
spec = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
spec *= 10.0 ** (-2.0 * np.fft.fftshift(np.arange(n)) / n)           # -40 dB across the band, in amplitude 10^-2
x = np.fft.ifft(spec).astype(np.complex64)
calls = [x[k * nblocks * H:(k + 1) * nblocks * H] for k in range(3)]

LIMIT, TARGET = 127.5, 0.5                                           # sc8; the AGC aims every channel's peak at half the range
pipe.set_levels(True)


def share(outs):
    """each channel's largest component as a share of the sc8 range"""
    return np.array([np.abs(o.astype(np.int16)).max() / 127.0 for o in outs])


def report(what, outs):
    s = share(outs)
    clipped = int(sum(((o == 127) | (o == -128)).any() for o in outs))
    print("%-34s peak / range: min %5.1f %%, median %5.1f %%, max %5.1f %%; channels at a limit value: %d"
          % (what, 100 * s.min(), 100 * np.median(s), 100 * s.max(), clipped))
    return s


# call 1: one scale for the whole plan, set from a float call's loudest channel (what set_output_format alone can do)
pipe.work(calls[0])
peak = pipe.levels()[:, :, 1].max(axis=0)                            # per channel, over the call's blocks: 2 floats per (block, channel) came back
scale = float(TARGET * LIMIT / peak.max())
pipe.set_output_format("sc8", scale)
pipe.reset()
before = report("one scale, no gains:", pipe.work(calls[0]))

# call 2: the gains from call 1's levels (its levels are those of the samples before the narrowing)
lev = pipe.levels()
gains = TARGET * LIMIT / (lev[:, :, 1].max(axis=0) * scale)
pipe.set_gains(gains)
after = report("gains from the previous call:", pipe.work(calls[1]))

# call 3: the loop closed — with gains on, the levels are those of the GAINED samples, so the correction multiplies the gains in force
lev = pipe.levels()
gains = pipe.gains() * TARGET * LIMIT / (lev[:, :, 1].max(axis=0) * scale)
pipe.set_gains(gains)
report("gains corrected once more:", pipe.work(calls[2]))

print("\nchannel   gain (dB)   peak / range before   after")
for c in range(0, C, 32):
    print("%7d   %9.1f   %18.1f %%   %5.1f %%" % (c, 20 * np.log10(abs(gains[c])), 100 * before[c], 100 * after[c]))
print(pipe.describe())
