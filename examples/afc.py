#!/usr/bin/env python3
"""A per-channel AFC in three lines: 16 channels whose carriers sit up to 8 bins of N off their slice centres and drift, pulled to DC by fine
tuning that is set from the lag-1 correlation the device sums (Pipeline.set_lag1).  The loop never pulls the float streams over the link:
lag1() -> average the call's blocks -> nu += mu * lag1_frequency(mean) -> set_fine_tuning(nu).
Needs libfdc_amd.so (python -c "import __graft_entry__ as g; g.build()").

  python examples/afc.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gr_fdc_amd as G  # noqa: E402

N, R, C, nblocks, calls = 16384, 2, 16, 16, 8
H, l = N - N // R, 256
plan = [(1024 * c + 256, l, 0.88, 1.0) for c in range(C)]            # 256-bin slices: lout = 128 output samples per block
pipe = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nblocks)

# one carrier per channel, off[c] bins of N above the slice centre at the start and drifting by drift[c] bins per call, in noise
rng = np.random.default_rng(5)
off, drift = rng.uniform(-8.0, 8.0, C), rng.uniform(-0.5, 0.5, C)
t = np.arange(calls * nblocks * H, dtype=np.float64)
x = 0.05 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
for c, (f, _l, _p, _s) in enumerate(plan):
    bins = f + l / 2 + off[c] + drift[c] * t / (nblocks * H) / 2     # (a chirp: the phase is the integral of the frequency)
    x += np.exp(2j * np.pi * (bins / N - 0.5) * t)                   # spectrum position b <-> frequency b / N - 0.5 (DC at the middle bin)
x = x.astype(np.complex64)

MU = 0.7                                                             # the loop gain: the caller's, like every time constant here
nu = np.zeros(C)
pipe.set_lag1(True)
print("call   largest |residual| over the channels (cycles per output sample)")
for k in range(calls):
    pipe.work(x[k * nblocks * H:(k + 1) * nblocks * H])
    est = G.lag1_frequency(pipe.lag1().mean(axis=0))                 # one complex float32 per (block, channel) came back; their mean per channel
    print("%4d   %.6f" % (k, np.abs(est).max()))
    nu += MU * est                                                   # the estimate is the residual left by the nu in force: it adds
    pipe.set_fine_tuning(nu)
print("nu in force, in bins of N:", np.round(nu * l, 3))          # one bin of N is 1 / l cycles per output sample
print("carrier offsets at the end:", np.round(off + drift * calls, 3))
print(pipe.describe())
