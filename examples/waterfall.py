#!/usr/bin/env python3
"""The reference's example flowgraph (examples/FDC_example.grc: N = 4096, R = 4, four throughput channels) with its waterfall sink attached:
the hier block's spectrum goes to the waterfall rows on the device, the picture (with a rectangle for one channel's band) is written as a
.npy array of height x 1024 x 3 bytes.

    python examples/waterfall.py [out.npy]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gr_fdc_amd as G        # noqa: E402

N, R, height, blocks = 4096, 4, 256, 512
user = [[0.12, 0.05], [0.22, 0.1], [-0.14, 0.12], [0, 0.081]]
wf = G.Waterfall(N, 1e6, R, 1, 0, -45.0, -20.0, 0, 0, max_items=64)     # WaterfallMsgTagging(loginput = 0, minvaldb = -45, maxvaldb = -20)
fdc = G.FrequencyDomainChannelizer(8, 1, N, R, user, None, 6.0, 1.0, 0.0, 'normalized', 1, False, False, "", False, None, 10.0, 0.005,
                                   1, 0.2, 0, 0, 128, 128, False, max_blocks=64, waterfall=wf)
img = G.WaterfallImage(height)
img.msg({"blockstart": 100, "blockend": 300, "rel_cfreq": 0.12 + 0.5, "rel_bw": 0.05})    # a mark over channel 0's band
rng = np.random.default_rng(0)
H = fdc.inpblocklen
n = np.arange(blocks * H)
# noise at about -40 dB per bin of the 1/N-scaled spectrum (power sigma^2 / N), carriers about 15 dB above it
x = 0.45 * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
for (f, bw) in user:
    m = np.convolve(rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size), np.ones(int(1 / bw)) * bw, "same")
    x += 3.0 * np.exp(2j * np.pi * f * n) * m                                  # crude carriers: noise low-passed to about their bandwidth
x = x.astype(np.complex64)
for k in range(0, blocks, 64):
    ports, rows = fdc.work(x[k * H:(k + 64) * H])
    img.append(rows.rgb)
out = sys.argv[1] if len(sys.argv) > 1 else "waterfall.npy"
np.save(out, img.image)
print("wrote %s: %s, %d rows" % (out, img.image.shape, wf.rows_done()))
