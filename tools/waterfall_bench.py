#!/usr/bin/env python3
"""Cost of the waterfall rows on the example flowgraph's plan (examples/FDC_example.grc: N = 4096, R = 4, l = 256 / 512 / 1024 / 512).

  (a) fdc_pipeline_work, no rows                              (path 5, k_f4096)
  (b) fdc_pipeline_work_waterfall, rows from the fused epilogue (path 5, k_f4096 ROWS form + k_wf_finish)
  (c) the alternative without it: the spectrum in memory (two launches, k_fft4096 + channel kernels) + k_wf_from_spectrum + k_wf_finish
      (fdc_pipeline_work_waterfall on a handle with FDC_PIPE_NO_FUSED, which is what keep_spectrum + a row kernel costs)

Per variant: the median over --steps calls (after --warmup) of the pipeline's kernels as its HIP events time them (fdc_pipeline_last_kernel_ms:
the transform and channel kernels, not the row kernels, which a rocprofv3 --kernel-trace --stats run of this script shows) and of the whole host
call.  One JSON line.
  python tools/waterfall_bench.py [--blocks 16384] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                   # noqa: E402
import gr_fdc_amd as G                               # noqa: E402

EXAMPLE = [(2412, 256, 0.8, 1.0), (2693, 512, 0.8, 1.0), (963, 1024, 0.8, 1.0), (1792, 512, 0.8, 1.0)]   # the example flowgraph's channels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    N, R, nb = 4096, 4, a.blocks
    H = N - N // R
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H)).astype(np.complex64) * 1e-2
    G.register_host(x)
    res = {"plan": "examples/FDC_example.grc, N = 4096, R = 4", "blocks": nb, "steps": a.steps}
    variants = (("a_no_rows", 0, False), ("b_fused_rows", 0, True), ("c_spectrum_rows", G.FDC_PIPE_NO_FUSED, True))
    for name, flags, rows in variants:
        p = G.Pipeline(N, R, EXAMPLE, windowtype=1, max_blocks=nb, flags=flags)
        w = G.Waterfall(N, 1e6, R, 1, 0, -45.0, -20.0, 0, 0, max_items=nb) if rows else None
        p.enable_timing(True)
        kern, wall = [], []
        for i in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            if rows:
                p.work_waterfall(x, w)
            else:
                p.work(x)
            t1 = time.perf_counter()
            ms = p.last_kernel_ms()
            if i >= a.warmup:
                kern.append(sum(ms[:3]))
                wall.append((t1 - t0) * 1e3)
        res[name] = {"path": p.path(), "describe": p.describe(), "kernel_ms_median": statistics.median(kern),
                     "call_ms_median": statistics.median(wall)}
        p.close()
        if w is not None:
            w.close()
    res["b_over_a_kernel"] = res["b_fused_rows"]["kernel_ms_median"] / res["a_no_rows"]["kernel_ms_median"]
    G.unregister_host(x)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
