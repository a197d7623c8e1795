"""Cost of fine tuning (fdc_pipeline_set_fine_tuning) on the device-resident entry: one JSON line per plan and variant.

Plans: configs[0] (the example flowgraph's 4096-pt plan, 16384 blocks a step: path 5) and configs[1] (65536-pt FFT, R = 2, 256 channels of 256 bins,
2048 blocks a step: the block kernel).  Variants, on the same build:
  off            fine tuning off (what the parent commit runs: on a build without fdc_pipeline_set_fine_tuning only this variant is timed)
  on             fine tuning on: path 5 turns the samples in its own stores (fused), the block kernel gets k_fine_rotate behind it (rotated)
  on_rotated     path 5 only: the same plan under FDC_PIPE_NO_FUSED with fine tuning on (two launches + k_fine_rotate), and off_no_fused beside it
Three input rings per variant, rotated as bench.py does, so the input of a step is cache-cold.  Every variant is timed in --rounds rounds, the order of
the variants rotated from round to round; each timing sits behind --settle-ms of untimed steps and the warm-up.  HIP events on the handle's stream;
ms = the median over the rounds, ms_rounds keeps each one.

usage: python tools/fine_bench.py [--steps 20] [--warmup 3] [--rounds 3] [--settle-ms 150]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(G):
    R = 2
    cfg1 = [(256 * c, 256, 0.88, 1.0) for c in range(256)]
    params = [G.get_opt_channelparams(4096, R, (u + 0.5) % 1.0, bw) for (u, bw) in ((0.12, 0.05), (0.22, 0.1), (-0.14, 0.12), (0.0, 0.081))]
    cfg0 = [(f, l, p, s) for (f, l, _lo, p, s) in params]
    return [("configs[0]", 4096, R, cfg0, 16384), ("configs[1]", 65536, R, cfg1, 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=150.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_fdc_amd as G
    have = hasattr(G.Pipeline, "set_fine_tuning")
    for (name, N, R, plan, nb) in shapes(G):
        H, ovl = N - N // R, N // R
        rng = np.random.default_rng(1)
        base = (rng.standard_normal(2 * (ovl + nb * H)) * 1e-2).astype(np.float32)
        rings = [torch.from_numpy(np.roll(base, 7919 * 2 * k)).cuda() for k in range(3)]
        nu = np.linspace(-0.45, 0.45, len(plan))
        variants = [("off", 0, False)]
        if have:
            variants.append(("on", 0, True))
            if N == 4096:
                variants += [("off_no_fused", G.FDC_PIPE_NO_FUSED, False), ("on_rotated", G.FDC_PIPE_NO_FUSED, True)]
        handles = {}
        for vname, flags, on in variants:
            p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb, flags=flags)
            if on:
                p.set_fine_tuning(nu)
            handles[vname] = (p, torch.empty(2 * p.output_samples(nb), dtype=torch.float32, device="cuda"), torch.cuda.ExternalStream(p.stream()))
        ms = {v[0]: [] for v in variants}
        for r in range(a.rounds):
            order = variants[r % len(variants):] + variants[:r % len(variants)]
            for vname, _flags, _on in order:
                p, out, stream = handles[vname]
                step = lambda i: p.process_device(rings[i % 3].data_ptr(), 0, nb, out.data_ptr())       # noqa: E731
                t0, i = time.perf_counter(), 0
                while (time.perf_counter() - t0) * 1e3 < a.settle_ms:
                    step(i)
                    p.synchronize()
                    i += 1
                for i in range(a.warmup):
                    step(i)
                p.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for i in range(a.steps):
                    step(i)
                e1.record(stream)
                e1.synchronize()
                ms[vname].append(e0.elapsed_time(e1) / a.steps)
        for vname, _flags, _on in variants:
            p = handles[vname][0]
            out_bytes = 8 * sum(p.lout) * nb
            print(json.dumps({"shape": name, "variant": vname, "N": N, "R": R, "channels": len(plan), "blocks": nb,
                              "ms": round(statistics.median(ms[vname]), 4), "ms_rounds": [round(v, 4) for v in ms[vname]],
                              "output_bytes": out_bytes, "describe": p.describe(), "steps": a.steps, "rounds": a.rounds}), flush=True)
            p.close()
        del rings


if __name__ == "__main__":
    main()
