"""Complex integer input (fdc_pipeline_process_device_iq / fdc_pipeline_work_iq) against complex float input: one JSON line per leg.

(a) device-resident, cache-cold: process_device against process_device_iq (sc16, sc8) on the configs[1] shape (65536-pt FFT, R = 2, 256 channels of
    256 bins, 2048 blocks a step) and the configs[0] shape (the example flowgraph's 4096-pt plan, 16384 blocks a step).  Three input rings per form,
    rotated as bench.py does, so no input byte of a step is still in the 256 MiB memory-side cache; HIP events around the timed steps.  Algorithmic
    bytes per block: esz * H in + 8 * sum(lout) out (esz = 8 float, 4 sc16, 2 sc8); frac_of_8TBps = bytes / time / 8e12.
(b) host-fed: work against work_iq on the configs[1] plan from buffers pinned with fdc_host_register, in Gsample/s of input.

usage: python tools/iq_bench.py [--steps 20] [--warmup 3] [--legs a,b]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(G):
    N1, R = 65536, 2
    cfg1 = [(256 * c, 256, 0.88, 1.0) for c in range(256)]
    params = [G.get_opt_channelparams(4096, R, (u + 0.5) % 1.0, bw) for (u, bw) in ((0.12, 0.05), (0.22, 0.1), (-0.14, 0.12), (0.0, 0.081))]
    cfg0 = [(f, l, p, s) for (f, l, _lo, p, s) in params]
    return [("configs[1]", N1, R, cfg1, 2048), ("configs[0]", 4096, R, cfg0, 16384)]


def leg_device(torch, np, G, name, N, R, plan, nb, steps, warmup):
    H, ovl = N - N // R, N // R
    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
    sum_lout = sum(p.lout)
    out = torch.empty(2 * p.output_samples(nb), dtype=torch.float32, device="cuda")
    stream = torch.cuda.ExternalStream(p.stream())            # the handle's own stream: the launches and the events on one queue
    rng = np.random.default_rng(1)
    base = rng.integers(-32768, 32768, 2 * (ovl + nb * H), dtype=np.int64)
    lines = []
    for form, esz in (("float", 8), ("sc16", 4), ("sc8", 2)):
        rings = []
        for k in range(3):
            v = np.roll(base, 7919 * 2 * k)
            if form == "sc8":
                rings.append(torch.from_numpy((v >> 8).astype(np.int8)).cuda())
            elif form == "sc16":
                rings.append(torch.from_numpy(v.astype(np.int16)).cuda())
            else:
                rings.append(torch.from_numpy((v.astype(np.float32) * np.float32(2.0 ** -15))).cuda())
        scale = 2.0 ** -15 if form == "sc16" else 2.0 ** -7

        def step(i):
            r = rings[i % 3].data_ptr()
            if form == "float":
                p.process_device(r, 0, nb, out.data_ptr())
            else:
                p.process_device_iq(form, scale, r, 0, nb, out.data_ptr())

        for i in range(warmup):
            step(i)
        p.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(steps):
            step(i)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / steps
        per_block = esz * H + 8 * sum_lout
        b = per_block * nb
        lines.append({"leg": "a", "shape": name, "input": form, "N": N, "R": R, "channels": len(plan), "blocks": nb, "ms": round(ms, 4),
                      "alg_bytes_per_block": per_block, "alg_bytes": b, "frac_of_8TBps": round(b / (ms * 1e-3) / 8e12, 4),
                      "describe": p.describe(), "rings": 3, "steps": steps})
        del rings
    p.close() if hasattr(p, "close") else None
    return lines


def leg_host(np, G, N, R, plan, nb, reps):
    H = N - N // R
    lines = []
    rng = np.random.default_rng(7)
    xi = rng.integers(-32768, 32768, 2 * nb * H, dtype=np.int64)
    for form in ("float", "sc16", "sc8"):
        p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
        if form == "float":
            x = (xi.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64)
        else:
            x = xi.astype(np.int16) if form == "sc16" else (xi >> 8).astype(np.int8)
        pool = np.zeros(nb * sum(p.lout), np.complex64)
        outs, off = [], 0
        for lo in p.lout:
            outs.append(pool[off:off + nb * lo])
            off += nb * lo
        G.register_host(x); G.register_host(pool)
        try:
            call = (lambda: p.work(x, outs=outs)) if form == "float" else (lambda: p.work_iq(x, scale=2.0 ** -15, outs=outs))
            for _ in range(2):
                call()
            t = time.perf_counter()
            for _ in range(reps):
                call()
            dt = (time.perf_counter() - t) / reps
        finally:
            G.unregister_host(x); G.unregister_host(pool)
        lines.append({"leg": "b", "shape": "configs[1] plan, host-fed", "input": form, "blocks_per_call": nb, "ms_per_call": round(dt * 1e3, 3),
                      "Gsample_per_s": round(nb * H / dt / 1e9, 4), "input_bytes_per_call": x.nbytes,
                      "entry": "fdc_pipeline_work" if form == "float" else "fdc_pipeline_work_iq", "buffers": "pinned with fdc_host_register"})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--host-blocks", type=int, default=512)
    a = ap.parse_args()
    import torch
    import numpy as np
    import gr_fdc_amd as G
    legs = a.legs.split(",")
    if "a" in legs:
        for (name, N, R, plan, nb) in shapes(G):
            for ln in leg_device(torch, np, G, name, N, R, plan, nb, a.steps, a.warmup):
                print(json.dumps(ln), flush=True)
    if "b" in legs:
        name, N, R, plan, _nb = shapes(G)[0]
        for ln in leg_host(np, G, N, R, plan, a.host_blocks, 8):
            print(json.dumps(ln), flush=True)


if __name__ == "__main__":
    main()
