"""Complex integer output (fdc_pipeline_set_output_format) against complex float output: one JSON line per measurement.

(a) device-resident, cache-cold: process_device with float output against sc16 / sc8 output, and process_device_iq sc16 in / sc16 out, on the
    configs[1] shape (65536-pt FFT, R = 2, 256 channels of 256 bins, 2048 blocks a step) and the configs[0] shape (the example flowgraph's 4096-pt
    plan, 16384 blocks a step).  Three input rings per form, rotated as tools/iq_bench.py does; HIP events around the timed steps.  Every form is
    timed in each of --rounds rounds, the order of the forms rotated from round to round, each time behind bench.py's running-in (--settle-ms of
    untimed steps, then the warm-up steps): ms is the median over the rounds, ms_rounds all of them.  Algorithmic bytes per block:
    esz_in * H in + esz_out * sum(lout) out (esz = 8 float, 4 sc16, 2 sc8); frac_of_8TBps = bytes / time / 8e12.
(b) host-fed on the configs[1] plan, 512 blocks per call, pinned input: work (float in / out) against work_iq + sc16 out and sc8 in / sc8 out, each with
    the outputs registered with fdc_host_register (k_scatter_out / k_scatter_oq into the caller's buffers) and staged (pageable outputs through the
    handle's pinned slots), in Gsample/s of input.

usage: python tools/oq_bench.py [--steps 20] [--warmup 3] [--settle-ms 150] [--rounds 3] [--legs a,b]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from iq_bench import shapes   # noqa: E402

ESZ = {"float": 8, "sc16": 4, "sc8": 2}
OUT_SCALE = 32768.0


def leg_device(torch, np, G, name, N, R, plan, nb, steps, warmup, settle_ms, rounds):
    H, ovl = N - N // R, N // R
    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
    sum_lout = sum(p.lout)
    out = torch.empty(2 * p.output_samples(nb), dtype=torch.float32, device="cuda")   # the widest output: float
    stream = torch.cuda.ExternalStream(p.stream())
    rng = np.random.default_rng(1)
    base = rng.integers(-32768, 32768, 2 * (ovl + nb * H), dtype=np.int64)
    rings = {"float": [], "sc16": []}
    for k in range(3):
        v = np.roll(base, 7919 * 2 * k)
        rings["sc16"].append(torch.from_numpy(v.astype(np.int16)).cuda())
        rings["float"].append(torch.from_numpy(v.astype(np.float32) * np.float32(2.0 ** -15)).cuda())
    forms = [("float", "float"), ("float", "sc16"), ("float", "sc8"), ("sc16", "sc16")]
    times = {f: [] for f in forms}
    describe = {}
    for rnd in range(rounds):
        for fin, fout in forms[rnd % len(forms):] + forms[:rnd % len(forms)]:
            p.set_output_format(None if fout == "float" else fout, OUT_SCALE)

            def step(i):
                r = rings[fin][i % 3].data_ptr()
                if fin == "float":
                    p.process_device(r, 0, nb, out.data_ptr())
                else:
                    p.process_device_iq(fin, 2.0 ** -15, r, 0, nb, out.data_ptr())

            # running-in as bench.py: untimed steps for settle_ms (the device leaves its idle clocks), then the warm-up steps
            t0, i = time.perf_counter(), 0
            while (time.perf_counter() - t0) * 1e3 < settle_ms:
                step(i)
                i += 1
                if i % 8 == 0:
                    p.synchronize()
            for k in range(warmup):
                step(i + k)
            p.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(steps):
                step(k)
            e1.record(stream)
            e1.synchronize()
            times[(fin, fout)].append(e0.elapsed_time(e1) / steps)
            describe[(fin, fout)] = p.describe()
    lines = []
    for fin, fout in forms:
        ms = float(np.median(times[(fin, fout)]))
        per_block = ESZ[fin] * H + ESZ[fout] * sum_lout
        b = per_block * nb
        lines.append({"leg": "a", "shape": name, "input": fin, "output": fout, "N": N, "R": R, "channels": len(plan), "blocks": nb, "ms": round(ms, 4),
                      "ms_rounds": [round(t, 4) for t in times[(fin, fout)]], "alg_bytes_per_block": per_block, "alg_bytes": b,
                      "frac_of_8TBps": round(b / (ms * 1e-3) / 8e12, 4), "describe": describe[(fin, fout)], "rings": 3, "steps": steps,
                      "settle_ms": settle_ms, "warmup": warmup})
    p.close()
    return lines


def leg_host(np, G, N, R, plan, nb, reps):
    H = N - N // R
    lines = []
    rng = np.random.default_rng(7)
    xi = rng.integers(-32768, 32768, 2 * nb * H, dtype=np.int64)
    for fin, fout in (("float", "float"), ("sc16", "sc16"), ("sc8", "sc8")):
        for route in ("registered", "staged"):
            p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
            if fin == "float":
                x = (xi.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64)
            else:
                x = xi.astype(np.int16) if fin == "sc16" else (xi >> 8).astype(np.int8)
            if fout != "float":
                p.set_output_format(fout, 1.0 if fout == "sc8" else 8.0)
            dt_out = {"float": np.complex64, "sc16": np.int16, "sc8": np.int8}[fout]
            per = 1 if fout == "float" else 2
            pool = np.zeros(per * nb * sum(p.lout), dt_out)
            outs, off = [], 0
            for lo in p.lout:
                o = pool[off:off + per * nb * lo]
                outs.append(o if fout == "float" else o.reshape(-1, 2))
                off += per * nb * lo
            G.register_host(x)
            if route == "registered":
                G.register_host(pool)
            try:
                call = (lambda: p.work(x, outs=outs)) if fin == "float" else (lambda: p.work_iq(x, scale=2.0 ** -15, outs=outs))
                for _ in range(2):
                    call()
                t = time.perf_counter()
                for _ in range(reps):
                    call()
                dt = (time.perf_counter() - t) / reps
            finally:
                G.unregister_host(x)
                if route == "registered":
                    G.unregister_host(pool)
            lines.append({"leg": "b", "shape": "configs[1] plan, host-fed", "input": fin, "output": fout, "outputs": route, "blocks_per_call": nb,
                          "ms_per_call": round(dt * 1e3, 3), "Gsample_per_s": round(nb * H / dt / 1e9, 4), "input_bytes_per_call": x.nbytes,
                          "output_bytes_per_call": pool.nbytes, "describe": p.describe()})
            p.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--settle-ms", type=float, default=150.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-blocks", type=int, default=512)
    a = ap.parse_args()
    import torch
    import numpy as np
    import gr_fdc_amd as G
    legs = a.legs.split(",")
    if "a" in legs:
        for (name, N, R, plan, nb) in shapes(G):
            for ln in leg_device(torch, np, G, name, N, R, plan, nb, a.steps, a.warmup, a.settle_ms, a.rounds):
                print(json.dumps(ln), flush=True)
    if "b" in legs:
        name, N, R, plan, _nb = shapes(G)[0]
        for ln in leg_host(np, G, N, R, plan, a.host_blocks, 8):
            print(json.dumps(ln), flush=True)


if __name__ == "__main__":
    main()
