"""Cost of the sink payload formats (fdc_sinks_set_payload_format): one JSON line per workload and variant.

Workloads: the configs[2] bank that `bench.py --config 3` builds (65536-pt FFT, R = 2, 256 PowerActivationChannels of 256 bins, bursty carriers, 1024
blocks a step) and configs[4]'s (`--config 5`: activity_detection_channelizer_vcm, two segments, 24 bursty carriers) on bench.py's own input.
Variants: payloads to pinned host memory and left in HBM (--payload device), each as fc32, sc16 and sc8.  On a build without
fdc_sinks_set_payload_format (the parent commit, through FDC_AMD_LIB) only fc32 is timed.
A step is bench.py's two-deep step: forward transform into the bank's buffer, power cells from the group sums, fdc_sinks_submit_device; the PDUs of
the batch before are read (counted) in every step.  Every variant is timed in --rounds rounds, the order of the variants rotated from round to round;
each timing sits behind --settle-ms of untimed steps and the warm-up, between two device-wide fences (the payload copy runs on a stream of its own:
the fence is what waits for it), with HIP events on the bank's stream beside it (ms_stream: the kernels' side alone).  ms = the median over the rounds.
payload_bytes = the bytes of the emitted runs per batch (used_a * bytes per sample: what the copy to the host moves), route = fdc_sinks_payload_route.

usage: python tools/payload_bench.py [--config 3|5] [--steps 20] [--warmup 3] [--rounds 3] [--settle-ms 150] [--lookahead]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = {"fc32": 8, "sc16": 4, "sc8": 2}
SCALE = {"fc32": 1.0, "sc16": 2048.0, "sc8": 8.0}


def workload(G, np, torch, bench, config, lookahead, device_payload):
    N, R, nb, C = 65536, 2, 1024, 256
    if config == 3:
        pac = [(((c + 0.5) / C) % 1.0, 0.8 / C, c) for c in range(C)]
        bank = G.Sinks(N, R, pac=pac, pac_thresh=6.0, pac_maxblocks=128, pac_delay=1, max_blocks=nb, device_payload=device_payload,
                       lookahead=lookahead)
        carriers, seed = [((c + 0.5) / C - 0.5, 1.0 / C) for c in range(C)], 2026
    else:
        segments = [((0.05 + 0.5) % 1.0, (0.45 + 0.5) % 1.0), ((-0.45 + 0.5) % 1.0, (-0.05 + 0.5) % 1.0)]
        bank = G.Sinks(N, R, segments=segments, det_thresh=10.0, det_maxblocks=128, minchandist=0.005, det_delay=1, puffer=0.2,
                       max_blocks=nb, device_payload=device_payload, lookahead=lookahead)
        rng = np.random.default_rng(2028)
        carriers, used, seed = [], [], 2028
        while len(carriers) < 24:
            wd = float(rng.uniform(0.002, 0.03))
            lo, hi = ((0.05, 0.45), (-0.45, -0.05))[int(rng.integers(0, 2))]
            fc = float(rng.uniform(lo + wd, hi - wd))
            if all(abs(fc - u) > (wd + v) * 0.75 + 0.006 for (u, v) in used):
                used.append((fc, wd)); carriers.append((fc, wd))
    return N, R, nb, bank, carriers, seed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3, choices=(3, 5))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=150.0)
    ap.add_argument("--lookahead", action="store_true")
    ap.add_argument("--formats", default="fc32,sc16,sc8")
    ap.add_argument("--payloads", default="host,device")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gr_fdc_amd as G
    from gr_fdc_amd import _lib
    import bench
    have = hasattr(G.Sinks, "set_payload_format")
    formats = [f for f in a.formats.split(",") if f == "fc32" or have]
    dev = torch.device("cuda:0")
    x, pipe, variants = None, None, []
    for payload in a.payloads.split(","):
        for fmt in formats:
            N, R, nb, bank, carriers, seed = workload(G, np, torch, bench, a.config, a.lookahead, payload == "device")
            if fmt != "fc32":
                bank.set_payload_format(fmt, SCALE[fmt])
            variants.append((payload, fmt, bank))
    x = bench.synth_bursty(torch, dev, N, R, carriers, nb, seed)
    pipe = G.Pipeline(N, R, [], windowtype=1, max_blocks=nb, keep_spectrum=True)
    if a.lookahead:
        pipe.reserve_compute_units(32)
    torch.cuda.synchronize()
    L = _lib.lib()

    def make_step(bank, tally):
        sstream, fstream = bank.stream(), bank.fill_stream()

        def step():
            if a.lookahead:
                pipe.process_device(x.data_ptr(), 0, nb, None, d_spectrum=bank.spectrum_ahead_ptr(), stream=fstream,
                                    d_group_power=bank.group_power_ahead_ptr())
                bank.prepare(nb, ahead=True, from_groups=True)
            else:
                pipe.process_device(x.data_ptr(), 0, nb, None, d_spectrum=bank.spectrum_ptr(), stream=sstream, d_group_power=bank.group_power_ptr())
                bank.prepare(nb, ahead=False, from_groups=True)
            done = _lib.check(L.fdc_sinks_submit_device(bank._h, nb))
            if done > 0:
                n = L.fdc_sinks_pdu_count(bank._h)
                if n > 0:
                    arr = (_lib.fdc_pdu * n)()
                    L.fdc_sinks_pdus(bank._h, arr, n)
                    tally[0] += int(np.frombuffer(arr, dtype=np.dtype(_lib.fdc_pdu))["nsamples"].sum())
                    tally[1] += n
                tally[2] += 1
        return step

    res = {(p, f): {"ms": [], "ms_stream": [], "tally": [0, 0, 0]} for (p, f, _b) in variants}
    for (p, f, bank) in variants:
        if a.lookahead:      # the first batch of a look-ahead bank goes into its current buffer
            pipe.process_device(x.data_ptr(), 0, nb, None, d_spectrum=bank.spectrum_ptr(), stream=bank.fill_stream(), d_group_power=bank.group_power_ptr())
            bank.prepare(nb, ahead=False, from_groups=True)
    for r in range(a.rounds):
        order = variants[r % len(variants):] + variants[:r % len(variants)]
        for (p, f, bank) in order:
            rec = res[(p, f)]
            idle = [0, 0, 0]
            step = make_step(bank, idle)
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < a.settle_ms:
                step()
                torch.cuda.synchronize()
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            step = make_step(bank, rec["tally"])
            stream = torch.cuda.ExternalStream(bank.stream())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            w0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            e1.record(stream)
            torch.cuda.synchronize()
            rec["ms"].append((time.perf_counter() - w0) * 1e3 / a.steps)
            rec["ms_stream"].append(e0.elapsed_time(e1) / a.steps)
            rec["route"] = int(L.fdc_sinks_payload_route(bank._h)) if have else 0
    for (p, f, bank) in variants:
        rec = res[(p, f)]
        samples, npdu, nbatch = rec["tally"]
        print(json.dumps({"workload": "configs[%d]" % (a.config - 1), "payload": p, "format": f, "lookahead": bool(a.lookahead), "blocks": nb,
                          "ms": round(statistics.median(rec["ms"]), 4), "ms_rounds": [round(v, 4) for v in rec["ms"]],
                          "ms_stream": round(statistics.median(rec["ms_stream"]), 4),
                          "used_a_samples_per_batch": round(samples / max(1, nbatch), 1),
                          "payload_bytes_per_batch": round(samples * BYTES[f] / max(1, nbatch), 1), "copied_to_host": p == "host",
                          "pdus_per_batch": round(npdu / max(1, nbatch), 1), "route": rec["route"], "steps": a.steps, "rounds": a.rounds,
                          "lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)) or "."}), flush=True)
        bank.flush()
        bank.close()


if __name__ == "__main__":
    main()
