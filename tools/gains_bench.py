"""Cost of the channel gains (fdc_pipeline_set_gains) on the device-resident entry: one JSON line per plan and mode.

Plans: configs[0] (the example flowgraph's 4096-pt plan, 16384 blocks a step: path 5) and configs[1] (65536-pt FFT, R = 2, 256 channels of 256 bins,
2048 blocks a step: the block kernel).  Modes, on the same build (a build without fdc_pipeline_set_gains — the parent commit, with this tool copied
beside it — times the first five only):
  off                 every setting off
  levels              levels on: k_chan_levels behind the plan's kernels
  sc16                sc16 output: the plan's kernels narrow in their own stores
  levels_sc16         both: float, k_chan_levels, then the call-wide k_complex_to_iq (two trips over the float results)
  fine                fine tuning on
  gains               gains on: k_chan_gain<false> in place
  gains_levels        k_chan_gain<true> in place (k_chan_levels is not launched)
  gains_sc16          k_chan_gain<false, sc16>: reads the float staging, stores narrow
  gains_levels_sc16   k_chan_gain<true, sc16>: one trip over the float results
  fine_gains          fine tuning and gains: k_fine_rotate<false, const float *> (off path 5), k_f4096's FINE form and k_chan_gain<false> (path 5)
Three input rings per mode, rotated as bench.py does, so the input of a step is cache-cold.  Every mode is timed in --rounds rounds, the order of the
modes rotated from round to round; each timing sits behind --settle-ms of untimed steps and the warm-up.  HIP events on the handle's stream; ms = the
median over the rounds, ms_rounds keeps each one.  kernel_ms: fdc_pipeline_last_kernel_ms of one more, untimed step (the plan's own kernels: the
passes behind them are not inside its events).  pass_ms = ms - ms(off) (ms - ms(fine) for fine_gains); pass_bytes = what the pass reads and writes
(in place: the float output twice; narrowing: the float output once and the narrow output once); pass_TBps = pass_bytes / pass_ms.

usage: python tools/gains_bench.py [--steps 20] [--warmup 3] [--rounds 3] [--settle-ms 150]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

#         name                 fine   levels gains  sc16
MODES = [("off",               False, False, False, False),
         ("levels",            False, True,  False, False),
         ("sc16",              False, False, False, True),
         ("levels_sc16",       False, True,  False, True),
         ("fine",              True,  False, False, False),
         ("gains",             False, False, True,  False),
         ("gains_levels",      False, True,  True,  False),
         ("gains_sc16",        False, False, True,  True),
         ("gains_levels_sc16", False, True,  True,  True),
         ("fine_gains",        True,  False, True,  False)]


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
    have = hasattr(G.Pipeline, "set_gains")
    modes = [m for m in MODES if have or not m[3]]
    for (name, N, R, plan, nb) in shapes(G):
        H, ovl = N - N // R, N // R
        rng = np.random.default_rng(1)
        base = (rng.standard_normal(2 * (ovl + nb * H)) * 1e-2).astype(np.float32)
        rings = [torch.from_numpy(np.roll(base, 7919 * 2 * k)).cuda() for k in range(3)]
        nu = np.linspace(-0.45, 0.45, len(plan))
        gains = np.exp2(np.linspace(-3.3, 3.3, len(plan))).astype(np.float32)      # 40 dB between the ends of the plan
        ms = {m[0]: [] for m in modes}
        handles = {}
        for mname, fine, lev, gain, sc16 in modes:
            p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
            if fine:
                p.set_fine_tuning(nu)
            if lev:
                p.set_levels(True)
            if gain:
                p.set_gains(gains)
            if sc16:
                p.set_output_format("sc16", 1000.0)
            handles[mname] = (p, torch.empty(2 * p.output_samples(nb), dtype=torch.float32, device="cuda"), torch.cuda.ExternalStream(p.stream()))
        for r in range(a.rounds):
            order = modes[r % len(modes):] + modes[:r % len(modes)]
            for mode in order:
                p, out, stream = handles[mode[0]]
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
                ms[mode[0]].append(e0.elapsed_time(e1) / a.steps)
        med = {m: statistics.median(v) for m, v in ms.items()}
        for mname, fine, lev, gain, sc16 in modes:
            p, out, _stream = handles[mname]
            p.enable_timing(True)
            p.process_device(rings[0].data_ptr(), 0, nb, out.data_ptr())
            p.synchronize()
            kms = p.last_kernel_ms()
            p.enable_timing(False)
            out_bytes = 8 * sum(p.lout) * nb
            res = {"shape": name, "mode": mname, "build": "change" if have else "parent", "N": N, "R": R, "channels": len(plan), "blocks": nb,
                   "ms": round(med[mname], 4), "ms_rounds": [round(v, 4) for v in ms[mname]], "kernel_ms": [round(v, 4) for v in kms[:3]],
                   "output_bytes": out_bytes, "describe": p.describe(), "steps": a.steps, "rounds": a.rounds}
            if gain:
                pass_ms = med[mname] - med["fine" if fine else "off"]
                pass_bytes = out_bytes + out_bytes // 2 if sc16 else 2 * out_bytes
                res["pass_ms"] = round(pass_ms, 4)
                res["pass_bytes"] = pass_bytes
                # (with the rotation the gain has no pass and no bytes of its own: the difference is a few instructions inside k_fine_rotate)
                merged = "gains: with the rotation" in p.describe()
                res["pass_TBps"] = round(pass_bytes / (pass_ms * 1e-3) / 1e12, 2) if pass_ms > 0 and not merged else None
            print(json.dumps(res), flush=True)
            p.close()
        del rings


if __name__ == "__main__":
    main()
