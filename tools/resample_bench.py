"""Cost of the audio resampler (fdc_pipeline_set_audio_resampler) on the device-resident entry, this tree and a parent build interleaved in one session:
one JSON line per build, plan and mode.  The method is tools/audio_bench.py's (profiles/audio/README.md).

Plans: configs[0] (the example flowgraph's 4096-pt plan, 16384 blocks a step: path 5) and configs[1] (65536-pt FFT, R = 2, 256 channels of 256 bins,
2048 blocks a step: the block kernel).  Modes:
  off            every setting off (the condition "nothing changes while it is off": this tree against the parent)
  fm             the demodulation alone: what every pass below runs behind
  dec_f32        FM and the decimating form at D = 8, K = 64 (lowpass_taps), float32: the parent's k_chan_audio, in both builds
  rs_1_8_f32     FM and the resampler at 1 / 8 with the same 64 taps, float32: the same arithmetic and the same bytes as dec_f32 (LIKE FOR LIKE)
  rs_8_25_f32, rs_8_25_s16, rs_48_25_f32, rs_48_25_s16
                 FM and the resampler at 8 / 25 and 48 / 25 with resampler_taps (16 taps per phase), float32 and int16
A build without fdc_pipeline_set_audio_resampler (the parent) is timed in off, fm and dec_f32 only.

Every build runs in a worker process of its own (this file with --worker: the build's own Python package and library, found under its root) that keeps
its handles and answers one timing at a time, so the driver interleaves the builds: per round every (build, mode) pair once, the order rotated from round
to round.  Each timing sits behind --settle-ms of untimed steps and the warm-up; three input rings per plan, rotated as bench.py does, so the input of
a step is cache-cold.  HIP events on the handle's stream; ms = the median over the rounds, ms_rounds keeps each one.
pass_ms = ms - ms(fm) of the same build: the time of the audio pass.  bytes = what the pass must move: 4 bytes per demodulated sample read and the
matrix written; pass_TBps = bytes / pass_ms.  like_for_like (rs_1_8_f32 of this tree) = its pass_ms over the PARENT's dec_f32 pass_ms (this tree's
where there is no parent).  link_bytes: what a step hands to the host, the matrix against the demodulated ports (port_bytes).

usage: python tools/resample_bench.py [--parent DIR] [--steps 20] [--warmup 3] [--rounds 5] [--settle-ms 150]
       DIR: a checkout of the parent commit with its library built (make -C gr-fdc_amd/csrc)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIM, NTAPS = 8, 64
# (name, demodulation, form, format): form None, ("dec", D) or ("rs", up, down)
MODES = [("off", None, None, None), ("fm", "fm", None, None), ("dec_f32", "fm", ("dec", DECIM), "f32"), ("rs_1_8_f32", "fm", ("rs", 1, DECIM), "f32"),
         ("rs_8_25_f32", "fm", ("rs", 8, 25), "f32"), ("rs_8_25_s16", "fm", ("rs", 8, 25), "s16"),
         ("rs_48_25_f32", "fm", ("rs", 48, 25), "f32"), ("rs_48_25_s16", "fm", ("rs", 48, 25), "s16")]


def shapes(G):
    R = 2
    cfg1 = [(256 * c, 256, 0.88, 1.0) for c in range(256)]
    params = [G.get_opt_channelparams(4096, R, (u + 0.5) % 1.0, bw) for (u, bw) in ((0.12, 0.05), (0.22, 0.1), (-0.14, 0.12), (0.0, 0.081))]
    cfg0 = [(f, l, p, s) for (f, l, _lo, p, s) in params]
    return {"configs[0]": (4096, R, cfg0, 16384), "configs[1]": (65536, R, cfg1, 2048)}


def worker(root):
    """answers on stdout, one JSON line per request line on stdin: "modes" | "open SHAPE" | "time SHAPE MODE STEPS WARMUP SETTLE_MS" | "info SHAPE MODE" |
    "close SHAPE" """
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gr_fdc_amd as G
    have = hasattr(G.Pipeline, "set_audio_resampler")
    modes = [m for m in MODES if have or not (m[2] and m[2][0] == "rs")]
    state = {}

    def say(obj):
        sys.stdout.write(json.dumps(obj) + "\n")
        sys.stdout.flush()

    for line in sys.stdin:
        cmd = line.split("\t")
        cmd[-1] = cmd[-1].rstrip("\n")
        if cmd[0] == "modes":
            say([m[0] for m in modes])
        elif cmd[0] == "open":
            N, R, plan, nb = shapes(G)[cmd[1]]
            H, ovl = N - N // R, N // R
            base = (np.random.default_rng(1).standard_normal(2 * (ovl + nb * H)) * 1e-2).astype(np.float32)
            rings = [torch.from_numpy(np.roll(base, 7919 * 2 * k)).cuda() for k in range(3)]
            handles = {}
            for mname, dem, form, fmt in modes:
                p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
                if dem:
                    p.set_demod(dem, 0.15915494)
                if form and form[0] == "dec":
                    p.set_audio(form[1], G.lowpass_taps(form[1], NTAPS), fmt, 30000.0)
                elif form:
                    taps = G.lowpass_taps(form[2], NTAPS) if form[1] == 1 else G.resampler_taps(form[1], form[2])
                    p.set_audio_resampler(form[1], form[2], taps, fmt, 30000.0)
                # (a buffer of the complex float size serves every mode: the real outputs use its first half)
                handles[mname] = (p, torch.empty(2 * p.output_samples(nb), dtype=torch.float32, device="cuda"), torch.cuda.ExternalStream(p.stream()))
            state[cmd[1]] = (rings, handles, nb)
            say("ok")
        elif cmd[0] == "time":
            rings, handles, nb = state[cmd[1]]
            p, out, stream = handles[cmd[2]]
            steps, warmup, settle = int(cmd[3]), int(cmd[4]), float(cmd[5])
            step = lambda i: p.process_device(rings[i % 3].data_ptr(), 0, nb, out.data_ptr())       # noqa: E731
            t0, i = time.perf_counter(), 0
            while (time.perf_counter() - t0) * 1e3 < settle:
                step(i)
                p.synchronize()
                i += 1
            for i in range(warmup):
                step(i)
            p.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(steps):
                step(i)
            e1.record(stream)
            e1.synchronize()
            say(e0.elapsed_time(e1) / steps)
        elif cmd[0] == "info":
            rings, handles, nb = state[cmd[1]]
            p, out, _stream = handles[cmd[2]]
            p.process_device(rings[0].data_ptr(), 0, nb, out.data_ptr())
            p.synchronize()
            info = {"samples": sum(p.lout) * nb, "describe": p.describe(), "channels": len(p.lout), "blocks": nb, "N": p.N, "R": p.R}
            if p.audio_device() is not None:
                a = p.audio(nb)
                info.update(audio_samples=int(a.size), link_bytes=int(a.nbytes), port_bytes=4 * info["samples"])
            say(info)
        elif cmd[0] == "close":
            rings, handles, _nb = state.pop(cmd[1])
            for p, _out, _stream in handles.values():
                p.close()
            del rings, handles
            torch.cuda.empty_cache()
            say("ok")


class Build:
    def __init__(self, name, root):
        self.name, self.root = name, root
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, *cmd):
        self.proc.stdin.write("\t".join(str(c) for c in cmd) + "\n")
        self.proc.stdin.flush()
        line = self.proc.stdout.readline()
        if not line:
            raise SystemExit("the worker of %s (%s) ended with status %r" % (self.name, self.root, self.proc.wait()))
        return json.loads(line)

    def close(self):
        self.proc.stdin.close()
        self.proc.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", metavar="ROOT")
    ap.add_argument("--parent", metavar="DIR")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=150.0)
    ap.add_argument("--shapes", default="configs[0],configs[1]")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    builds = [Build("change", ROOT)] + ([Build("parent", os.path.abspath(a.parent))] if a.parent else [])
    try:
        for shape in a.shapes.split(","):
            pairs = [(b, m) for b in builds for m in b.ask("modes")]
            for b in builds:
                b.ask("open", shape)
            ms = {(b.name, m): [] for b, m in pairs}
            for r in range(a.rounds):
                k = r % len(pairs)
                for b, m in pairs[k:] + pairs[:k]:
                    ms[(b.name, m)].append(b.ask("time", shape, m, a.steps, a.warmup, a.settle_ms))
            med = {k: statistics.median(v) for k, v in ms.items()}
            yard = med[(builds[-1].name, "dec_f32")] - med[(builds[-1].name, "fm")]           # the parent's k_chan_audio where there is a parent
            for b, m in pairs:
                res = {"build": b.name, "shape": shape, "mode": m, "ms": round(med[(b.name, m)], 4), "ms_rounds": [round(v, 4) for v in ms[(b.name, m)]],
                       "steps": a.steps, "rounds": a.rounds}
                res.update(b.ask("info", shape, m))
                if "_" in m:
                    own = med[(b.name, m)] - med[(b.name, "fm")]
                    res["pass_ms"] = round(own, 4)
                    res["bytes"] = 4 * res["samples"] + res["link_bytes"]
                    res["pass_TBps"] = round(res["bytes"] / (own * 1e-3) / 1e12, 3) if own > 0 else None
                    if m == "rs_1_8_f32":
                        res["like_for_like"] = round(own / yard, 3) if yard > 0 else None
                if b.name == "change" and len(builds) > 1 and ("parent", m) in med:
                    res["over_parent"] = round(med[("change", m)] / med[("parent", m)], 4)
                print(json.dumps(res), flush=True)
            for b in builds:
                b.ask("close", shape)
    finally:
        for b in builds:
            b.close()


if __name__ == "__main__":
    main()
