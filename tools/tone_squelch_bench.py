"""Cost and gain of the tone squelch (fdc_pipeline_set_tone_squelch), this tree and a parent build interleaved in one session: one JSON line per build,
plan and mode.

Plans: configs[0] (the example flowgraph's 4096-pt plan, 16384 blocks a step: FOUR channels and many blocks) and configs[1] (65536-pt FFT, R = 2, 256
channels of 256 bins, 2048 blocks a step).  THE BAND: every channel carries a carrier at its centre, and every eighth channel (configs[0]: one of the
four) is phase-modulated by the selected tone, CTCSS 100.0 Hz at a 25 kHz channel rate; a little noise.  The chain: levels, FM, the audio filter D = 8,
K = 64 (float32), the carrier squelch (thresholds a tenth of every channel's own median power: all open), the packing, the 50 CTCSS tones with S = 16,
W = 32.  The tone squelch's thresholds: the geometric mean of the selected tone's median |Z|^2 in the channels that carry it and in those that do
not, close = open / 2, ratio 0, guard 1, hang 1.  Modes, on the device-resident entry (HIP events on the handle's stream):
  off             every setting off (the condition "nothing changes while it is off": this tree against the parent)
  carrier         the chain with the tone squelch off: the parent's carrier-gated packed step (both builds)
  tsq             the chain with the tone squelch on (this tree)
  k_squelch, k_tones, k_decide, k_decide_gate
                  fdc_pipeline_squelch_pass_device, fdc_pipeline_tones_pass_device and fdc_pipeline_tone_squelch_pass_device (without and with the
                  mask) alone, over the buffers of tsq's last call: the launches' own time on the same call; gate_ms = k_decide_gate - k_decide
and on the host entry, fdc_pipeline_work from a registered (pinned) host buffer with outs = NULL, wall clock around the call (it synchronises itself):
  host_carrier    the parent's carrier-gated packed step (both builds)
  host_tsq        the same with the tone squelch on; link_bytes: what the call copies home (packed audio, count, mask, levels, frame rows, decisions)
A build without fdc_pipeline_set_tone_squelch (the parent) is timed in off, carrier and host_carrier only.  With --parent the parent is timed TWICE, by
two workers of its own ("parent", "parent_again"): the spread of the parent against itself in the session is the margin of every comparison with it.

Every build runs in a worker process of its own (this file with --worker) that keeps its handles and answers one timing at a time, so the driver
interleaves the builds: per round every (build, mode) pair once, the order rotated from round to round.  ms = the median over the rounds.

usage: python tools/tone_squelch_bench.py [--parent DIR] [--steps 20] [--host-steps 4] [--warmup 3] [--rounds 5] [--settle-ms 150]
       DIR: a checkout of the parent commit with its library built (make -C gr-fdc_amd/csrc)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIM, NTAPS, GROUP, FRAME, RATE, SEL, BETA = 8, 64, 16, 32, 25000.0, 12, 0.5
# (name, the chain on, the tone squelch on, entry: "dev" / "host" / a pass)
MODES = [("off", False, False, "dev"), ("carrier", True, False, "dev"), ("tsq", True, True, "dev"), ("k_squelch", True, True, "squelch"),
         ("k_tones", True, True, "tones"), ("k_decide", True, True, "decide"), ("k_decide_gate", True, True, "decide_gate"),
         ("host_carrier", True, False, "host"), ("host_tsq", True, True, "host")]


def shapes(G):
    R = 2
    cfg1 = [(256 * c, 256, 0.88, 1.0) for c in range(256)]
    params = [G.get_opt_channelparams(4096, R, (u + 0.5) % 1.0, bw) for (u, bw) in ((0.12, 0.05), (0.22, 0.1), (-0.14, 0.12), (0.0, 0.081))]
    cfg0 = [(f, l, p, s) for (f, l, _lo, p, s) in params]
    return {"configs[0]": (4096, R, cfg0, 16384), "configs[1]": (65536, R, cfg1, 2048)}


def band(torch, G, N, plan, n, every):
    """n samples of the band on the device: a carrier per channel, every `every`-th one phase-modulated by the selected tone"""
    t = torch.arange(n, dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    x = 1e-4 * torch.view_as_complex(torch.randn(n, 2, dtype=torch.float32, device="cuda", generator=g))
    f_tone = float(G.ctcss_tones()[SEL]) / RATE                          # cycles per output sample of the channel
    for c, (f, l, _p, _s) in enumerate(plan):
        ph = torch.frac(((f + 0.5 * l) / N - 0.5) * t)
        if c % every == 0:
            ph = ph + (BETA / 6.283185307179586) * torch.sin(6.283185307179586 * torch.frac(f_tone * l / N * t))
        ph = (6.283185307179586 * ph).to(torch.float32)
        x = x + 1e-2 * torch.complex(torch.cos(ph), torch.sin(ph))
    return x


def worker(root):
    """answers on stdout, one JSON line per request line on stdin: "modes" | "open SHAPE" | "time SHAPE MODE STEPS WARMUP SETTLE_MS" | "info SHAPE MODE" |
    "close SHAPE" """
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gr_fdc_amd as G
    have = hasattr(G.Pipeline, "set_tone_squelch")
    modes = [m for m in MODES if have or not m[2]]
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
            H, ovl, Cn = N - N // R, N // R, len(plan)
            every = 8 if Cn > 4 else 4
            x = band(torch, G, N, plan, ovl + nb * H, every)
            rings = [torch.view_as_real(torch.roll(x, 7919 * k)).contiguous() for k in range(3)]
            host = x[ovl:].cpu().numpy().copy()                                   # the host entry's input: nb * H complex samples, registered (pinned)
            G.register_host(host)
            del x
            inc = G.tone_increments(G.ctcss_tones(), RATE, GROUP)

            def chain():
                p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
                p.set_levels(True)
                p.set_demod("fm", 0.15915494)
                p.set_audio(DECIM, G.lowpass_taps(DECIM, NTAPS), "f32")
                p.set_tones(inc, GROUP, FRAME)
                return p

            # the thresholds, from one call of the chain without a squelch: the same figures in every build (the same kernels made them)
            p = chain()
            out = torch.empty(2 * p.output_samples(nb), dtype=torch.float32, device="cuda")
            p.process_device(rings[0].data_ptr(), 0, nb, out.data_ptr())
            p.synchronize()
            power = np.median(p.levels(nb)[:, :, 0], axis=0)
            e = np.median(np.abs(p.tones(nb)[:, :, SEL].astype(np.complex128)) ** 2, axis=0)
            toned = np.arange(Cn) % every == 0
            thr_sq = (0.1 * power).astype(np.float32)
            thr_tone = np.float32(np.sqrt(np.median(e[toned]) * np.median(e[~toned])))
            p.close()
            handles = {}
            for mname, on, tsq, entry in modes:
                if entry not in ("dev", "host"):
                    continue                                                      # (the passes run on tsq's handle)
                if on:
                    p = chain()
                    p.set_squelch(thr_sq, thr_sq, 2)
                    p.set_audio_packing(True)
                    if tsq:
                        p.set_tone_squelch(SEL, thr_tone, thr_tone / 2, 0.0, 1, 1)
                else:
                    p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
                # (a buffer of the complex float size serves every mode: the real outputs use its first half)
                handles[mname] = (p, torch.empty(2 * p.output_samples(nb), dtype=torch.float32, device="cuda"), torch.cuda.ExternalStream(p.stream()))
            nf = nb // FRAME
            scratch = dict(mask=torch.empty(nb * Cn, dtype=torch.uint8, device="cuda"), state=torch.zeros(4 * Cn, dtype=torch.int32, device="cuda"),
                           dec=torch.empty(nf * Cn, dtype=torch.uint8, device="cuda"), rows=torch.empty(2 * nf * Cn * 50, dtype=torch.float32, device="cuda"),
                           carry=torch.zeros(4 * Cn * 50, dtype=torch.float32, device="cuda"))
            state[cmd[1]] = (rings, host, handles, nb, scratch, dict(thr_tone=float(thr_tone), e_toned=float(np.median(e[toned])), e_other=float(np.median(e[~toned]))))
            say("ok")
        elif cmd[0] == "time":
            rings, host, handles, nb, sc, _thr = state[cmd[1]]
            entry = [m[3] for m in modes if m[0] == cmd[2]][0]
            p, out, stream = handles[cmd[2] if entry in ("dev", "host") else "tsq"]
            Cn = len(p.lout)
            steps, warmup, settle = int(cmd[3]), int(cmd[4]), float(cmd[5])
            if entry not in ("dev", "host"):
                p.process_device(rings[0].data_ptr(), 0, nb, out.data_ptr())     # (the levels, the samples, the rows and the mask the passes go over)
                p.synchronize()
            s0, s1 = sc["state"].data_ptr(), sc["state"].data_ptr() + 8 * Cn
            step = {"host": lambda i: p.work_raw(host.ctypes.data, nb, None),
                    "dev": lambda i: p.process_device(rings[i % 3].data_ptr(), 0, nb, out.data_ptr()),
                    "squelch": lambda i: p.squelch_pass_device(p.levels_device(), sc["mask"].data_ptr(), nb, s0, s1),
                    "tones": lambda i: p.tones_pass_device(out.data_ptr(), sc["rows"].data_ptr(), nb, 0, 0, None, sc["carry"].data_ptr()),
                    "decide": lambda i: p.tone_squelch_pass_device(p.tones_device(), sc["dec"].data_ptr(), nb, 0, s0, s1, None),
                    "decide_gate": lambda i: p.tone_squelch_pass_device(p.tones_device(), sc["dec"].data_ptr(), nb, 0, s0, s1, sc["mask"].data_ptr())}[entry]
            t0, i = time.perf_counter(), 0
            while (time.perf_counter() - t0) * 1e3 < settle:
                step(i)
                p.synchronize()
                i += 1
            for i in range(warmup):
                step(i)
            p.synchronize()
            if entry == "host":
                t0 = time.perf_counter()
                for i in range(steps):
                    step(i)
                say((time.perf_counter() - t0) * 1e3 / steps)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(steps):
                step(i)
            e1.record(stream)
            e1.synchronize()
            say(e0.elapsed_time(e1) / steps)
        elif cmd[0] == "info":
            rings, host, handles, nb, _sc, thr = state[cmd[1]]
            mode = [m for m in modes if m[0] == cmd[2]][0]
            p, out, _stream = handles[cmd[2] if mode[3] in ("dev", "host") else "tsq"]
            Cn = len(p.lout)
            info = {"channels": Cn, "blocks": nb, "N": p.N, "R": p.R}
            if mode[3] == "host":
                p.work_raw(host.ctypes.data, nb, None)                            # (the stream goes on from the timed calls: the steady state)
            else:
                p.process_device(rings[0].data_ptr(), 0, nb, out.data_ptr())
                p.synchronize()
            info["describe"] = p.describe()
            if mode[1]:
                mask = p.squelch(nb)
                count = int(p.audio_packed(nb).size)
                rows = p.tones(nb)
                info["open_fraction"] = round(float(mask.mean()), 4)
                info["link_bytes"] = {"packed_audio": 4 * count, "count": 8, "mask": int(mask.size), "levels": 8 * nb * Cn, "rows": int(rows.nbytes)}
                info["unpacked_audio_bytes"] = 4 * nb * (sum(p.lout) // DECIM)
                if mode[2]:
                    dec = p.tone_squelch(nb)
                    info["link_bytes"]["dec"] = int(dec.size)
                    info["dec_open_fraction"] = round(float(dec.mean()), 4) if dec.size else None
                    info.update(thr)
                info["link_bytes"]["total"] = sum(info["link_bytes"].values())
            say(info)
        elif cmd[0] == "close":
            rings, host, handles, _nb, _sc, _thr = state.pop(cmd[1])
            for p, _out, _stream in handles.values():
                p.close()
            G.unregister_host(host)
            del rings, handles, host
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
    ap.add_argument("--host-steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=150.0)
    ap.add_argument("--shapes", default="configs[0],configs[1]")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    builds = [Build("change", ROOT)]
    if a.parent:
        builds += [Build("parent", os.path.abspath(a.parent)), Build("parent_again", os.path.abspath(a.parent))]
    try:
        for shape in a.shapes.split(","):
            pairs = [(b, m) for b in builds for m in b.ask("modes")]
            for b in builds:
                b.ask("open", shape)
            ms = {(b.name, m): [] for b, m in pairs}
            for r in range(a.rounds):
                k = r % len(pairs)
                for b, m in pairs[k:] + pairs[:k]:
                    host = m.startswith("host_")
                    ms[(b.name, m)].append(b.ask("time", shape, m, a.host_steps if host else a.steps, 1 if host else a.warmup, a.settle_ms))
            med = {k: statistics.median(v) for k, v in ms.items()}
            for b, m in pairs:
                res = {"build": b.name, "shape": shape, "mode": m, "ms": round(med[(b.name, m)], 4), "ms_rounds": [round(v, 4) for v in ms[(b.name, m)]],
                       "steps": a.host_steps if m.startswith("host_") else a.steps, "rounds": a.rounds}
                res.update(b.ask("info", shape, m))
                if m == "k_decide_gate":
                    res["gate_ms"] = round(med[(b.name, m)] - med[(b.name, "k_decide")], 4)
                if b.name != "parent" and len(builds) > 1:
                    ref = {"tsq": "carrier", "host_tsq": "host_carrier"}.get(m, m)
                    if ("parent", ref) in med:
                        res["over_parent"] = round(med[(b.name, m)] / med[("parent", ref)], 4)
                        res["parent_mode"] = ref
                print(json.dumps(res), flush=True)
            for b in builds:
                b.ask("close", shape)
    finally:
        for b in builds:
            b.close()


if __name__ == "__main__":
    main()
