"""Cost and gain of the packed channel audio (fdc_pipeline_set_audio_packing), this tree and a parent build interleaved in one session: one JSON line
per build, plan and mode.

AT FULL OCCUPANCY THE PACKED HOST STEP PAYS A SECOND SYNCHRONISE AND SAVES NOTHING: profiles/audiopack/README.md has the measured ratio; leave the
packing off on a band whose channels are mostly open.

Plans: configs[0] (the example flowgraph's 4096-pt plan, 16384 blocks a step: FOUR channels and many blocks, 65536 cells) and configs[1] (65536-pt FFT,
R = 2, 256 channels of 256 bins, 2048 blocks a step: 524288 cells).  FM, the audio filter D = 8, K = 64 from lowpass_taps, float32.  Occupancies: `open`
(thresholds 0: every cell open), `part` (every eighth channel open on configs[1], one channel of four on configs[0]), `closed` (thresholds no power
reaches).  Modes, on the device-resident entry (HIP events on the handle's stream):
  off              every setting off (the condition "nothing changes while it is off": this tree against the parent)
  lev, fm_lev      the levels alone; the levels and FM
  lev_sq           the levels and the squelch: squelch_ms = ms(lev_sq) - ms(lev), the time of k_chan_squelch
  gate_<occ>       levels, FM, audio and squelch: the GATED pass, gated_ms = ms - ms(fm_lev) - squelch_ms (both builds: the parent's is the yardstick)
  pack_<occ>       the same with the packing on: packed_ms = ms - ms(fm_lev) - squelch_ms is the three offsets launches and the PACK pass together
  offsets_<occ>    fdc_pipeline_audio_pack_offsets_device alone over the mask of pack_<occ>'s last call: offsets_ms, the three launches
and on the host entry, work() from a registered (pinned) host buffer, wall clock around the call (it synchronises itself):
  host_gate_<occ>  the gated, unpacked form (both builds)
  host_pack_<occ>  the packed form; link_bytes: what the call copies home (audio or packed audio, mask, count, levels), computed from the shapes
                   Both include what Pipeline.work() does on top in numpy (slicing the matrix per channel, or gathering every channel's open blocks
                   with unpack_audio): the C entry alone is not timed here
packed_over_gated = packed_ms / the PARENT's gated_ms (this tree's without a parent); host_packed_over_gated likewise for the host step.

Every build runs in a worker process of its own (this file with --worker) that keeps its handles and answers one timing at a time, so the driver
interleaves the builds: per round every (build, mode) pair once, the order rotated from round to round.  ms = the median over the rounds.

usage: python tools/audio_pack_bench.py [--parent DIR] [--steps 20] [--host-steps 6] [--warmup 3] [--rounds 5] [--settle-ms 150]
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
OCC = ("open", "part", "closed")
# (name, levels, demodulation, audio, squelch occupancy or None, packing, entry: "dev" / "host" / "offsets")
MODES = ([("off", False, None, False, None, False, "dev"), ("lev", True, None, False, None, False, "dev"), ("fm_lev", True, "fm", False, None, False, "dev"),
          ("lev_sq", True, None, False, "part", False, "dev")]
         + [("gate_" + o, True, "fm", True, o, False, "dev") for o in OCC] + [("pack_" + o, True, "fm", True, o, True, "dev") for o in OCC]
         + [("offsets_" + o, True, "fm", True, o, True, "offsets") for o in OCC]
         + [("host_gate_" + o, True, "fm", True, o, False, "host") for o in OCC] + [("host_pack_" + o, True, "fm", True, o, True, "host") for o in OCC])


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
    have = hasattr(G.Pipeline, "set_audio_packing")
    modes = [m for m in MODES if have or not m[5]]
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
            host = base[2 * ovl:].copy().view(np.complex64)                      # the host entry's input: nb * H complex samples, registered (pinned)
            G.register_host(host)
            handles = {}
            for mname, lev, dem, aud, sq, pack, entry in modes:
                if entry == "offsets":
                    continue                                                      # (it runs on pack_<occ>'s handle)
                p = G.Pipeline(N, R, plan, windowtype=1, max_blocks=nb)
                if lev:
                    p.set_levels(True)
                if dem:
                    p.set_demod(dem, 0.15915494)
                if aud:
                    p.set_audio(DECIM, G.lowpass_taps(DECIM, NTAPS), "f32")
                if sq:
                    C = len(p.lout)
                    closed = np.full(C, 3e38, np.float32)
                    thr = {"open": np.zeros(C, np.float32), "closed": closed,
                           "part": np.where(np.arange(C) % (8 if C > 4 else 4) == 0, np.float32(0), closed)}[sq]
                    p.set_squelch(thr, thr, 2)
                if pack:
                    p.set_audio_packing(True)
                # (a buffer of the complex float size serves every mode: the real outputs use its first half)
                handles[mname] = (p, torch.empty(2 * p.output_samples(nb), dtype=torch.float32, device="cuda"), torch.cuda.ExternalStream(p.stream()))
            scratch = (torch.empty(nb * len(plan), dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda"))
            state[cmd[1]] = (rings, host, handles, nb, scratch)
            say("ok")
        elif cmd[0] == "time":
            rings, host, handles, nb, scratch = state[cmd[1]]
            entry = [m[6] for m in modes if m[0] == cmd[2]][0]
            p, out, stream = handles[cmd[2].replace("offsets_", "pack_")]
            steps, warmup, settle = int(cmd[3]), int(cmd[4]), float(cmd[5])
            if entry == "host":
                step = lambda i: p.work(host)                                                               # noqa: E731
            elif entry == "offsets":
                p.process_device(rings[0].data_ptr(), 0, nb, out.data_ptr())                                # (the mask of this occupancy)
                p.synchronize()
                step = lambda i: p.audio_pack_offsets_device(p.squelch_device(), scratch[0].data_ptr(), scratch[1].data_ptr(), nb)   # noqa: E731
            else:
                step = lambda i: p.process_device(rings[i % 3].data_ptr(), 0, nb, out.data_ptr())           # noqa: E731
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
            rings, host, handles, nb, _scratch = state[cmd[1]]
            p, out, _stream = handles[cmd[2].replace("offsets_", "pack_")]
            p.process_device(rings[0].data_ptr(), 0, nb, out.data_ptr())
            p.synchronize()
            C, A = len(p.lout), sum(p.lout) // DECIM
            info = {"describe": p.describe(), "channels": C, "blocks": nb, "N": p.N, "R": p.R, "cells": nb * C}
            if p.squelch_setting() is not None:
                mask = p.squelch(nb)
                info["open_fraction"] = round(float(mask.mean()), 4)
                if cmd[2].startswith("host"):
                    count = int((mask.astype(np.int64) * (np.array(p.lout) // DECIM)[None, :]).sum())
                    info["link_bytes"] = (4 * count + 8 if "pack" in cmd[2] else 4 * nb * A) + nb * C + 8 * nb * C
                    info["audio_link_bytes"] = 4 * count if "pack" in cmd[2] else 4 * nb * A
            say(info)
        elif cmd[0] == "close":
            rings, host, handles, _nb, _scratch = state.pop(cmd[1])
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
    ap.add_argument("--host-steps", type=int, default=6)
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
                    host = m.startswith("host")
                    ms[(b.name, m)].append(b.ask("time", shape, m, a.host_steps if host else a.steps, 1 if host else a.warmup, a.settle_ms))
            med = {k: statistics.median(v) for k, v in ms.items()}
            yard = "parent" if len(builds) > 1 else "change"
            own = lambda bn, m: med[(bn, m)] - med[(bn, "fm_lev")] - (med[(bn, "lev_sq")] - med[(bn, "lev")])      # noqa: E731
            for b, m in pairs:
                res = {"build": b.name, "shape": shape, "mode": m, "ms": round(med[(b.name, m)], 4), "ms_rounds": [round(v, 4) for v in ms[(b.name, m)]],
                       "steps": a.host_steps if m.startswith("host") else a.steps, "rounds": a.rounds}
                res.update(b.ask("info", shape, m))
                if m == "lev_sq":
                    res["squelch_ms"] = round(med[(b.name, "lev_sq")] - med[(b.name, "lev")], 4)
                if m.startswith("gate_"):
                    res["gated_ms"] = round(own(b.name, m), 4)
                if m.startswith("pack_"):
                    g = own(yard, m.replace("pack_", "gate_"))
                    res["packed_ms"] = round(own(b.name, m), 4)
                    res["packed_over_gated"] = round(own(b.name, m) / g, 3) if g > 0 else None
                if m.startswith("offsets_"):
                    sq = med[(b.name, "lev_sq")] - med[(b.name, "lev")]
                    res["offsets_ms"] = res["ms"]
                    res["offsets_over_squelch"] = round(med[(b.name, m)] / sq, 3) if sq > 0 else None
                if m.startswith("host") and "_pack_" in m:
                    res["host_packed_over_gated"] = round(med[(b.name, m)] / med[(yard, m.replace("_pack_", "_gate_"))], 4)
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
