"""Generates the committed fixtures in tests/golden/.  Run in the BUILD container only
(`python tests/golden/make_golden.py`); needs oracle/_ref (built from /root/reference/lib/windows.h
by oracle/Makefile) for the window tables.

Fixtures are DATA (inputs + expected outputs):
  windows_ref.npz      tables produced by the reference's own cr_win (lib/windows.h:41-78), unmodified,
                       through oracle/ref_windows_driver.cpp.
  windows_ref_seeded.npz  the same, on 60 seeded random parameter sets (SEEDED_WINDOW_CASES).
  channel_params.json  NOT made here: tests/golden/make_params_from_reference.py produces it by running the
                       reference's own get_opt_channelparams / frequency-mode lambdas.
  chain_numpy.npz      the throughput chain evaluated with numpy.fft in
                       complex128 — an implementation independent of oracle/fdc_oracle.c — on seeded
                       multicarrier input, float32-rounded at the reference's stage boundaries.
  sink_known_answers.json  PDU metadata of three cases from the reference's own sink blocks, compiled where they lie into
                       oracle/_ref/libref_sinks.so (sink_known_answers() below).
  sink_ref_runs.npz    NOT made here: tests/golden/make_sink_ref_runs.py records the reference's sink blocks on seeded cases.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import oracle as O  # noqa: E402

WINDOW_CASES = [  # (wintype, l, passbw, stopbw, R)
    (t, l, p, s, R)
    for t in (0, 1, 2)
    for (l, p, s, R) in [(256, 0.88, 1.0, 2), (256, 0.88, 1.0, 4), (1024, 0.528, 0.778, 4),
                         (512, 0.7128, 1.0, 8), (64, 1.0, 1.0, 2), (16, 0.3, 0.55, 4), (2, 0.5, 0.75, 2),
                         (128, 0.4, 0.65, 2), (4096, 0.6, 0.85, 2)]
]


def make_windows():
    assert O.have_ref(), "oracle/_ref missing: run `make -C oracle` with /root/reference present"
    d = {}
    for i, (t, l, p, s, R) in enumerate(WINDOW_CASES):
        d["case%02d" % i] = O.ref_window(t, l, np.float32(p), np.float32(s), R)
    d["params"] = np.array(WINDOW_CASES, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "windows_ref.npz"), **d)


def SEEDED_WINDOW_CASES():
    """60 random (wintype, l, passbw, stopbw, R), seed 7; passbw/stopbw are float32."""
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(60):
        t = int(rng.integers(0, 3)); l = int(2 ** rng.integers(1, 12)); R = int(2 ** rng.integers(1, 4))
        p = np.float32(rng.uniform(0.05, 1.1)); s = np.float32(p + rng.uniform(0, 0.5))
        cases.append((t, l, p, s, R))
    return cases


def make_windows_seeded():
    assert O.have_ref(), "oracle/_ref missing: run `make -C oracle` with /root/reference present"
    cases = SEEDED_WINDOW_CASES()
    d = {"case%02d" % i: O.ref_window(t, l, p, s, R) for i, (t, l, p, s, R) in enumerate(cases)}
    d["params"] = np.array(cases, dtype=np.float64)      # float32 passbw/stopbw are exact in float64
    np.savez_compressed(os.path.join(HERE, "windows_ref_seeded.npz"), **d)


def multicarrier(N, chans, nsamp, seed, noise=0.1):
    """One QPSK-like carrier per channel (rect-shaped random symbols at 0.6x the channel bandwidth)
    plus complex white noise."""
    rng = np.random.default_rng(seed)
    n = np.arange(nsamp)
    x = noise * (rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp)) / np.sqrt(2)
    for (f, l, _p, _s) in chans:
        sps = max(2, int(round(N / (0.6 * l))))
        nsym = nsamp // sps + 2
        sym = (rng.integers(0, 2, nsym) * 2 - 1) + 1j * (rng.integers(0, 2, nsym) * 2 - 1)
        base = np.repeat(sym, sps)[:nsamp] / np.sqrt(2)
        fc = (f + l / 2 - N / 2) / N
        x = x + base * np.exp(2j * np.pi * fc * n)
    return x.astype(np.complex64)


def numpy_chain(N, R, wintype, chans, x):
    """App. A.1-A.4 with numpy.fft (complex128), float32 at the reference's stage boundaries.  A restatement by reading, kept because it
    documents the algorithm line by line; the reference's own run (oracle/ref_hier.py, tests/test_hier_reference_cpu.py) now judges the
    oracle that this function cross-checks, and so this function too."""
    ovl = N // R
    H = N - ovl
    nb = x.size // H
    xp = np.concatenate([np.zeros(ovl, np.complex64), x])
    outs = [[] for _ in chans]
    for m in range(nb):
        blk = xp[m * H: m * H + N].astype(np.complex128)
        S = np.fft.fftshift(np.fft.fft(blk)).astype(np.complex64)
        X = (S * np.float32(1.0 / N)).astype(np.complex64)
        for ci, (f, l, p, s) in enumerate(chans):
            W = O.ref_window(wintype, l, np.float32(p), np.float32(s), R)
            cnt = (m * (f % R)) % R
            a = X[f:f + l]
            w = W[cnt]
            yr = (a.real * w.real).astype(np.float32) - (a.imag * w.imag).astype(np.float32)
            yi = (a.real * w.imag).astype(np.float32) + (a.imag * w.real).astype(np.float32)
            Y = (yr.astype(np.float32) + 1j * yi.astype(np.float32)).astype(np.complex64)
            y = (np.fft.ifft(np.fft.ifftshift(Y.astype(np.complex128))) * l).astype(np.complex64)
            lout = l - l // R
            outs[ci].append((y[l - lout:] * np.float32(l)).astype(np.complex64))
    return [np.concatenate(o) for o in outs]


def make_chain():
    d = {}
    cases = []
    # cfg1: the example flowgraph's four channels (examples/FDC_example.grc), R = 2 and R = 4,
    # plus the same plan shifted by +1 bin so f is odd (exercises the phase rotation, App. B.8)
    user = [(0.12, 0.05), (0.22, 0.1), (-0.14, 0.12), (0.0, 0.081)]
    for name, N, R, shiftbin, wt, nb in [("cfg1_R2", 4096, 2, 0, 1, 8), ("cfg1_R4_odd", 4096, 4, 1, 1, 8),
                                         ("cfg1_R2_odd_rect", 4096, 2, 1, 0, 6), ("cfg1_R8_ramp", 4096, 8, 3, 2, 6)]:
        chans = []
        for (u, bw) in user:
            f, l, lout, p, s = O.channel_params(N, R, (u + 0.5) % 1.0, bw % 1.0)
            chans.append((min(f + shiftbin, N - l), l, p, s))
        H = N - N // R
        x = multicarrier(N, chans, nb * H, 1234)
        outs = numpy_chain(N, R, wt, chans, x)
        d[name + "_x"] = x
        for i, o in enumerate(outs):
            d[name + "_out%d" % i] = o
        cases.append(dict(name=name, N=N, R=R, wintype=wt, nblocks=nb,
                          chans=[[int(c[0]), int(c[1]), float(c[2]), float(c[3])] for c in chans]))
    d["cases"] = np.array(json.dumps(cases))
    np.savez_compressed(os.path.join(HERE, "chain_numpy.npz"), **d)


def _known_answer_spectrum():
    """burst_spectrum(4096, 12, [(1600, 1800, 3, 7, 1.0)], 0) of tests/test_sinks_gpu.py: bins 1600-1799 active in blocks 3-7"""
    N, nb = 4096, 12
    rng = np.random.default_rng(0)
    s = 1e-3 * (rng.standard_normal((nb, N)) + 1j * rng.standard_normal((nb, N)))
    s[3:8, 1600:1800] += 1.0 * (rng.standard_normal((5, 200)) + 1j * rng.standard_normal((5, 200)))
    return s.astype(np.complex64)


def sink_known_answers():
    """The three known-answer cases of tests/test_sinks_gpu.py through the reference's OWN sink blocks (oracle/_ref/libref_sinks.so:
    lib/*_impl.cc compiled where they lie over oracle/ref_standins/, recipe `make -C oracle ref`)."""
    N, R = 4096, 4
    spec = _known_answer_spectrum()
    (p,) = O.RefPowerActivationChannel(N, (1600 + 1800) / 2 / N, 200 / N, R, 6.0, -1, 0, 0).work(spec)
    (v,) = O.RefActivityDetectionVcm(N, [[0.3, 0.55]], 10.0, R, -1, 0.005, 1, 0.2).work(spec)
    (d,) = O.RefSegmentDetection(0, N, R, 0.3, 0.55, 10.0, 0.005, 0.2, -1, 1).work(spec)

    def det(m):
        return dict(vectorstart=int(m["vectorstart"]), vectorend=int(m["vectorend"]), rel_bw=float(m["rel_bw"]),
                    blockstart=int(m["blockstart"]), blockend=int(m["blockend"]), nsamples=int(m["samples"].size))
    return {
        "source": "the reference's own sink blocks, compiled by `make -C oracle ref` into oracle/_ref/libref_sinks.so over the stand-ins of "
                  "oracle/ref_standins/, fed a synthetic burst (bins 1600-1799 active in blocks 3-7, N=4096, R=4); "
                  "tests/golden/make_golden.py sink_known_answers()",
        "PowerActivationChannel": dict(rel_bw=float(p["rel_bw"]), blockstart=int(p["blockstart"]), blockend=int(p["blockend"]),
                                       nsamples=int(p["samples"].size)),
        "SegmentDetection": det(d),
        "activity_detection_channelizer_vcm": det(v),
    }


def make_sink_known_answers():
    with open(os.path.join(HERE, "sink_known_answers.json"), "w") as fh:
        json.dump(sink_known_answers(), fh, indent=1)


if __name__ == "__main__":
    make_windows()
    make_windows_seeded()
    make_chain()
    make_sink_known_answers()
    print("fixtures written to", HERE)
