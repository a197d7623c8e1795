"""Sink payloads as sc16 / sc8 (fdc_sinks_set_payload_format), narrowed on the device before they leave it.

The reference of every comparison is the float PDU of an untouched FC32 bank on the same input, narrowed in numpy by the rule of the
header: t = float32(y) * float32(scale) per component, rint (half to even), NaN -> 0, clip, cast.  The device multiplies the same float32
values by the same rule, so equality is exact: every metadata field (the time stamp in front of the ID aside) and every payload byte.

The scale comes from the float run — 32767 (sc16) or 127 (sc8) over half the largest component — so that some components saturate: each
test asserts a saturated share above zero and below 5 %, and more than 1000 distinct output values (distinct (I, Q) samples: an int8
component has 256 values at most), so neither the clamp nor the rounding is tested vacuously."""
import ctypes as C

import numpy as np
import pytest

import gr_fdc_amd as G
from gr_fdc_amd import _lib

pytestmark = pytest.mark.gpu

KEYS = ("kind", "source", "chan_id", "finalized", "part", "has_part", "blockstart", "blockend", "vectorstart", "vectorend",
        "rel_bw", "rel_cfreq")
LIMIT = {"sc16": 32767, "sc8": 127}
DTYPE = {"sc16": np.int16, "sc8": np.int8}
N = 4096
CALLS = (7, 16)                      # items of the first two calls; the rest follows (in batches of max_blocks = 16)


def burst_spectrum(nb, bursts, seed, floor=1e-3):
    """normalised-spectrum items: white floor plus rectangular bursts (lo_bin, hi_bin, first_block, last_block, amp)"""
    rng = np.random.default_rng(seed)
    s = floor * (rng.standard_normal((nb, N)) + 1j * rng.standard_normal((nb, N)))
    for lo, hi, b0, b1, amp in bursts:
        s[b0:b1 + 1, lo:hi] += amp * (rng.standard_normal((b1 - b0 + 1, hi - lo)) + 1j * rng.standard_normal((b1 - b0 + 1, hi - lo)))
    return s.astype(np.complex64)


def pac_bursts(plan, spans, amps):
    return [(int(round((cf - bw / 2) * N)), int(round((cf + bw / 2) * N)), b0, b1, amps[i % len(amps)])
            for i, (cf, bw, _id) in enumerate(plan) for (b0, b1) in spans[i]]


def pieces(nb):
    cuts, a = [], 0
    for n in CALLS:
        cuts.append((a, min(nb, a + n)))
        a = min(nb, a + n)
    while a < nb:
        cuts.append((a, min(nb, a + 16)))
        a = min(nb, a + 16)
    return [c for c in cuts if c[1] > c[0]]


def scale_for(ref, fmt):
    top = max(float(np.abs(d.view(np.float32)).max()) for _, d in ref if d.size)
    return np.float32(LIMIT[fmt] / (0.5 * top))


def narrow(y, scale, fmt):
    """the header's rule in numpy: complex64[n] -> int[n, 2]"""
    lim = LIMIT[fmt]
    t = np.rint(y.view(np.float32) * np.float32(scale))
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.clip(t, -lim - 1, lim).astype(DTYPE[fmt]).reshape(-1, 2)


def check_not_vacuous(ref, scale, fmt):
    allq = np.concatenate([narrow(d, scale, fmt) for _, d in ref if d.size])
    sat = float(np.mean((allq == LIMIT[fmt]) | (allq == -LIMIT[fmt] - 1)))
    distinct = len(np.unique(allq.astype(np.int32)[:, 0] * 65536 + allq.astype(np.int32)[:, 1]))
    print("%s: scale %.6g, %d samples, saturated share %.4f, %d distinct samples" % (fmt, scale, allq.shape[0], sat, distinct))
    assert 0.0 < sat < 0.05, sat
    assert distinct > 1000, distinct


def same(got, ref, scale, fmt, what):
    """got: narrow PDUs; ref: float PDUs of the FC32 bank"""
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k, ((mg, dg), (mr, dr)) in enumerate(zip(got, ref)):
        for key in KEYS:
            assert mg[key] == mr[key], (what, k, key, mg, mr)
        assert mg["id"][19:] == mr["id"][19:], (what, k, mg["id"], mr["id"])
        want = narrow(dr, scale, fmt)
        assert dg.dtype == DTYPE[fmt] and dg.shape == want.shape, (what, k, dg.dtype, dg.shape, want.shape)
        assert dg.tobytes() == want.tobytes(), (what, k, int((dg != want).sum()))


_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip


def fetch(pdus, fmt):
    """device payloads (address, sample count) -> arrays, the way tests/test_sinks_engines_gpu.py reads them back"""
    out = []
    for m, (ptr, n) in pdus:
        arr = np.zeros((n, 2), DTYPE[fmt])
        if n:
            assert hip().hipMemcpy(arr.ctypes.data, ptr, arr.nbytes, 2) == 0
        out.append((m, arr))
    return out


def run(bank, spec, mode, fmt=None, routes=None):
    """the stream in calls of 7, 16 and the rest; mode: how the batches reach the bank"""
    got = []

    def note():
        if routes is not None:
            routes.append(bank.payload_route)
    for a, b in pieces(spec.shape[0]):
        blk = np.ascontiguousarray(spec[a:b].reshape(-1))
        if mode == "work":
            got += bank.work(blk); note()
        elif mode == "work_device":
            assert hip().hipMemcpy(bank.spectrum_ptr(), blk.ctypes.data, blk.nbytes, 1) == 0
            got += bank.work_device(b - a); note()
        else:                                                  # two deep: the PDUs of batch k are read while batch k + 1 is in flight
            assert hip().hipMemcpy(bank.spectrum_ptr(), blk.ctypes.data, blk.nbytes, 1) == 0
            p = bank.submit_device(b - a)
            if a:
                note()
            got += fetch(p, fmt) if mode == "devpay" else p
    if mode in ("submit", "devpay"):
        p = bank.flush(); note()
        got += fetch(p, fmt) if mode == "devpay" else p
        assert bank.flush() == []
    return got


# ---------------------------------------------------------------- 1. fused route
FUSED_PLAN = [(0.15, 0.05, 3), (0.35, 0.05, 4), (0.55, 0.05, 5), (0.8, 0.05, 6)]
# batches: [0, 7) [7, 23) [23, 39) [39, 44).  Bursts start in one batch and end in the next; channel 1's spans three batches
FUSED_SPANS = [[(3, 10)], [(5, 30)], [(20, 26), (33, 41)], [(9, 12), (36, 42)]]
FUSED_NB = 44
_fused_ref = {}


def fused_reference(R, maxblocks):
    key = (R, maxblocks)
    if key not in _fused_ref:
        spec = burst_spectrum(FUSED_NB, pac_bursts(FUSED_PLAN, FUSED_SPANS, (1.0, 0.6, 0.35, 0.8)), 31 + R)
        spec.setflags(write=False)
        bank = G.Sinks(N, R, pac=FUSED_PLAN, pac_thresh=6.0, pac_maxblocks=maxblocks, max_blocks=16)
        ref = run(bank, spec, "work")
        assert bank.payload_route == 0 and bank.payload_format == ("fc32", 1.0)
        _fused_ref[key] = (spec, ref)
    return _fused_ref[key]


@pytest.mark.parametrize("fmt", ["sc16", "sc8"])
@pytest.mark.parametrize("maxblocks", [-1, 3])
@pytest.mark.parametrize("R", [2, 4])
def test_fused_route_256_bin_bank(R, maxblocks, fmt):
    """Four 256-bin PowerActivationChannels: k_x256 and the carry copy store the emitted runs narrow themselves (route 2), through every
    way a batch reaches the bank; bursts cross one and two batch boundaries, maxblocks = 3 forces `part` emissions."""
    spec, ref = fused_reference(R, maxblocks)
    assert len(ref) >= (6 if maxblocks < 0 else 12)
    assert any(m["blockend"] - m["blockstart"] > 16 for m, _ in ref) or maxblocks == 3     # a PDU that collects three batches
    scale = scale_for(ref, fmt)
    check_not_vacuous(ref, scale, fmt)
    for mode, extra in (("work", {}), ("work_device", {}), ("submit", {}), ("work", dict(lookahead=True)), ("devpay", dict(device_payload=True))):
        bank = G.Sinks(N, R, pac=FUSED_PLAN, pac_thresh=6.0, pac_maxblocks=maxblocks, max_blocks=16, **extra)
        assert [bank.pac_params(i)["extract_width"] for i in range(4)] == [256] * 4
        bank.set_payload_format(fmt, scale)
        assert bank.payload_format == (fmt, float(scale))
        routes = []
        got = run(bank, spec, mode, fmt, routes)
        assert routes and all(r == 2 for r in routes), (mode, extra, routes)
        same(got, ref, scale, fmt, "fused %s %s" % (mode, extra))


# ---------------------------------------------------------------- 2. narrowed route
@pytest.mark.parametrize("fmt", ["sc16", "sc8"])
@pytest.mark.parametrize("variant", [0, 1])
def test_narrowed_route_mixed_width_classes(variant, fmt):
    """PowerActivationChannels of 64, 256 and 1024 bins plus a detection segment in one bank: the batch runs as in FC32 and one pass narrows
    the emitted runs (route 1)."""
    R, nb = 2, 40
    plan = [(0.05, 0.012, 1), (0.15, 0.05, 2), (0.35, 0.2, 3)]
    spans = [[(2, 9), (20, 30)], [(5, 25)], [(4, 8), (21, 37)]]
    bursts = pac_bursts(plan, spans, (1.0, 0.7, 0.3))
    for lo, hi, b0, b1 in ((0.62, 0.64, 3, 12), (0.7, 0.73, 6, 27), (0.8, 0.81, 20, 36)):
        bursts.append((int(lo * N), int(hi * N), b0, b1, 0.5))
    spec = burst_spectrum(nb, bursts, 5 + variant)
    kw = dict(pac=plan, pac_thresh=6.0, pac_maxblocks=5, segments=[(0.6, 0.95)], det_thresh=10.0, det_maxblocks=4, minchandist=0.005,
              det_delay=1, puffer=0.2, max_blocks=16, det_variant=variant)
    fbank = G.Sinks(N, R, **kw)
    assert [fbank.pac_params(i)["extract_width"] for i in range(3)] == [64, 256, 1024]
    ref = run(fbank, spec, "work")
    assert sum(m["kind"] == 0 for m, _ in ref) >= 6 and sum(m["kind"] == 1 for m, _ in ref) >= 3
    scale = scale_for(ref, fmt)
    check_not_vacuous(ref, scale, fmt)
    for mode in ("work", "submit"):
        bank = G.Sinks(N, R, **kw)
        bank.set_payload_format(fmt, scale)
        routes = []
        got = run(bank, spec, mode, fmt, routes)
        assert routes and all(r == 1 for r in routes), routes
        same(got, ref, scale, fmt, "narrowed variant %d %s" % (variant, mode))


# ---------------------------------------------------------------- 3. odd landing offsets
@pytest.mark.parametrize("fmt", ["sc8", "sc16"])
def test_odd_landing_offsets(fmt):
    """R = 16 and a 16-bin channel: 15 samples per block, and its first emitted run has an odd block count — the runs behind it start at odd
    sample offsets (2-byte aligned sc8 samples, the scalar path of the carry copy, the padded start of the buffered rests)."""
    R, nb = 16, 40
    plan = [(0.1, 0.003, 1), (0.3, 0.05, 2), (0.5, 0.006, 3), (0.7, 0.05, 4)]
    spans = [[(2, 4), (11, 21), (30, 34)], [(3, 12), (18, 31)], [(4, 8), (20, 24)], [(5, 26)]]
    spec = burst_spectrum(nb, pac_bursts(plan, spans, (1.0, 0.5, 0.8, 0.3)), 9)
    kw = dict(pac=plan, pac_thresh=6.0, pac_maxblocks=-1, max_blocks=16)
    fbank = G.Sinks(N, R, **kw)
    assert [fbank.pac_params(i)["extract_width"] for i in range(4)] == [16, 256, 32, 256]
    assert fbank.pac_params(0)["output_len"] == 15
    ref = run(fbank, spec, "work")
    # the first PDU of the first call: channel 1's burst of blocks 2..4 — an odd number of 15-sample blocks in front of every later run
    first = ref[0]
    assert first[0]["source"] == 1 and first[1].size % 2 == 1 and len(ref) >= 8
    scale = scale_for(ref, fmt)
    check_not_vacuous(ref, scale, fmt)
    for mode in ("work", "submit", "devpay"):
        bank = G.Sinks(N, R, device_payload=mode == "devpay", **kw)
        bank.set_payload_format(fmt, scale)
        routes = []
        got = run(bank, spec, mode, fmt, routes)
        assert all(r == 1 for r in routes), routes
        same(got, ref, scale, fmt, "odd offsets %s" % mode)


# ---------------------------------------------------------------- 4. setter semantics
def test_setter_semantics():
    R = 2
    spec, ref = fused_reference(R, -1)
    L = _lib.lib()
    bank = G.Sinks(N, R, pac=FUSED_PLAN, pac_thresh=6.0, pac_maxblocks=-1, max_blocks=16)
    # refusals change nothing
    for bad in (3, -1, 77):
        assert L.fdc_sinks_set_payload_format(bank._h, bad, 1.0) == -1
    for bad in (0.0, float("inf"), float("-inf"), float("nan")):
        assert L.fdc_sinks_set_payload_format(bank._h, _lib.FDC_OQ_SC16, bad) == -1
        with pytest.raises(ValueError):
            bank.set_payload_format("sc16", bad)
    with pytest.raises(ValueError):
        bank.set_payload_format("sc12")
    assert bank.payload_format == ("fc32", 1.0)
    # between submit and flush
    blk = np.ascontiguousarray(spec[:7].reshape(-1))
    assert hip().hipMemcpy(bank.spectrum_ptr(), blk.ctypes.data, blk.nbytes, 1) == 0
    bank.submit_device(7)
    with pytest.raises(ValueError):
        bank.set_payload_format("sc16", 100.0)
    assert bank.payload_format == ("fc32", 1.0)
    assert len(bank.flush()) >= 0
    # a host-engine bank: sc16 unsupported, FC32 accepted
    host = G.Sinks(N, R, pac=FUSED_PLAN, pac_thresh=6.0, pac_maxblocks=-1, max_blocks=16, host_decisions=True)
    assert host.engine() == 0
    assert L.fdc_sinks_set_payload_format(host._h, _lib.FDC_OQ_SC16, 1.0) == -4
    with pytest.raises(_lib.FdcError):
        host.set_payload_format("sc8", 2.0)
    host.set_payload_format("fc32", 1.0)
    assert host.payload_format == ("fc32", 1.0)
    # a successful set drops the current PDUs
    bank = G.Sinks(N, R, pac=FUSED_PLAN, pac_thresh=6.0, pac_maxblocks=-1, max_blocks=16)
    scale = scale_for(ref, "sc16")
    bank.set_payload_format("sc16", scale)
    a, b = pieces(FUSED_NB)[0], pieces(FUSED_NB)[1]
    got = bank.work(spec[a[0]:a[1]].reshape(-1)) + bank.work(spec[b[0]:b[1]].reshape(-1))
    assert L.fdc_sinks_pdu_count(bank._h) > 0 and len(got) > 0
    # sc16 -> FC32 in mid-stream (nothing in flight): what follows equals a bank that was FC32 throughout — also the PDUs whose first blocks were
    # buffered while sc16 was set (channel 1's burst runs from block 5 to 30): the buffered blocks stay float
    bank.set_payload_format("fc32")
    assert L.fdc_sinks_pdu_count(bank._h) == 0 and bank.pdus() == []
    rest = []
    for (p, q) in pieces(FUSED_NB)[2:]:
        rest += bank.work(spec[p:q].reshape(-1))
    assert bank.payload_route == 0
    same(got, ref[:len(got)], scale, "sc16", "before the change")
    tail = ref[len(got):]
    assert len(rest) == len(tail) and any(m["blockstart"] < 23 <= m["blockend"] for m, _ in tail)
    for (mg, dg), (mr, dr) in zip(rest, tail):
        assert all(mg[k] == mr[k] for k in KEYS) and mg["id"][19:] == mr["id"][19:]
        assert dg.dtype == np.complex64 and dg.tobytes() == dr.tobytes()


# ---------------------------------------------------------------- 5. group
@pytest.mark.parametrize("fmt", ["sc16", "sc8"])
def test_group_emits_one_banks_pdus_narrow(fmt):
    R = 2
    spec, ref = fused_reference(R, 3)
    scale = scale_for(ref, fmt)
    grp = G.SinksGroup(N, R, [0, 0], pac=FUSED_PLAN, pac_thresh=6.0, pac_maxblocks=3, max_blocks=16)
    assert grp.size() == 2
    grp.set_payload_format(fmt, scale)
    assert grp.payload_format == (fmt, float(scale))
    got = run(grp, spec, "work")
    assert grp.payload_route == [2, 2]
    same(got, ref, scale, fmt, "group")
    with pytest.raises(ValueError):
        grp.set_payload_format(fmt, 0.0)


# ---------------------------------------------------------------- 6. hier block
@pytest.mark.parametrize("pipelined", [False, True])
def test_hier_block_payload_format(pipelined, tmp_path):
    """FrequencyDomainChannelizer(..., payload_format="sc16"): ragged calls, then flush(); the same PDUs in the same order as the same block
    without the setting, payloads equal to its payloads narrowed, output files of nsamples * 4 bytes."""
    import os
    R, sizes = 4, [5, 8, 1, 8, 2, 7, 8, 3]
    nb, H = sum(sizes), N - N // R
    # noise floor plus bursty carriers of band-limited GAUSSIAN noise (a constant-envelope carrier would saturate in most samples at this scale)
    rng = np.random.default_rng(8)
    n = np.arange(nb * H)
    x = 0.01 * (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H))
    for fc, t0, t1, amp in [(-0.2, 3, 9, 1.0), (0.31, 6, 15, 0.5), (-0.2, 17, 22, 0.7), (0.33, 20, nb - 2, 0.35)]:
        w = rng.standard_normal((t1 - t0) * H + 31) + 1j * rng.standard_normal((t1 - t0) * H + 31)
        base = np.convolve(w, np.ones(32) / np.sqrt(32.0), mode="valid")
        x[t0 * H:t1 * H] += amp * base * np.exp(2j * np.pi * fc * n[t0 * H:t1 * H])
    x = x.astype(np.complex64)
    dirs = [tmp_path / "float", tmp_path / "narrow"]
    for d in dirs:
        d.mkdir()

    def args(path):
        return (8, 1, N, R, [[0.1, 0.05]], [[-0.2, 0.04]], 6.0, 1.0, 0.0, 'normalized', 1,
                True, True, str(path), False, [[0.25, 0.4]], 10.0, 0.005, 1, 0.2, 0, 0, 3, 3, False)
    cuts = np.cumsum([0] + sizes)

    def stream(block):
        msgs = []
        for i in range(len(sizes)):
            block.work(x[cuts[i] * H:cuts[i + 1] * H])
            msgs += block.messages
        msgs += block.flush()
        assert block.flush() == []
        return msgs
    ref = stream(G.FrequencyDomainChannelizer(*args(dirs[0]), max_blocks=max(sizes), pipelined=pipelined))
    assert len(ref) >= 4
    top = max(float(np.abs(d.view(np.float32)).max()) for _, d in ref if d.size)
    scale = np.float32(32767 / (0.5 * top))
    allq = np.concatenate([narrow(d, scale, "sc16") for _, d in ref if d.size])
    sat = float(np.mean((allq == 32767) | (allq == -32768)))
    assert 0.0 < sat < 0.05 and len(np.unique(allq)) > 1000, (sat, len(np.unique(allq)))
    blk = G.FrequencyDomainChannelizer(*args(dirs[1]), max_blocks=max(sizes), pipelined=pipelined, payload_format="sc16", payload_scale=scale)
    assert blk.sinks.payload_format == ("sc16", float(scale))
    got = stream(blk)
    assert len(got) == len(ref)
    for (gd, gs), (rd, rs) in zip(got, ref):
        assert {k: gd[k] for k in gd if k != "ID"} == {k: rd[k] for k in rd if k != "ID"}
        assert gd["ID"][19:] == rd["ID"][19:]
        want = narrow(rs, scale, "sc16")
        assert gs.dtype == np.int16 and gs.shape == want.shape and gs.tobytes() == want.tobytes()
    # files: the narrow bytes as they are, under the names the float block writes (time stamp aside: compared by what follows it)
    fl = sorted(os.listdir(dirs[0]), key=lambda s: s[19:])
    nr = sorted(os.listdir(dirs[1]), key=lambda s: s[19:])
    assert [s[19:] for s in fl] == [s[19:] for s in nr] and len(nr) == len({s[19:] for s in nr}) >= 4
    for a, b in zip(fl, nr):
        y = np.fromfile(dirs[0] / a, dtype=np.complex64)
        raw = np.fromfile(dirs[1] / b, dtype=np.int16)
        assert raw.nbytes == y.size * 4
        assert raw.tobytes() == narrow(y, scale, "sc16").tobytes()
    with pytest.raises(ValueError):
        a = list(args(dirs[1])); a[20] = 1
        G.FrequencyDomainChannelizer(*a, max_blocks=8, payload_format="sc16")
