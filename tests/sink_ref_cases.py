"""Seeded cases for the three stateful sink blocks, shared by the differential fuzz of the compiled reference against the oracle
(tests/test_sinks_reference_cpu.py), the recorder of reference runs (tests/golden/make_sink_ref_runs.py) and the GPU tests that
hold the device against those recordings (tests/test_sinks_reference_gpu.py).  Nothing here reads the reference or the oracle:
a case is its constructor arguments and an input that both sides regenerate from the seed (numpy.random.default_rng streams are
stable across numpy versions; the recordings store a CRC of every input all the same).

Two input classes:

exact   Every bin carries an amplitude from {1, 2, 4, 8, 16, 32} times a phase from {1, i, -1, -i}; floor 1, bursts are rectangles
        in (bin, block).  Every |x|^2 is an integer <= 1024 and every sum of them an integer < 2^24: exact in float32 in ANY
        summation order.  What follows a sum is one correctly rounded operation (a product with 1/dec, a quotient), so no decision
        can depend on how a kernel orders its additions.  Thresholds come from EXACT_DB, none of which is 10 log10 of a ratio two
        such sums can have; margin() measures how close any quotient of a case comes to its threshold and the tests assert that it
        stays away by more than 1e-4 relative (a float32 quotient is good to 6e-8).
noisy   burst_spectrum of tests/test_sinks_gpu.py: Gaussian floor 1e-3, Gaussian bursts of amplitude 0.05 ... 1 (34-60 dB over the
        floor), thresholds 6-15 dB.  Decisions here CAN depend on rounding; a noisy case is used only where the compiled reference
        gives the same metadata for the input and for the input plus noise 100 dB under the strongest burst (perturbed()).  The power
        cells hold at least 16 bins (32 below 9 dB) so that the floor's own fluctuation does not sit at the threshold.
"""
import zlib

import numpy as np

GEN_VERSION = 2
BLOCKS = ("pac", "vcm", "sd")
AMPS = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
EXACT_DB = (3.3, 5.1, 7.3, 9.1, 11.7, 13.3)
N_FUZZ = 300            # per block; indices 0 .. N_FUZZ-1, two thirds exact, one third noisy
RECORDED = 44           # per block: the first RECORDED indices of the fuzz are recorded for the GPU machine (noisy ones if stable)


def klass_of(index):
    return "noisy" if index % 3 == 2 else "exact"


def _seed(block, index):
    return 1000003 * (BLOCKS.index(block) + 1) + 7919 * index + GEN_VERSION


def crc(spec):
    return zlib.crc32(np.ascontiguousarray(spec, dtype=np.complex64).tobytes()) & 0xFFFFFFFF


def _geometry_vcm(N, seg, dec):
    """activity_detection_channelizer_vcm's segment in bins, as the block's documentation describes it (rounded centre and
    width, width raised to a multiple of the decimation) — used only to PLACE bursts, never to judge a result."""
    mid, width = int(round((seg[0] + seg[1]) * 0.5 * N)), int(round((seg[1] - seg[0]) * N))
    if width % dec:
        width += dec - width % dec
    start = max(0, mid - width // 2)
    return start, start + width


def _phases(rng, shape):
    return np.array([1, 1j, -1, -1j], dtype=np.complex128)[rng.integers(0, 4, shape)]


def _runs(rng, nb, first_on=None):
    """on/off pattern over nb blocks in runs of 1-5; may start `on` in block 0 and may still be on in the last block"""
    on = bool(rng.integers(0, 2)) if first_on is None else first_on
    out, m = np.zeros(nb, dtype=bool), 0
    while m < nb:
        ln = int(rng.integers(1, 6))
        out[m:m + ln] = on
        m += ln
        on = not on
    return out


# ---------------------------------------------------------------------------------------------------------------- PowerActivationChannel
def _pac_case(index, klass, rng):
    N = int(rng.choice([256, 1024, 4096]))
    R = int(rng.choice([2, 4, 8]))
    nb = int(rng.integers(10, 25))
    nch = int(rng.integers(1, 4))
    chans, spans = [], []
    for c in range(nch):                                  # disjoint slots of a third of the band each
        lo_f, hi_f = c / 3.0 + 0.02, (c + 1) / 3.0 - 0.02
        bw = float(rng.uniform(16.5 / N if klass == "noisy" else 3.0 / N, min(0.12, (hi_f - lo_f) / 2)))
        cf = float(rng.uniform(lo_f + bw / 2, hi_f - bw / 2))
        if rng.integers(0, 6) == 0 and c == nch - 1:      # now and then a channel against the upper band edge
            cf = float(np.float32(1.0 - bw / 2 - 1e-3))
        cf, bw = float(np.float32(cf)), float(np.float32(bw))
        chans.append((cf, bw, 10 * index % 97 + c))
        spans.append((int(round((cf - bw / 2) * N)), int(round((cf + bw / 2) * N))))
    thresh = float(rng.choice(EXACT_DB)) if klass == "exact" else float(np.float32(rng.uniform(6.0, 15.0)))
    args = dict(N=N, R=R, chans=chans, thresh=thresh, maxblocks=int(rng.choice([-1, 0, 1, 3])), delay=int(rng.integers(0, 4)))
    if klass == "exact":
        amp = np.ones((nb, N))
        for lo, hi in spans:
            on = _runs(rng, nb)
            level = rng.choice(AMPS[2:], nb)              # the on-level may step between runs and inside a run
            keep = rng.integers(0, 3, nb) > 0
            for m in range(1, nb):
                if keep[m]:
                    level[m] = level[m - 1]
            a, b = lo, hi
            if rng.integers(0, 3) == 0:                   # a carrier that fills only part of the measured range, or spills over it
                a, b = lo + int(rng.integers(-2, 3)), hi + int(rng.integers(-2, 3))
            a, b = max(0, a), min(N, max(a + 1, b))
            amp[np.ix_(on, np.arange(a, b))] = level[on][:, None]
        spec = (amp * _phases(rng, (nb, N))).astype(np.complex64)
        strongest = 32.0
    else:
        spec = 1e-3 * (rng.standard_normal((nb, N)) + 1j * rng.standard_normal((nb, N)))
        strongest = 0.0
        for lo, hi in spans:
            on = _runs(rng, nb)
            a = float(rng.uniform(0.05, 1.0))
            strongest = max(strongest, a)
            k = int(on.sum())
            spec[np.ix_(on, np.arange(lo, hi))] += a * (rng.standard_normal((k, hi - lo)) + 1j * rng.standard_normal((k, hi - lo)))
        spec = spec.astype(np.complex64)
    return args, spec, strongest


# ---------------------------------------------------------------------------------------------------------------- the two detection blocks
def _det_case(block, index, klass, rng):
    N = int(rng.choice([256, 1024, 4096]))
    R = int(rng.choice([2, 4, 8]))
    nb = int(rng.integers(10, 25))
    if klass == "exact":
        dec = int(rng.choice([1, 2, 3, 5, 8, 13, 16] if N == 256 else [1, 4, 8, 11, 16, 32, 61]))
        thresh = float(rng.choice(EXACT_DB[2:]))
    else:
        thresh = float(np.float32(rng.uniform(6.0, 15.0)))
        dec = int(rng.choice([32, 40, 64] if thresh < 9.0 else [16, 21, 32, 64])) if N > 256 else int(rng.choice([16, 32] if thresh >= 9.0 else [32]))
    mcd = float(np.float32((2.0 * dec + 0.5) / N)) if dec > 1 else float(np.float32(1.0 / N))   # dec = int(N * mcd / 2)
    assert (int(N * float(mcd) / 2.0) if N * float(mcd) / 2.0 >= 2.0 else 1) == dec
    if block == "vcm":
        nseg = int(rng.integers(1, 4))
        edges = np.sort(rng.uniform(0.03, 0.93, 2 * nseg))
        segs = [(float(np.float32(edges[2 * i])), float(np.float32(edges[2 * i + 1]))) for i in range(nseg)]
        segs = [s for s in segs if (s[1] - s[0]) * N >= 6 * dec] or [(0.125, 0.875)]
        if rng.integers(0, 5) == 0:
            segs[0] = (0.0, segs[0][1])                   # a segment from bin 0
    else:
        a = float(np.float32(rng.uniform(0.03, 0.3)))
        b = float(np.float32(rng.uniform(min(0.9, a + max(0.2, 6.0 * dec / N)), 0.93)))
        segs = [(a, b)] if rng.integers(0, 4) else [(b, a)]                      # SegmentDetection swaps a reversed pair
    args = dict(N=N, R=R, segs=segs, thresh=thresh, maxblocks=int(rng.choice([-1, 0, 1, 3])), delay=int(rng.integers(0, 4)),
                minchandist=mcd, puffer=float(rng.choice([0.0, 0.1, 0.2, 0.5])), ident=index % 7)
    bursts = []
    for s in segs:
        lo_s, hi_s = _geometry_vcm(N, (min(s), max(s)), dec)
        hi_s = min(hi_s, N)
        for _ in range(int(rng.integers(1, 5))):
            # mostly at least two cells wide, so that one cell is filled whatever the grid offset; now and then narrower than a cell
            wmin = 2 * dec if rng.integers(0, 5) else max(1, dec // 2)
            # ... and mostly narrow enough for its extraction (width times 1 + 2 puffer, raised to a power of two) to fit the block
            wmax = min((hi_s - lo_s) // 3, 12 * dec, int(N / (2.0 * (1.0 + 2.0 * args["puffer"]))) if rng.integers(0, 8) else N)
            w = int(rng.integers(min(wmin, max(1, wmax)), max(wmin, wmax) + 1))
            lo = int(rng.integers(lo_s, max(lo_s + 1, hi_s - w)))
            kind = int(rng.integers(0, 16))
            if kind == 0:
                lo = lo_s                                 # touches the lower segment edge
            elif kind == 1:
                lo = hi_s - w                             # touches the upper segment edge
            elif kind == 2:
                lo = lo_s + dec * ((lo - lo_s) // dec)    # sits on the cell grid
                w = dec * max(1, w // dec)
            b0 = int(rng.integers(0, nb - 2))             # may start in block 0
            b1 = int(min(nb - 1, b0 + rng.integers(1, 9)))            # may still be on in the last block ...
            if rng.integers(0, 4):
                b1 = max(b0, min(b1, nb - 3 - args["delay"]))         # ... but mostly ends early enough to be published
            bursts.append((lo, min(N, lo + w), b0, b1))
            if rng.integers(0, 3) == 0:                   # the same carrier again, one or two blocks after it closed
                c0 = b1 + int(rng.integers(2, 4))
                if c0 < nb:
                    bursts.append((lo, min(N, lo + w), c0, int(min(nb - 1, c0 + rng.integers(1, 5)))))
            if rng.integers(0, 3) == 0:                   # a stronger carrier inside or across it: more candidates than survive
                w2 = max(1, w // 2)
                lo2 = lo + int(rng.integers(-w2, w))
                lo2 = max(lo_s, min(hi_s - 1, lo2))
                bursts.append((lo2, min(N, lo2 + w2), b0, b1))
    if klass == "exact":
        amp = np.ones((nb, N))
        for lo, hi, b0, b1 in bursts:
            # mostly an amplitude whose power clears the threshold over the floor by 3 dB or more; one in five: any, also too weak ones
            strong = [v for v in AMPS[1:] if v * v >= 2.0 * 10.0 ** (thresh / 10.0)]
            amp[b0:b1 + 1, lo:hi] = float(rng.choice(strong if rng.integers(0, 5) else AMPS[1:]))
        spec = (amp * _phases(rng, (nb, N))).astype(np.complex64)
        strongest = 32.0
    else:
        spec = 1e-3 * (rng.standard_normal((nb, N)) + 1j * rng.standard_normal((nb, N)))
        strongest = 0.0
        for lo, hi, b0, b1 in bursts:
            a = float(rng.uniform(0.05, 1.0))
            strongest = max(strongest, a)
            spec[b0:b1 + 1, lo:hi] += a * (rng.standard_normal((b1 - b0 + 1, hi - lo)) + 1j * rng.standard_normal((b1 - b0 + 1, hi - lo)))
        spec = spec.astype(np.complex64)
    return args, spec, strongest


def make_case(block, index):
    """dict(block, index, klass, seed, args, spec (nb, N) complex64, per_call, strongest)"""
    klass, seed = klass_of(index), _seed(block, index)
    rng = np.random.default_rng(seed)
    args, spec, strongest = _pac_case(index, klass, rng) if block == "pac" else _det_case(block, index, klass, rng)
    per_call = int(rng.choice([0, 1, 2, 7]))              # items per work() call of the reference block (0: all in one)
    return dict(block=block, index=index, klass=klass, seed=seed, args=args, spec=spec, per_call=per_call, strongest=strongest)


def perturbed(case):
    """the case's input plus independent Gaussian noise 100 dB under its strongest burst (1e-5 of it: the payload tolerance)"""
    rng = np.random.default_rng(case["seed"] + 500000007)
    s = case["spec"]
    return (s + 1e-5 * case["strongest"] * (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape))).astype(np.complex64)


def margin(case):
    """exact class: the smallest relative distance of any decision quotient of the case from its threshold (or its inverse),
    computed in float64 from the integer powers.  PowerActivationChannel: successive block powers of each measured range;
    detection: neighbouring power cells of every cell grid offset the segments can have (all `dec` of them: no geometry needed)."""
    a, p = case["args"], np.abs(case["spec"].astype(np.complex128)) ** 2
    p = np.rint(p)
    thr = 10.0 ** (a["thresh"] / 10.0)
    worst = np.inf

    def near(q):
        q = q[np.isfinite(q) & (q > 0)]
        if q.size == 0:
            return np.inf
        return min(np.abs(q / thr - 1.0).min(), np.abs(q * thr - 1.0).min())
    if case["block"] == "pac":
        for cf, bw, _ in a["chans"]:
            cf32, bw32 = np.float32(cf), np.float32(bw)
            lo, hi = int(round(float(cf32 - bw32 / np.float32(2)) * a["N"])), int(round(float(cf32 + bw32 / np.float32(2)) * a["N"]))
            for d0, d1 in ((0, 0), (-1, 0), (0, 1), (1, 0), (0, -1)):            # the range as given and one bin either way
                s = p[:, max(0, lo + d0):max(0, hi + d1)].sum(axis=1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst = min(worst, near(s[1:] / s[:-1]), near(s[:-1] / s[1:]))
    else:
        dec = int(a["N"] * float(np.float32(a["minchandist"])) / 2.0) if a["N"] * float(np.float32(a["minchandist"])) / 2.0 >= 2.0 else 1
        for off in range(dec):
            n = (a["N"] - off) // dec
            cells = p[:, off:off + n * dec].reshape(p.shape[0], n, dec).sum(axis=2)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = min(worst, near(cells[:, 1:] / cells[:, :-1]))
    return worst


# ---------------------------------------------------------------------------------------------------------------- running a case
def run_blocks(case, make_pac, make_vcm, make_sd, **work_kw):
    """The case through the classes of oracle/oracle.py (oracle: PowerActivationChannel, ActivityDetectionVcm, SegmentDetection;
    reference: the Ref* ones).  Returns the PDU dicts; PowerActivationChannel banks channel after channel (sorted by source)."""
    a, spec = case["args"], case.get("input", case["spec"])
    if case["block"] == "pac":
        out = []
        for cf, bw, ident in a["chans"]:
            out += make_pac(a["N"], cf, bw, a["R"], a["thresh"], a["maxblocks"], a["delay"], ident).work(spec, **work_kw)
        return out
    if case["block"] == "vcm":
        return make_vcm(a["N"], [list(s) for s in a["segs"]], a["thresh"], a["R"], a["maxblocks"], a["minchandist"], a["delay"],
                        a["puffer"]).work(spec, **work_kw)
    s = a["segs"][0]
    return make_sd(a["ident"], a["N"], a["R"], s[0], s[1], a["thresh"], a["minchandist"], a["puffer"], a["maxblocks"],
                   a["delay"]).work(spec, **work_kw)


META = ("kind", "source", "chan_id", "finalized", "has_part", "part", "blockstart", "blockend", "vectorstart", "vectorend")


def meta_of(pdus, vec=True):
    """what is compared EXACTLY: ID suffix (source, channel number, .fin / .part of the PowerActivationChannel follow from
    `finalized`), finalized, part and its absence, block and vector range, sample count — in publication order"""
    keys = META if vec else META[:-2]
    return [tuple(int(d[k]) if not (k == "part" and not d["has_part"]) else -1 for k in keys) + (int(d["samples"].size),) for d in pdus]


# ---------------------------------------------------------------------------------------------------------------- BASELINE-shaped cases
def baseline_case(block):
    """One case each in the shape of BASELINE.json configs[2] (N = 65536, 256 PowerActivationChannels) and configs[4] (N = 65536,
    activity_detection_channelizer_vcm over two wide segments), at a block count that keeps the input small; noisy class."""
    N, R, nb = 65536, 2, 8
    seed = 900001 + BLOCKS.index(block)
    rng = np.random.default_rng(seed)
    spec = 1e-3 * (rng.standard_normal((nb, N)) + 1j * rng.standard_normal((nb, N)))
    if block == "pac":
        chans = [(float(np.float32((c + 0.5) / 256.0)), float(np.float32(1.0 / 512.0)), c) for c in range(256)]
        args = dict(N=N, R=R, chans=chans, thresh=6.0, maxblocks=3, delay=0)
        for cf, bw, _ in chans:
            lo, hi = int(round((cf - bw / 2) * N)), int(round((cf + bw / 2) * N))
            b0 = int(rng.integers(0, nb - 1))
            b1 = int(min(nb - 1, b0 + rng.integers(0, 5)))
            spec[b0:b1 + 1, lo:hi] += 0.5 * (rng.standard_normal((b1 - b0 + 1, hi - lo)) + 1j * rng.standard_normal((b1 - b0 + 1, hi - lo)))
    else:
        args = dict(N=N, R=R, segs=[(0.05, 0.45), (0.55, 0.95)], thresh=10.0, maxblocks=3, delay=1, minchandist=0.005, puffer=0.2, ident=0)
        pos = 0.07
        while pos < 0.92:
            w = float(rng.uniform(0.004, 0.03))
            if not (0.43 < pos + w and pos < 0.57):
                lo, hi = int(pos * N), int((pos + w) * N)
                b0 = int(rng.integers(0, nb - 1))
                b1 = int(min(nb - 1, b0 + rng.integers(1, 6)))
                spec[b0:b1 + 1, lo:hi] += 0.5 * (rng.standard_normal((b1 - b0 + 1, hi - lo)) + 1j * rng.standard_normal((b1 - b0 + 1, hi - lo)))
            pos += w + float(rng.uniform(0.02, 0.05))
    return dict(block=block, index=-1, klass="noisy", seed=seed, args=args, spec=spec.astype(np.complex64), per_call=0, strongest=0.5)


def spectrum_of(x, N, R):
    """The normalised spectrum items the hier block feeds its sinks: overlap-save blocks of N samples (N/R from the block before,
    zeros in front of the first), forward DFT, halves swapped, times 1/N — with numpy.fft in double, rounded to float32 once."""
    ovl = N // R
    H = N - ovl
    xp = np.concatenate([np.zeros(ovl, np.complex128), np.asarray(x, dtype=np.complex128)])
    nb = x.size // H
    blocks = np.stack([xp[m * H:m * H + N] for m in range(nb)])
    return (np.fft.fftshift(np.fft.fft(blocks, axis=1), axes=1) / N).astype(np.complex64)


def samples_case(block, k):
    """Cases that start from TIME SAMPLES (the hier block's path: forward transform on the device, sinks fed from the spectrum in
    HBM): a white floor and keyed QPSK carriers.  case["samples"] is what the device gets, case["spec"] = spectrum_of(samples)
    what the reference blocks get; noisy class (the device's float32 transform is not numpy's), strongest = the largest bin."""
    N, R, nb = 4096, (2, 4)[k % 2], 26
    H = N - N // R
    seed = 700001 + 10 * BLOCKS.index(block) + k
    rng = np.random.default_rng(seed)
    n = np.arange(nb * H)
    x = 0.01 * (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H))
    carriers = [(-0.2, [(3, 9), (11, 12), (17, 22)]), (0.31, [(0, 5), (8, 15), (20, nb - 1)])]       # (frequency, keyed-on block ranges)
    for fc, spans in carriers:
        env = np.zeros(nb * H)
        for t0, t1 in spans:
            env[t0 * H:t1 * H] = 1.0
        sym = (rng.integers(0, 2, nb * H // 64 + 1) * 2 - 1) + 1j * (rng.integers(0, 2, nb * H // 64 + 1) * 2 - 1)
        x += env * np.repeat(sym, 64)[:nb * H] * np.exp(2j * np.pi * fc * n)
    x = x.astype(np.complex64)
    thresh, mb, delay = (6.0, 10.0)[k % 2], (3, -1)[k % 2], (1, 2)[k % 2]
    if block == "pac":
        args = dict(N=N, R=R, chans=[(0.3, 0.04, 5), (0.81, 0.05, 6)], thresh=thresh, maxblocks=mb, delay=0)
    elif block == "vcm":
        args = dict(N=N, R=R, segs=[(0.2, 0.4), (0.7, 0.92)], thresh=10.0, maxblocks=mb, delay=delay, minchandist=0.02, puffer=0.2, ident=0)
    else:
        args = dict(N=N, R=R, segs=[(0.7, 0.92)], thresh=10.0, maxblocks=mb, delay=delay, minchandist=0.02, puffer=0.2, ident=3)
    spec = spectrum_of(x, N, R)
    return dict(block=block, index=-2 - k, klass="noisy", seed=seed, args=args, spec=spec, samples=x, per_call=0,
                strongest=float(np.abs(spec).max()), cuts=[5, 8, 1, 7, nb - 21])


def regenerate(rec):
    """the case of a recording's entry (dict with block and index)"""
    if rec["index"] <= -2:
        return samples_case(rec["block"], -2 - rec["index"])
    return baseline_case(rec["block"]) if rec["index"] == -1 else make_case(rec["block"], rec["index"])


def device_engine_expected(args, geometry):
    """Whether a bank WITHOUT host_decisions runs its decisions on the device: a bank with a detection segment of more than 1024
    power cells (or more than 512 possible simultaneous carriers: cells / 2 + 1) takes the host engine (include/fdc_amd.h).
    geometry: the segment_params() of the bank's segments."""
    return all(g["npower"] <= 1024 and g["npower"] // 2 + 1 <= 512 for g in geometry)


def recorded_cases():
    """(name, case) of everything tests/golden/make_sink_ref_runs.py records: the first RECORDED fuzz indices of every block
    (noisy ones only where the recorder finds them stable) and the BASELINE-shaped cases."""
    for block in BLOCKS:
        for index in range(RECORDED):
            yield "%s_%03d" % (block, index), make_case(block, index)
    yield "pac_baseline", baseline_case("pac")
    yield "vcm_baseline", baseline_case("vcm")
    for block in BLOCKS:
        for k in range(2):
            yield "%s_samples%d" % (block, k), samples_case(block, k)


# what a recording keeps of a payload: everything up to SMALL samples, else length, float64 L2 norm and EXCERPT strided samples
SMALL, EXCERPT = 64, 64


def excerpt_index(n):
    return (np.arange(EXCERPT, dtype=np.int64) * n) // EXCERPT
