"""Cases for the executed reference hier block (oracle/ref_hier.py), shared by the recorder (tests/golden/make_hier_ref_runs.py),
the CPU test (tests/test_hier_reference_cpu.py) and the GPU test (tests/test_hier_reference_gpu.py).  Nothing here reads the reference,
the oracle or the product: a case is the FULL argument list of the hier block's constructor (python/FrequencyDomainChannelizer.py:46-60,
in its order) plus a seeded input.

Inputs are int16 I/Q pairs with the power-of-two scale SCALE: (I + jQ) * SCALE is exact in float32, so the same integers serve the
complex64 entry and the iq_input="sc16" entry.  Every case has nblocks >= 2 relinvovl + 1 items, so that every window phase occurs
twice.  Several cases share one input (cases of one geometry name the same `input` key): an N = 65536 input is 0.6 MB.

Families:
  a  the example flowgraph's parameters (examples/FDC_example.grc: N = 4096, R = 4, its four channels), window types 0 / 1 / 2, debug
     off / on (the port shift)
  b  N = 4096 and 1024, R = 2 / 4 / 8, mixed widths; user frequencies that put the slice on an ODD first bin; the wrap below zero and the
     clamp at the upper band edge (:338-341); passband < 0.7 (stop band = pass band + 0.25).  "Pass band clamped to 1" (:331-332) cannot
     be reached through the derivation: l >= occupied bins, and whenever occupied / l > 1 / 1.2 the slice is doubled (:326-327), so the
     pass band is at most 1.1 / 1.2; the block-level phase-window cases below use passbw = 1.0 instead.
  c  banks that reach each block kernel through the derivation (256-, 512-, 1024-, 128- and 64-bin channels; N = 65536, 32768, 16384;
     R = 2 and 4; bw = 0.8 / C, bw = 1 / C (doubled, half-overlapping slices) and banks centred on multiples of l), with the kernel path
     and the words of describe() that the parity tests of the same plans assert
  d  one mixed plan at N = 65536 (spectrum path) and one split plan (a tiling of 256-bin channels plus three others)
  e  basebandfs and centerfreqfs, the mode given as integer and as string
  f  inpveclen = blocksize: the input is spectrum items and goes straight into normalize_input; with and without debug
  g  the sink blocks as the hier block wires them at N = 4096: activity-controlled channels plus detection segments, msgoutput on, negative
     *_deactivation_delay and negative minchanflankpuffer (the clamps at :246, :271, :273); input: time samples with keyed carriers
     60 dB over the floor (the levels of sink_ref_cases.samples_case); kept only while the reference decides the same under noise
     100 dB below the carriers (sink_ref_cases' stability criterion; asserted by the recorder and the CPU test)
  h  constructions the reference refuses (REFUSED) and constructions only the product refuses (DIVERGENCES)
"""
import numpy as np

GEN_VERSION = 1
SCALE_LOG2 = -11
SCALE = 2.0 ** SCALE_LOG2
EXAMPLE = [[0.12, 0.05], [0.22, 0.1], [-0.14, 0.12], [0, 0.081]]          # examples/FDC_example.grc, variable `channels`


def args(blocksize, relinvovl, throughput, windowtype=1, debug=False, inptype=8, inpveclen=1, act_channels=None, act_thresh=6.0, fs=1.0,
         centerfrequency=0.0, freqmode=0, msgoutput=False, segments=None, det_thresh=10.0, minchandist=0.005, det_delay=1, puffer=0.2,
         pow_delay=1, pow_maxblocks=128, det_maxblocks=128, threaded=False):
    """the hier block's 25 constructor arguments, in the reference's order"""
    return [inptype, inpveclen, blocksize, relinvovl, throughput, act_channels, act_thresh, fs, centerfrequency, freqmode, windowtype,
            msgoutput, False, "", threaded, segments, det_thresh, minchandist, det_delay, puffer, 0, pow_delay, pow_maxblocks, det_maxblocks,
            debug]


def _case(name, a, inp, nb, path=None, words=(), store="all", max_blocks=None):
    N, R = 1 << int(np.ceil(np.log2(a[2]))), 1 << int(np.ceil(np.log2(a[3])))
    assert nb >= 2 * R + 1, name
    return dict(name=name, family=name[0], args=a, input=inp, N=N, R=R, nblocks=nb, path=path, words=list(words), store=store,
                max_blocks=max_blocks or nb)


def cases():
    out = []
    # ---- a
    for wt in (0, 1, 2):
        for debug in (False, True):
            out.append(_case("a_example_w%d_%s" % (wt, "debug" if debug else "plain"), args(2 ** 12, 4, EXAMPLE, wt, debug), "noise_4096_4", 9,
                             path=5 if not debug else None))
    # ---- b
    odd = lambda N, k: k / N - 0.5                                               # internal centre bin k (odd k and l/2 even: odd first bin)
    b4096 = [[odd(4096, 1001), 0.05], [odd(4096, 2047), 0.1], [odd(4096, 3), 0.03], [odd(4096, 4093), 0.03], [odd(4096, 3001), 0.12],
             [odd(4096, 777), 0.004], [0.25, 0.3]]
    b1024 = [[odd(1024, 301), 0.05], [odd(1024, 1), 0.1], [odd(1024, 1021), 0.06], [odd(1024, 555), 0.12], [-0.125, 0.02]]
    for N, lst, R, wt, nb in ((4096, b4096, 2, 1, 5), (4096, b4096, 8, 2, 17), (1024, b1024, 2, 0, 6), (1024, b1024, 4, 1, 10), (1024, b1024, 8, 1, 19)):
        out.append(_case("b_mixed_%d_R%d" % (N, R), args(N, R, lst, wt, debug=(N == 1024 and R == 8)), "noise_%d_%d" % (N, R), nb))
    # ---- c
    bank = lambda C, bw, off=0.0, lo=0: [[(k + off) / C - 0.5, bw / C] for k in range(lo, C)]
    few = "bank"
    out += [
        _case("c_256bin_65536_R2", args(65536, 2, bank(256, 0.8, 0.5)), "noise_65536_2", 5, 3, ["k_blk256, 1 tiling (r = 0)"], few),
        _case("c_128bin_centred_65536_R2", args(65536, 2, bank(512, 0.8, 0.0, 1), freqmode="normalized"), "noise_65536_2", 5, 3,
              ["k_blknar, l = 128, bank of 511 half a channel off the grid"], few),
        _case("c_512bin_doubled_65536_R2", args(65536, 2, bank(256, 1.0)), "noise_65536_2", 5, 3, ["k_blk512", "two launches", "1 copies"], few),
        _case("c_1024bin_65536_R2", args(65536, 2, bank(64, 0.8, 0.5)), "noise_65536_2", 5, 3, ["k_blk1024"], few),
        _case("c_64bin_65536_R2", args(65536, 2, bank(1024, 0.8, 0.5)), "noise_65536_2", 5, 3, ["k_blknar, l = 64, bank of 1024 on the grid"], few),
        _case("c_256bin_centred_32768_R2", args(32768, 2, bank(128, 0.8)), "noise_32768_2", 5, 3, ["k_blk256, 2 tilings"], few),
        _case("c_256bin_centred_16384_R4", args(16384, 4, bank(64, 0.8), windowtype=0), "noise_16384_4", 9, 3, ["k_blk256, 2 tilings"], few),
        _case("c_512bin_16384_R2", args(16384, 2, bank(32, 0.8, 0.5), windowtype=2), "noise_16384_2", 5, 3, ["k_blk512, l = 512, bank of 32 on the grid"], few),
    ]
    # ---- d
    out += [
        _case("d_mixed_65536_R2", args(65536, 2, bank(256, 0.8, 0.5)[::3] + [[0.1, 0.01], [-0.3, 0.05]]), "noise_65536_2", 5, 1, [], few),
        _case("d_split_65536_R2", args(65536, 2, bank(256, 0.8, 0.5) + [[0.1003, 0.01], [-0.3, 0.05], [0.2, 0.002]]), "noise_65536_2", 5, 4,
              ["k_blk256, 1 tiling (r = 0) + 3 other channels"], few),
    ]
    # ---- e
    fs, cf = 2.4e6, 433.92e6
    for mode in (1, "basebandfs"):
        out.append(_case("e_basebandfs_%s" % ("int" if mode == 1 else "str"),
                         args(4096, 4, [[u * fs, bw * fs] for u, bw in EXAMPLE], fs=fs, freqmode=mode), "noise_4096_4", 9))
    for mode in (2, "centerfreqfs"):
        out.append(_case("e_centerfreqfs_%s" % ("int" if mode == 2 else "str"),
                         args(4096, 4, [[u * fs + cf, bw * fs] for u, bw in EXAMPLE], fs=fs, centerfrequency=cf, freqmode=mode, debug=(mode == 2)),
                         "noise_4096_4", 9))
    # ---- f
    for debug in (False, True):
        out.append(_case("f_spectrum_items_%s" % ("debug" if debug else "plain"), args(1024, 4, b1024, 1, debug, inpveclen=1024), "items_1024", 9))
    # ---- g
    seg = [[0.2, 0.42]]                                   # user frequencies: internal 0.7 .. 0.92, around the carrier at +0.31
    act = [[-0.2, 0.04], [0.31, 0.05]]                    # on the two carriers
    out.append(_case("g_sinks_R4", args(4096, 4, EXAMPLE[:2], 1, False, act_channels=act, act_thresh=6.0, msgoutput=True, segments=seg, det_thresh=10.0,
                                        minchandist=0.02, det_delay=-3, puffer=-1.0, pow_delay=-2, pow_maxblocks=3, det_maxblocks=3), "bursts_4096_4", 26))
    out.append(_case("g_sinks_R2", args(4096, 2, EXAMPLE[2:], 1, False, act_channels=act, act_thresh=10.0, msgoutput=True, segments=seg, det_thresh=10.0,
                                        minchandist=0.02, det_delay=2, puffer=0.2, pow_delay=0, pow_maxblocks=-1, det_maxblocks=-1), "bursts_4096_2", 26))
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_input(key):
    """int16 array of shape (n, 2): I and Q in counts of SCALE"""
    kind, *dims = key.split("_")
    if kind == "noise":                                   # white Gaussian noise, sigma 300 counts, clipped to 12 bits
        N, R = int(dims[0]), int(dims[1])
        nb = {(1024, 2): 6, (1024, 4): 10, (1024, 8): 19}.get((N, R), 2 * R + 1)
        rng = np.random.default_rng(77000 + N + R)
        return np.clip(np.rint(300.0 * rng.standard_normal((nb * (N - N // R), 2))), -2047, 2047).astype(np.int16)
    if kind == "items":                                   # spectrum items (inpveclen = blocksize): any complex numbers will do
        N = int(dims[0])
        rng = np.random.default_rng(78000 + N)
        return np.clip(np.rint(300.0 * rng.standard_normal((9 * N, 2))), -2047, 2047).astype(np.int16)
    if kind == "bursts":                                  # sink_ref_cases.samples_case: floor 0.01, keyed QPSK carriers of amplitude 1 at -0.2 and +0.31
        # (32 samples per symbol instead of 64: a carrier three power cells wide, which the detection segment sees whatever the cell grid's offset)
        N, R, nb = int(dims[0]), int(dims[1]), 26
        H = N - N // R
        rng = np.random.default_rng(79000 + N + R)
        n = np.arange(nb * H)
        x = 0.01 * (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H))
        for fc, spans in [(-0.2, [(3, 9), (11, 12), (17, 22)]), (0.31, [(0, 5), (8, 15), (20, nb - 1)])]:
            env = np.zeros(nb * H)
            for t0, t1 in spans:
                env[t0 * H:t1 * H] = 1.0
            sym = (rng.integers(0, 2, nb * H // 32 + 1) * 2 - 1) + 1j * (rng.integers(0, 2, nb * H // 32 + 1) * 2 - 1)
            x += env * np.repeat(sym, 32)[:nb * H] * np.exp(2j * np.pi * fc * n)
        q = np.rint(x / SCALE)
        assert np.abs(q.real).max() < 32767 and np.abs(q.imag).max() < 32767
        return np.stack([q.real, q.imag], axis=1).astype(np.int16)
    raise KeyError(key)


def as_complex(iq):
    """(I + jQ) * SCALE, exact in float32"""
    iq = np.asarray(iq)
    return ((iq[:, 0].astype(np.float32) + 1j * iq[:, 1].astype(np.float32)) * np.float32(SCALE)).astype(np.complex64)


def perturbed(x, seed):
    """the complex input plus independent Gaussian noise 100 dB under the carriers (amplitude 1): sink_ref_cases.perturbed"""
    rng = np.random.default_rng(seed + 500000007)
    return (x + 1e-5 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))).astype(np.complex64)


def stored_ports(case, nports):
    """which output ports a recording keeps: all, or for a bank the debug port (if any), the first and the last channel and a seeded
    choice of 16 others"""
    if case["store"] == "all" or nports <= 18:
        return list(range(nports))
    first = 1 if case["args"][24] else 0
    rng = np.random.default_rng(abs(hash_name(case["name"])))
    pick = rng.choice(np.arange(first + 1, nports - 1), 16, replace=False)
    return sorted(set(range(first + 1)) | {nports - 1} | {int(p) for p in pick})


def hash_name(name):
    import zlib
    return zlib.crc32(name.encode())


def ragged(nb):
    """work() calls of the GPU test in items: 1, several, 0, the rest"""
    several = min(3, nb - 2)
    return [1, several, 0, nb - 1 - several]


# ---------------------------------------------------------------------------------------------------------------- h: refusals
def refused():
    """(name, args): constructions the reference refuses; the recorder notes the exception type, the product must raise ValueError"""
    return [
        ("h_channels_not_a_list", args(4096, 4, "0.1,0.05")),
        ("h_channel_not_a_pair", args(4096, 4, [[0.1, 0.05, 3]])),
        ("h_channel_a_number", args(4096, 4, [0.1])),
        ("h_act_channels_not_a_list", args(4096, 4, EXAMPLE, act_channels=3)),
        ("h_act_channel_not_a_pair", args(4096, 4, EXAMPLE, act_channels=[[0.1]])),
        ("h_segments_not_a_list", args(4096, 4, EXAMPLE, segments=0.5)),
        ("h_segment_not_a_pair", args(4096, 4, EXAMPLE, segments=[[0.1, 0.2], 0.3])),
        ("h_unknown_freqmode_int", args(4096, 4, EXAMPLE, freqmode=3)),
        ("h_unknown_freqmode_str", args(4096, 4, EXAMPLE, freqmode="baseband")),
        ("h_bw_one", args(4096, 4, [[0.1, 1.0]])),                      # bw % 1.0 == 0 -> nextpow2(0) raises (:324)
        ("h_bw_zero", args(4096, 4, [[0.1, 0.0]])),
        ("h_blocksize_zero", args(0, 4, EXAMPLE)),
        ("h_relinvovl_zero", args(4096, 0, EXAMPLE)),
        ("h_unknown_input_type", args(4096, 4, EXAMPLE, inptype=2)),    # :209-210
    ]


def divergences():
    """(name, args, what the reference does, the line of gr-fdc_amd/channelizer.py that explains the product): constructions the reference
    accepts and the product refuses with ValueError, or the other way round.  One by one; there is no open-ended "except where different"."""
    return [
        # the reference: itemsize 4 with inpveclen 1 raises ValueError('Unknown input type. ') (:205-210: the second branch repeats the first
        # condition, fft_vfc is unreachable).  The product serves the Float input type of the GRC block by the fft_vfc front end that was meant.
        ("h_float_input", args(4096, 4, EXAMPLE, inptype=4), "raises ValueError", "accepts", "if self.itemsize not in (8, 4):"),
        # the reference: any inpveclen != 1 is wired straight into normalize_input, whose item is blocksize long: GNU Radio would refuse the
        # connection at start for another length (item size mismatch); the construction itself succeeds.  The product refuses at construction.
        ("h_inpveclen_other", args(4096, 4, EXAMPLE, inpveclen=7), "accepts (the flowgraph would fail at start)", "raises ValueError",
         "if self.inpveclen != 1 and self.inpveclen != self.blocksize:"),
    ]


# ---------------------------------------------------------------------------------------------------------------- block-level cases
def block_cases():
    """Seeded differential cases for the three chain blocks on their own: dicts with block, ctor (constructor arguments), input (numpy
    array) and calls (items per work() call; state crosses the calls)."""
    rng = np.random.default_rng(20261016)
    out = []

    def calls_for(n, k):
        if k % 3 == 0:
            return [1] * n                                # one-item calls
        if k % 3 == 1:
            return [n]
        cuts, left = [], n
        while left:
            c = int(min(left, rng.integers(1, 5)))
            cuts.append(c)
            left -= c
        return cuts
    dt = {1: np.uint8, 2: np.uint16, 4: np.float32, 8: np.complex64}
    k = 0
    for isz in (1, 2, 4, 8):
        for outlen, ovl in ((2, 1), (7, 1), (7, 3), (64, 32), (100, 37), (256, 64), (4096, 1024), (4096, 2048), (128, 16)):
            if outlen == 4096 and isz != 8:               # the hier block's own geometry: complex items only (file size)
                continue
            n = int(rng.integers(3, 12)) if outlen < 4096 else 3
            raw = rng.integers(0, 256, n * isz * (outlen - ovl), dtype=np.uint8)
            if isz >= 4:                                  # finite floats, so that array comparisons mean what they say
                raw = rng.standard_normal(n * (outlen - ovl) * isz // 4).astype(np.float32).view(np.uint8)
            out.append(dict(block="overlap_save", ctor=(isz, outlen, ovl), input=raw.view(dt[isz]), calls=calls_for(n, k)))
            k += 1
        for veclen, blk, off in ((8, 8, 0), (8, 3, 0), (8, 3, 5), (4096, 256, 2412), (4096, 256, 3840), (256, 192, 64), (300, 1, 299), (300, 299, 1)):
            if veclen == 4096 and isz != 8:
                continue
            n = int(rng.integers(1, 9)) if veclen < 4096 else 3
            raw = rng.standard_normal(n * veclen * isz // 4 + 1).astype(np.float32).view(np.uint8)[:n * veclen * isz] if isz >= 4 else \
                rng.integers(0, 256, n * isz * veclen, dtype=np.uint8)
            out.append(dict(block="vector_cut_vxx", ctor=(isz, veclen, off, blk), input=np.ascontiguousarray(raw).view(dt[isz]), calls=calls_for(n, k)))
            k += 1
    Rs = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    for i, R in enumerate(Rs):
        for wt in (0, 1, 2):
            l = [2, 7, 33, 64, 16, 101, 128][(i + wt) % 7]
            shifts = int([-1, -R, -R - 1, R, R + 1, 3 * R + 2, -4093, 2412, 0][(i * 3 + wt) % 9])
            pbw = float(np.float32([0.528, 0.88, 1.0, 0.7128, 0.3][(i + 2 * wt) % 5]))
            sbw = 1.0 if pbw >= 0.7 else float(np.float32(pbw + 0.25))
            n = 2 * R + 3
            x = (rng.standard_normal(n * l) + 1j * rng.standard_normal(n * l)).astype(np.complex64)
            out.append(dict(block="phase_shifting_windowing_vcc", ctor=(l, R, shifts, pbw, sbw, wt), input=x, calls=calls_for(n, k)))
            k += 1
    return out


PHASE_WINDOW_REFUSALS = [(64, 4, 1, 0.0, 1.0, 1), (64, 4, 1, 0.5, 0.0, 1), (64, 4, 1, 0.8, 0.5, 1), (64, 4, 1, -0.1, 1.0, 0)]
# the first three are the constructor's three refusals (passbw <= 0, stopbw <= 0, stopbw < passbw); the fourth is the first again, negative
