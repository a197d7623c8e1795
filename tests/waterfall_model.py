"""numpy restatement of FDC.WaterfallMsgTagging's arithmetic (python/WaterfallMsgTagging.py), written from the algorithm, shared by the
waterfall tests.  Everything in float64; the colour index is counted against the float32 row value the library hands out, as the reference
digitizes its float32 means."""
import numpy as np

W = 1024


def block_rows(power):
    """work() :250-254: [nitems, N] powers -> [nitems, 1024]: the mean of N/1024 consecutive bins (reshape(n, 1024, N/1024).mean(2)) or
    each bin repeated 1024/N times (kron)"""
    p = np.asarray(power, np.float64)
    n, N = p.shape
    if N >= W:
        return p.reshape(n, W, N // W).mean(2)
    return np.kron(p, np.ones(W // N))


def decimate(rows, D):
    """pxupdate :154-163: the mean of D consecutive rows, groups aligned to the first block; the rest stays in puffer_blocks"""
    k = rows.shape[0] // D
    return rows[:k * D].reshape(k, D, W).mean(1)


def model_edges(loginput, minvaldb, maxvaldb):
    """cr_colorscheme :284-287, from the levels as Python floats (float64), as the reference takes them"""
    b = np.linspace(float(minvaldb), float(maxvaldb), W - 1)
    return b if loginput else 10.0 ** (b / 10.0)


def colour_index(values, e):
    """apply_colorscheme :262: digitize(x, bins, right=False)"""
    return np.digitize(np.asarray(values, np.float64), e, False)


def near_edge(values, e, rel=1e-5):
    """pixels whose value lies within rel (relative) of an edge: their index may differ by one between two correct roundings.  e: monotonic
    either way, as digitize takes it (non-decreasing, equal edges included, or decreasing); a NaN pixel is near nothing"""
    v = np.asarray(values, np.float64)
    a = np.asarray(e, np.float64)
    if a[0] > a[-1]:
        a = a[::-1]                                                        # the distance to the nearest edge does not depend on the order
    j = np.clip(np.searchsorted(a, v), 1, len(a) - 1)
    with np.errstate(invalid="ignore"):
        d = np.minimum(np.abs(v - a[j - 1]), np.abs(v - a[j]))
        return d <= rel * np.maximum(np.abs(v), 1e-300)


def row_bound(n):
    """Relative bound of a float32 sum of n bin powers re^2 + im^2 against the exact sum of the same float32 bins: every term is >= 0, so the
    relative errors do not amplify; per bin two products and one add (3 roundings), n - 1 adds of the running sum, and the rounding of the
    result the library hands out as float32 (1) — (3 + n - 1 + 1) 2^-24 = (n + 3) 2^-24 to first order.  Where the device sums in FP64 and
    rounds once, the bound holds all the more.  n = 13 gives 9.5e-7: the suite's 1e-6."""
    return (n + 3) * 2.0 ** -24


def noise_stream(n, seed):
    """the parity tests' input: complex64 white noise of unit variance per component"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def stream_rows(x, N, R):
    """float64 model of the block rows of a pipeline call on a fresh stream: overlap-save blocks (N/R samples of history, zero at the start),
    the forward transform times 1/N, fftshift, |.|^2, block_rows"""
    ovl = N // R
    H = N - ovl
    s = np.concatenate([np.zeros(ovl, np.complex128), np.asarray(x, np.complex128)])
    nb = len(x) // H
    blocks = np.stack([s[m * H:m * H + N] for m in range(nb)])
    spec = np.fft.fftshift(np.fft.fft(blocks, axis=1), axes=1) / N
    return block_rows(np.abs(spec) ** 2)


def noise_levels(N):
    """colour levels (dB) around the mean bin power 2 / N of noise_stream's spectrum, 25 dB apart as the example flowgraph's -45 ... -20"""
    c = 10.0 * np.log10(2.0 / N)
    return (float(np.round(c - 12.5, 1)), float(np.round(c + 12.5, 1)))


def near_share(rows, e, rel=1e-5):
    """the share of pixels the index comparison with the model leaves out"""
    return float(near_edge(rows, e, rel).mean())


# the pipeline cases of tests/test_waterfall_routes_gpu.py: (N, R, blocks of the stream, D, seed of noise_stream); the CPU suite checks that the
# model's pixels of each stay under the cap of pixels near an edge (test_waterfall_cpu.py)
NEAR_CAP = 0.01


def route_seed(N, R, nb):
    return N // 64 + 131 * R + nb + 1


def route_streams():
    """(N, R, blocks, D, seed, times the samples are fed): the stream is noise_stream(blocks (N - N / R), seed), fed once or twice"""
    cases = [(4096, R, 6, D, 1) for R in (2, 4, 8, 16) for D in (1, 2)]                        # every ROWS form
    cases += [(4096, R, 7, 3, 1) for R in (2, 4)]                                              # launch groups and sub-batches
    cases += [(N, R, nb, 2, 2) for N in (16384, 32768) for nb in (3, 9) for R in (2, 4)]       # group sums (odd counts: a second call)
    cases += [(65536, 2, nb, 2, 2) for nb in (3, 9)] + [(262144, 2, 2, 2, 1)]
    cases += [(N, 2, 10, 2, 1) for N in (64, 256, 512, 1024, 2048, 4096)]                      # spectrum route
    return [(N, R, nb, D, route_seed(N, R, nb), reps) for (N, R, nb, D, reps) in cases]


def power_stream(nitems, N, seed, level=1e-3):
    """noise plus tones: powers spread over the example's -45 ... -20 dB colour range"""
    rng = np.random.default_rng(seed)
    x = level * (rng.standard_normal((nitems, N)) + 1j * rng.standard_normal((nitems, N)))
    for f in rng.integers(0, N, 4):
        x[:, f] += 0.05 * np.exp(2j * np.pi * rng.random(nitems))
    return (np.abs(x) ** 2).astype(np.float32)
