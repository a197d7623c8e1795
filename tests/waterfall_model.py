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
    """pixels whose value lies within rel (relative) of an edge: their index may differ by one between two correct roundings"""
    v = np.asarray(values, np.float64)
    j = np.clip(np.searchsorted(e, v), 1, len(e) - 1)
    d = np.minimum(np.abs(v - e[j - 1]), np.abs(v - e[j]))
    return d <= rel * np.maximum(np.abs(v), 1e-300)


def power_stream(nitems, N, seed, level=1e-3):
    """noise plus tones: powers spread over the example's -45 ... -20 dB colour range"""
    rng = np.random.default_rng(seed)
    x = level * (rng.standard_normal((nitems, N)) + 1j * rng.standard_normal((nitems, N)))
    for f in rng.integers(0, N, 4):
        x[:, f] += 0.05 * np.exp(2j * np.pi * rng.random(nitems))
    return (np.abs(x) ** 2).astype(np.float32)
