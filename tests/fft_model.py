"""TEST INFRASTRUCTURE — the yardstick of tests/test_transform_accuracy_gpu.py, in plain numpy, with nothing of the product in it.

  dft64, dft64_forms   the transform of fft_vcc(n, forward, rectangular, shift) in complex128 (numpy.fft): the reference
  fft32_model      a textbook radix-2 transform whose every intermediate is complex64: what a correct float32 transform loses
  fft32_model_steps    the same with the roundings a radix-16 / two-pass transform legitimately takes and a radix-2 one does not (see there)
  channel_stage64  one channel of the channel stage (slice, window row, ifftshift, inverse transform, discard, times l) in complex128
  channel_stage32  the same with complex64 products and one of the float32 models
  chain64, chain32 the whole chain (block, forward transform, shift and 1/N, channel stage) in complex128 / with complex64 intermediates and any
                   pair of the float32 models; stream_blocks, chain_noise_stream, chain_impulse_stream, chain_tone_stream: its inputs, as streams
  noise, impulse_positions, wide_impulse_positions, impulses, tone      the inputs
  model_error, transform_model_error, channel_model_error, ratios       the criterion: error against the reference, held to a multiple of E_model

The criterion (per item or per (block, channel) row):  rms error <= 2 x E_rms and max error <= 3 x E_max, E the model's error on the same input (the
larger of the two models' on that row), each with
a floor of 2**-23 * max|ref| (one float32 ulp at the output's scale: the model is exact for an impulse at n <= 4, for the impulse at sample 0, ...).
The factors come from two independent CPU float32 transforms (this model and scipy.fft's complex64 one, test_fft_model_cpu.py): they agree within
1.2 x in L2 and 1.5 x in per-sample max at every size, in either direction; 2 and 3 leave room for a third factorisation.
"""
import numpy as np

L2_FACTOR, MAX_FACTOR = 2.0, 3.0
ULP = 2.0 ** -23


# ---------------------------------------------------------------- transforms
def dft64(x, inverse=False, shift=False):
    """fft_vcc's transform of every row of x in complex128, unnormalised both ways.  forward + shift: the output halves swapped; inverse + shift:
    the input halves swapped (tests/test_oracle.py::test_fft_vcc_matches_numpy states the same and is the authority)."""
    x = np.asarray(x).astype(np.complex128)
    n = x.shape[-1]
    if inverse:
        if shift:
            x = np.fft.ifftshift(x, axes=-1)
        return np.fft.ifft(x, axis=-1) * n
    y = np.fft.fft(x, axis=-1)
    return np.fft.fftshift(y, axes=-1) if shift else y


def dft64_forms(x):
    """{(inverse, shift): dft64(x, inverse, shift)} from two transforms: forward + shift is the forward result with its halves swapped; inverse + shift
    (the input's halves swapped) is the inverse result times (-1)**k — both exact."""
    x = np.asarray(x)
    n = x.shape[-1]
    fwd, inv = dft64(x), dft64(x, inverse=True)
    sign = 1.0 - 2.0 * (np.arange(n) & 1)
    return {(False, False): fwd, (False, True): np.roll(fwd, n // 2, axis=-1), (True, False): inv, (True, True): inv * sign}


def stage_twiddles(ns, inverse=False):
    """The ns twiddles of the radix-2 stage that joins transforms of length ns: exp(-+2 pi i k / (2 ns)), in float64, rounded once."""
    a = (2.0 if inverse else -2.0) * np.pi * np.arange(ns, dtype=np.float64) / (2.0 * ns)
    return (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)


def fft32_model(x, inverse=False, defect=None):
    """Radix-2 Stockham transform (decimation in time, autosort) of every row of x; every intermediate is complex64, every product and sum is
    numpy's complex64 arithmetic.  Unnormalised, unshifted.  defect = (stage, index, angle): twiddle `index` of stage `stage` (0 = the first, whose only
    twiddle is 1) is rotated by `angle` radians before it is rounded — one wrong table entry, for test_fft_model_cpu.py."""
    x = np.array(x, dtype=np.complex64)
    lead, n = x.shape[:-1], x.shape[-1]
    lg = n.bit_length() - 1
    assert n == 1 << lg and n >= 1
    x = x.reshape(-1, n)
    rows = x.shape[0]
    y = np.empty_like(x)
    t = np.empty((rows, n // 2), dtype=np.complex64)
    for s in range(lg):
        ns = 1 << s
        w = stage_twiddles(ns, inverse)
        if defect is not None and defect[0] == s:
            a = (2.0 if inverse else -2.0) * np.pi * defect[1] / (2.0 * ns) + defect[2]
            w[defect[1]] = np.complex64(np.cos(a) + 1j * np.sin(a))
        # butterfly j = q * ns + k takes x[j] and x[j + n/2] * w[k] to y[q * 2 ns + k] and y[q * 2 ns + ns + k]
        xv = x.reshape(rows, 2, n // (2 * ns), ns)
        yv = y.reshape(rows, n // (2 * ns), 2, ns)
        tv = t.reshape(rows, n // (2 * ns), ns)
        np.multiply(xv[:, 1], w, out=tv)
        np.add(xv[:, 0], tv, out=yv[:, :, 0])
        np.subtract(xv[:, 0], tv, out=yv[:, :, 1])
        x, y = y, x
    return x.reshape(lead + (n,))


# ---- the same yardstick with the rounding steps the kernels legitimately take and a radix-2 transform does not -------------------------------
# Per item an impulse compares PATHS: the impulse at sample 1 meets one rounded twiddle in the radix-2 model (its error is 4.2e-8) and, in a
# radix-16 / two-pass transform, a product of several — a correct one is 1.4e-7 ... 1.8e-7 off there (first device run: 3.4 - 4.3 x the radix-2
# figure), as the radix-2 model itself is for other impulses.  The steps, written from the textbook (Stockham autosort, mixed radix; Bailey's
# four-step form), with every table entry computed in float64 here and rounded once:
#   - a radix-16 pass multiplies input r = 4 a + b of a butterfly by TWO rounded table entries in turn, W^(b k) and W^(4 a k), not by one W^(r k);
#     its 16-point transform is two layers of radix-4 butterflies with the rounded constants W16^(b k1) between them;
#   - what is left of log2 n goes to one radix-4 and / or one radix-2 pass;
#   - above 8192 points the transform is N1 x N2 (N1 = 2**ceil(log2 n / 2)): length-N2 transforms down the columns, one more product with a rounded
#     W_n^(n1 k2), length-N1 transforms along the rows.
# A row's bound is taken from the larger of the two models' errors on it (model_error): the radix-2 yardstick never shrinks, the factors 2 and 3 stay.
def _tw(n, e, inverse):
    a = (2.0 if inverse else -2.0) * np.pi * (np.asarray(e, dtype=np.int64) % n) / n
    return (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)


def _dft4(a0, a1, a2, a3, inverse):
    mi = np.complex64(1j if inverse else -1j)          # (times -+i: exact)
    t0, t1, t2, t3 = a0 + a2, a0 - a2, a1 + a3, (a1 - a3) * mi
    return t0 + t2, t1 + t3, t0 - t2, t1 - t3


def _dft16(v, inverse):
    """X[k1 + 4 k2] of x[4 a + b]: radix 4 over a, times W16^(b k1), radix 4 over b"""
    u = [[None] * 4 for _ in range(4)]
    for b in range(4):
        u[0][b], u[1][b], u[2][b], u[3][b] = _dft4(v[b], v[4 + b], v[8 + b], v[12 + b], inverse)
    out = [None] * 16
    for k1 in range(4):
        for b in range(1, 4):
            if k1:
                u[k1][b] = u[k1][b] * _tw(16, b * k1, inverse)
        out[k1], out[k1 + 4], out[k1 + 8], out[k1 + 12] = _dft4(u[k1][0], u[k1][1], u[k1][2], u[k1][3], inverse)
    return out


def _lds_transform(x, inverse):
    """rows of 2**lg points: radix-16 passes, then one radix-4 and / or one radix-2 pass (Stockham autosort, decimation in time)"""
    rows, n = x.shape
    lg = n.bit_length() - 1
    passes = [4] * (lg // 4) + ([2] if lg % 4 >= 2 else []) + ([1] if lg % 2 else [])
    y = np.empty_like(x)
    ns = 1
    for p in passes:
        R = 1 << p
        Q = n // (R * ns)
        xv = x.reshape(rows, R, Q, ns)
        v = [xv[:, r] for r in range(R)]
        if ns > 1:
            k = np.arange(ns)
            if R == 16:
                for r in range(1, 16):
                    if r & 3:
                        v[r] = v[r] * _tw(R * ns, (r & 3) * k, inverse)
                    if r >> 2:
                        v[r] = v[r] * _tw(R * ns, 4 * (r >> 2) * k, inverse)
            else:
                for r in range(1, R):
                    v[r] = v[r] * _tw(R * ns, r * k, inverse)
        out = _dft16(v, inverse) if R == 16 else _dft4(v[0], v[1], v[2], v[3], inverse) if R == 4 else (v[0] + v[1], v[0] - v[1])
        yv = y.reshape(rows, Q, R, ns)
        for r in range(R):
            yv[:, :, r] = out[r]
        x, y = y, x
        ns *= R
    return x


def fft32_model_steps(x, inverse=False):
    """fft32_model with the steps above: unnormalised, unshifted, every intermediate complex64."""
    x = np.array(x, dtype=np.complex64)
    lead, n = x.shape[:-1], x.shape[-1]
    x = x.reshape(-1, n)
    rows = x.shape[0]
    if n <= 8192:
        return _lds_transform(x, inverse).reshape(lead + (n,))
    lg = n.bit_length() - 1
    N1 = 1 << ((lg + 1) // 2)
    N2 = n // N1
    # sample n1 + N1 n2, bin N2 k1 + k2
    a = _lds_transform(np.ascontiguousarray(x.reshape(rows, N2, N1).transpose(0, 2, 1)).reshape(rows * N1, N2), inverse).reshape(rows, N1, N2)
    a *= _tw(n, np.arange(N1, dtype=np.int64)[:, None] * np.arange(N2, dtype=np.int64)[None, :], inverse)
    b = _lds_transform(np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(rows * N2, N1), inverse).reshape(rows, N2, N1)
    return np.ascontiguousarray(b.transpose(0, 2, 1)).reshape(lead + (n,))


FLOAT32_MODELS = (fft32_model, fft32_model_steps)


# ---------------------------------------------------------------- the channel stage
def window_row_index(m, R, f):
    """phase_shifting_windowing_vcc: the row of the (R, l) window table that block m (counted from the stream's start) is multiplied by."""
    return ((m % R) * (f % R)) % R


def channel_stage64(spec, N, R, chan, window_rows, first_block=0):
    """One channel of the channel stage on the spectrum items `spec` ((nb, N), what the channel kernels read: 1/N applied), in complex128:
    slice [f, f + l), times window row ((first_block + m) mod R * f) mod R, ifftshift, unnormalised inverse transform of length l, the first l // R
    samples discarded, times l (the composition tests/test_oracle.py::test_chain_blockwise_equals_composed_blocks spells out).
    chan = (f, l); window_rows: the (R, l) table of the ORACLE (tests/golden/windows_ref.npz pins it).  Returns (nb, l - l // R).
    f may be an array of C offsets that agree mod R (one window table, one row per block: a uniform bank): one transform call for all of them,
    (nb, C, l - l // R)."""
    return _channel_stage(spec, N, R, chan, window_rows, first_block, np.complex128)


def channel_stage32(spec, N, R, chan, window_rows, first_block=0, transform=None):
    """channel_stage64 as a float32 kernel computes it: the window product in complex64, fft32_model (or another of FLOAT32_MODELS), the scale by l
    (exact)."""
    return _channel_stage(spec, N, R, chan, window_rows, first_block, np.complex64, transform or fft32_model)


def channel_model_error(spec, N, R, chan, window_rows, first_block, ref):
    """E_model of the channel stage per row: the larger of the float32 models' errors (model_error)"""
    es = [model_error(channel_stage32(spec, N, R, chan, window_rows, first_block, t), ref) for t in FLOAT32_MODELS]
    return np.maximum(es[0][0], es[1][0]), np.maximum(es[0][1], es[1][1])


def _channel_stage(spec, N, R, chan, window_rows, first_block, dtype, transform=None):
    f, l = chan
    fs = np.atleast_1d(np.asarray(f, dtype=np.int64))
    assert (fs % R == fs[0] % R).all() and fs.min() >= 0 and fs.max() + l <= N
    spec = np.asarray(spec).reshape(-1, N)
    nb = spec.shape[0]
    win = np.asarray(window_rows).reshape(R, l)
    rows = np.array([window_row_index(first_block + m, R, int(fs[0])) for m in range(nb)])
    y = spec[:, fs[:, None] + np.arange(l)[None, :]].astype(dtype) * win[rows].astype(dtype)[:, None, :]
    y = np.fft.ifftshift(y, axes=-1)
    y = transform(y, inverse=True) if dtype == np.complex64 else dft64(y, inverse=True)
    y = y[..., l // R:] * dtype(l)
    return y[:, 0] if np.ndim(f) == 0 else y


# ---------------------------------------------------------------- the whole chain: block -> forward N -> shift, 1/N -> channel stage
# What the one-launch block kernels (k_blk256 / 512 / 1024, k_blknar, k_f4096) and the two-launch forms compute without a spectrum in memory: the
# yardstick is the same two transforms in a row.  E of a (block, channel) row: the largest error over the FOUR (forward model, inverse model)
# combinations of FLOAT32_MODELS.  There are NO factors for it yet: independent correct float32 chains (scipy.fft on complex64, the oracle's compiled
# float32 chain) are up to 6.1 x (rms) and 8.7 x (per sample) off this E on rows where the models are nearly exact and the other chain is one ulp off
# (profiles/accuracy/README.md, profiles/accuracy/chain_factors.py) — twice that is no float32-grade bound.
CHAIN_COMBINATIONS = tuple((fwd, inv) for fwd in FLOAT32_MODELS for inv in FLOAT32_MODELS)


def stream_blocks(stream, N, R):
    """The blocks overlap-save cuts from a stream with N/R zeros in front of it: block m = samples [m H - N/R, m H + H), H = N - N/R.  (nb, N)."""
    ovl = N // R
    H = N - ovl
    s = np.asarray(stream)
    nb = s.size // H
    ring = np.concatenate([np.zeros(ovl, dtype=s.dtype), s[:nb * H]])
    return ring[H * np.arange(nb)[:, None] + np.arange(N)[None, :]]


def forward64(blocks, N):
    """fftshift(fft(block)) / N in complex128 — never rounded to complex64"""
    y = np.fft.fft(np.asarray(blocks).astype(np.complex128).reshape(-1, N), axis=-1)
    return np.fft.fftshift(y, axes=-1) / N


def forward32(blocks, N, fwd):
    """the same with one of FLOAT32_MODELS (or any complex64 transform of that signature), rounded to complex64 after the exact 1/N"""
    y = np.asarray(fwd(np.asarray(blocks).astype(np.complex64).reshape(-1, N)))
    assert y.dtype == np.complex64
    return np.fft.fftshift(y, axes=-1) * np.float32(1.0 / N)


def chain64(blocks, N, R, chan, window_rows, first_block=0, spec=None):
    """The chain in complex128.  spec: forward64(blocks, N) when the caller already has it (many channel groups on one input)."""
    return channel_stage64(forward64(blocks, N) if spec is None else spec, N, R, chan, window_rows, first_block)


def chain32(blocks, N, R, chan, window_rows, first_block=0, fwd=fft32_model, inv=fft32_model, spec=None):
    """The chain with complex64 intermediates: fwd and inv each one of FLOAT32_MODELS.  spec: forward32(blocks, N, fwd) when the caller has it."""
    return channel_stage32(forward32(blocks, N, fwd) if spec is None else spec, N, R, chan, window_rows, first_block, transform=inv)


def chain_model_error(blocks, N, R, chan, window_rows, first_block, ref, specs=None):
    """E of every row: the largest (rms, max) error, relative to max|ref| (model_error), over the four combinations.  specs: {fwd: forward32(...)}."""
    e_rms = e_max = None
    for fwd, inv in CHAIN_COMBINATIONS:
        y = chain32(blocks, N, R, chan, window_rows, first_block, fwd, inv, None if specs is None else specs[fwd])
        a, b = model_error(y, ref)
        e_rms, e_max = (a, b) if e_rms is None else (np.maximum(e_rms, a), np.maximum(e_max, b))
    return e_rms, e_max


def chain_noise_stream(N, R, seed):
    """R + 1 blocks of noise: every window row occurs"""
    return noise((R + 1) * (N - N // R), seed)


def chain_impulse_stream(N, R):
    """One unit impulse per block: block m + 1 holds one at impulse_positions(N)[m] (block 0 begins with the N/R zeros in front of the stream and
    cannot hold the positions below N/R: it only sees block 1's impulse, N - N/R later — as every block sees a neighbour's impulse when that lies
    in the samples the two share; the reference has them all).  len(impulse_positions(N)) + 1 blocks."""
    ovl = N // R
    H = N - ovl
    pos = impulse_positions(N)
    s = np.zeros((len(pos) + 1) * H, dtype=np.complex64)
    for m, p in enumerate(pos):
        s[(m + 1) * H + p - ovl] = 1.0
    return s


def chain_tone_stream(N, R, cut, j):
    """R + 1 blocks of a sum of exact-bin tones, one inside every channel's slice: channel c = cut[c] = (f, l) takes bin
    f + slice_positions(l)[(c + j) % len] of the shifted spectrum.  Every block behind block 0 (which begins with zeros) transforms to one impulse
    per slice, every channel row to one window value times a pure exponential.  Summed in float64 (one period by an inverse transform of the
    impulses), rounded once."""
    H = N - N // R
    X = np.zeros(N, dtype=np.complex128)
    for c, (f, l) in enumerate(cut):
        pos = slice_positions(l)
        X[f + pos[(c + j) % len(pos)]] = 1.0
    period = np.fft.ifft(np.fft.ifftshift(X)) * N
    return period[np.arange((R + 1) * H) % N].astype(np.complex64)


def chain_tone_calls(cut):
    """How many calls j of chain_tone_stream it takes until every slice position has met every residue of c mod 16 that the plan has, per width"""
    need = set((l, i, c % 16) for c, (f, l) in enumerate(cut) for i in range(len(slice_positions(l))))
    j = 0
    while need:
        need -= set((l, (c + j) % len(slice_positions(l)), c % 16) for c, (f, l) in enumerate(cut))
        j += 1
    return j


def quantise(stream, bits=16):
    """(integers (n, 2), scale): the stream on the finest power-of-two grid that keeps its peak inside `bits`-bit integers; the samples a kernel then
    works on are integers * scale, exact in float32"""
    s = np.asarray(stream)
    top = max(float(np.abs(s.real).max()), float(np.abs(s.imag).max()), 1e-30)
    k = int(np.floor(np.log2((2 ** (bits - 1) - 1) / top)))
    q = np.stack([np.rint(s.real * 2.0 ** k), np.rint(s.imag * 2.0 ** k)], axis=-1).astype(np.int16 if bits == 16 else np.int8)
    return q, 2.0 ** -k


# ---------------------------------------------------------------- inputs
def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def impulse_positions(n):
    """Positions in [0, n) that between them set (and clear) every bit of the index: 0, 1, n/2, n - 1, every single bit, and the alternating patterns."""
    pos = [0, 1, n // 2, n - 1] + [1 << b for b in range(max(n.bit_length() - 1, 0))]
    pos += [m & (n - 1) for m in (0x555555, 0xAAAAAA, 0x333333, 0xCCCCCC)]
    out = []
    for p in pos:
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def wide_impulse_positions(n, count=4):
    """For a two-pass size n = N1 * N2 (N1 = 2**ceil(log2 n / 2)): positions p with both p mod N1 and p div N1 non-zero — so the impulse meets a
    column transform, the W_n product between the passes and a row transform — the last one n - 1."""
    lg = n.bit_length() - 1
    N1 = 1 << ((lg + 1) // 2)
    N2 = n // N1
    pos = [1 + N1 * 1, (N1 - 1) + N1 * (N2 // 2), ((0x555555 & (N1 - 1)) | 1) + N1 * ((0xAAAAAA & (N2 - 1)) | 1)][:max(count - 1, 0)] + [n - 1]
    assert all(p % N1 and p // N1 for p in pos)
    return pos


def impulses(n, positions):
    x = np.zeros((len(positions), n), dtype=np.complex64)
    x[np.arange(len(positions)), positions] = 1.0
    return x


def tone(n, k):
    """exp(2 pi i k t / n), t < n, rounded to complex64: its forward transform is bin k at height n, every other bin is rounding."""
    a = 2.0 * np.pi * ((k * np.arange(n, dtype=np.int64)) % n) / n
    return (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)


def block_scale(m):
    """Block m's items times 2**(3 (m mod 5) - 6): exact, and neighbouring rows differ by up to 2**12 — a row written under the wrong block is not
    within any rounding of the right one."""
    return np.float32(2.0 ** (3 * (np.asarray(m) % 5) - 6))


def slice_positions(l):
    """The walk of the impulse over a channel's slice of l bins: the edges and the middle (where the ifftshift cuts), the alternating patterns, every
    single bit."""
    pos = [0, 1, l // 2 - 1, l // 2, l - 1] + [m & (l - 1) for m in (0x555555, 0xAAAAAA, 0x333333, 0xCCCCCC)] + [1 << b for b in range(l.bit_length() - 1)]
    out = []
    for p in pos:
        if 0 <= p < l and p not in out:
            out.append(p)
    return out


def channel_noise_items(N, first_block, nb, seed):
    """nb spectrum items of noise, block m (counted from the stream's start) times block_scale(m)"""
    return noise((nb, N), seed) * block_scale(first_block + np.arange(nb))[:, None]


def channel_impulse_items(N, chans, first_block, nb):
    """nb spectrum items, block m: block_scale(m) at one bin inside every channel's slice, the bin walking over slice_positions(l) with m — alone in
    its slice, a channel's output row is one window value times a pure exponential: the inverse transform's tables, bare."""
    x = np.zeros((nb, N), dtype=np.complex64)
    for i in range(nb):
        m = first_block + i
        for (f, l) in chans:
            pos = slice_positions(l)
            x[i, f + pos[m % len(pos)]] = block_scale(m)
    return x


# ---------------------------------------------------------------- the criterion
def item_errors(y, ref):
    """(rms error, max error, max|ref|) of every row of y against ref, as float64 arrays."""
    d = np.abs(np.asarray(y).astype(np.complex128) - ref)
    return np.sqrt(np.mean(d * d, axis=-1)), d.max(axis=-1), np.abs(ref).max(axis=-1)


def relative_errors(y, ref):
    """(rms error / rms ref, max error / max|ref|) of every row: the two figures of the suite's present criterion."""
    rms, mx, top = item_errors(y, ref)
    return rms / np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1)), mx / top


def model_error(model, ref):
    """E_model: the model's (rms error / max|ref|, max error / max|ref|) per row — relative to the output's scale, so that it carries over to the other
    three forms of the same transform (whose outputs are the same values in another order, or conjugate-mirrored ones)."""
    rms, mx, top = item_errors(model, ref)
    one = np.where(top > 0, top, 1.0)
    return rms / one, mx / one


def transform_model_error(x, ref):
    """E_model of the forward unshifted transform of the rows of x: the larger of the float32 models' errors (radix 2, and the steps of a radix-16 /
    two-pass transform) on each row"""
    es = [model_error(t(x), ref) for t in FLOAT32_MODELS]
    return np.maximum(es[0][0], es[1][0]), np.maximum(es[0][1], es[1][1])


def ratios(y, ref, e_model):
    """The device's error over its bound's base, per row: (rms error / max(E_rms, ulp / L2_FACTOR), max error / max(E_max, ulp / MAX_FACTOR)), each
    relative to max|ref|.  A row passes when the first is <= L2_FACTOR and the second <= MAX_FACTOR — that is, rms <= max(2 E_rms, ulp) and
    max <= max(3 E_max, ulp)."""
    rms, mx, top = item_errors(y, ref)
    e_rms, e_max = e_model
    one = np.where(top > 0, top, 1.0)                      # a row whose reference is all zeros has to come out as zeros (ratio 0, or inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_l2 = np.where(top > 0, (rms / one) / np.maximum(e_rms, ULP / L2_FACTOR), np.where(mx == 0, 0.0, np.inf))
        r_max = np.where(top > 0, (mx / one) / np.maximum(e_max, ULP / MAX_FACTOR), np.where(mx == 0, 0.0, np.inf))
    return r_l2, r_max
