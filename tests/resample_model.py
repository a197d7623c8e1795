"""The numpy model of the audio resampler behind the channel demodulation (fdc_pipeline_set_audio_resampler): a polyphase FIR with interpolation L = up
and decimation M = down, GNU Radio's rational_resampler_fff started at sample 0.  It is the definition the device pass reproduces bit for bit.

With d[t] the float32 stream the demodulation gives for one channel, t the ABSOLUTE sample index (sample 0 is the first of block 0; block m holds the
samples m lout .. (m + 1) lout - 1; d = +0 in front of the stream's start), h[0 .. ntaps-1] the float32 prototype taps, Kp = ceil(ntaps / L) and h
padded with +0 to L Kp entries, output n (n = 0, 1, ...; it stands at input time n M / L) is

    a[n] = sum over k = 0 .. Kp-1 of h[k L + (n M mod L)] d[floor(n M / L) - k]

THE ORDER IS PART OF THE DEFINITION: float32, k ascending, from acc = +0, every product and every sum rounded on its own (audio_model.fir_decim32's
rule).  The padded zero taps are part of the sum, so NaN and +-Inf in d follow IEEE through them.  With L = 1 this is fir_decim32 with D = M.

Output n belongs to the block of its newest sample, floor(floor(n M / L) / lout): block m owns the outputs ceil(m lout L / M) .. ceil((m+1) lout L / M) - 1
(block_counts), W or W - 1 of them with W = ceil(lout L / M).  The audio of a call is the block-major matrix [nblocks][A], A = sum of the W_c: cell
(m, c) holds its outputs in order and, where it owns W_c - 1, one pad of zero bits (matrix).  A closed cell of a gated call is all zero bits.

The history rule is audio_model.History with K = Kp; phase and counts come from the absolute index of the call's first block whether or not the
history is used."""
import numpy as np

from audio_model import F32, History, f32, s16          # noqa: F401  (History, s16: the rules shared with the decimating form)


def ceil_div(a, b):
    return -((-a) // b)


def phase_taps(taps, up):
    """(Kp, hp) with hp[ph, k] = h[k up + ph], h padded with +0 to up Kp entries"""
    h = f32(taps)
    kp = ceil_div(h.size, up)
    return kp, np.concatenate([h, np.zeros(up * kp - h.size, F32)]).reshape(kp, up).T.copy()


def first_output(block, lout, up, down):
    """the index of the first output block `block` owns: ceil(block lout up / down), in exact integers"""
    return ceil_div(int(block) * int(lout) * int(up), int(down))


def block_counts(lout, up, down, first_block, nblocks):
    """the outputs each of the blocks first_block .. first_block + nblocks - 1 owns (Python integers inside: first_block may be 2^40 and more)"""
    edge = [first_output(int(first_block) + i, lout, up, down) for i in range(int(nblocks) + 1)]
    return np.array([edge[i + 1] - edge[i] for i in range(int(nblocks))], dtype=np.int64)


def _call(d, taps, up, down, lout, first_block, hist, dtype):
    """(z, at, ph, hp): z the call's samples behind the Kp - 1 in front of them, at[i] the index in z of output i's newest sample, ph[i] its phase"""
    kp, hp = phase_taps(taps, up)
    d = np.ascontiguousarray(d, dtype).reshape(-1)
    assert d.size % lout == 0, "a call is whole blocks"
    front = np.zeros(kp - 1, dtype) if hist is None else np.ascontiguousarray(hist, dtype).reshape(-1)
    assert front.size == kp - 1, (front.size, kp)
    z = np.concatenate([front, d])
    nb = d.size // lout
    n0, n1 = first_output(first_block, lout, up, down), first_output(int(first_block) + nb, lout, up, down)
    e0 = n0 * down - int(first_block) * lout * up          # exact, in [0, down): where the call's first output stands, counted from its first sample
    assert 0 <= e0 < down
    pos = e0 + down * np.arange(n1 - n0, dtype=np.int64)
    at, ph = pos // up + (kp - 1), pos % up
    return z, at, ph, hp, kp


def resample32(d, taps, up, down, lout, first_block=0, hist=None):
    """the outputs of one call of one channel, bit for bit: d its float32 demodulated samples (whole blocks of lout), hist the Kp - 1 in front"""
    z, at, ph, hp, kp = _call(d, taps, up, down, lout, first_block, hist, F32)
    acc = np.zeros(at.size, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(kp):
            p = hp[ph, k] * z[at - k]           # float32 x float32 -> float32: rounded once
            acc = acc + p                       # and the sum rounded on its own
    assert acc.dtype == F32
    return acc


def resample64(d, taps, up, down, lout, first_block=0, hist=None, absolute=False):
    """the same sum in float64 of float64 d and the float32 taps (absolute: of |h| and |d|, the bound's sum)"""
    z, at, ph, hp, kp = _call(d, taps, up, down, lout, first_block, hist, np.float64)
    hp = hp.astype(np.float64)
    if absolute:
        z, hp = np.abs(z), np.abs(hp)
    acc = np.zeros(at.size, np.float64)
    for k in range(kp):
        acc = acc + hp[ph, k] * z[at - k]
    return acc


def audio32(d, taps, up, down, lout, first_block=0, fmt="f32", scale=1.0, hist=None):
    a = resample32(d, taps, up, down, lout, first_block, hist)
    return s16(a, scale) if fmt == "s16" else a


def matrix(chan_out, louts, up, down, first_block, nblocks, mask=None):
    """the call's matrix [nblocks][A] of the channels' outputs (one array per channel: resample32 / audio32 of the call): pads of zero bits, and with
    mask ([nblocks][C], nonzero: open) the closed cells all zero bits"""
    per = [ceil_div(int(lo) * up, down) for lo in louts]
    dtype = chan_out[0].dtype if len(chan_out) else F32
    mat = np.zeros((nblocks, sum(per)), dtype)
    col = 0
    for c, lo in enumerate(louts):
        cnt = block_counts(lo, up, down, first_block, nblocks)
        assert cnt.sum() == chan_out[c].size, (cnt.sum(), chan_out[c].size)
        assert ((cnt == per[c]) | (cnt == per[c] - 1)).all()
        at = 0
        for m in range(nblocks):
            if mask is None or mask[m][c]:
                mat[m, col:col + cnt[m]] = chan_out[c][at:at + cnt[m]]
            at += cnt[m]
        col += per[c]
    return mat


def stream(history, calls, taps, up, down, louts, fmt="f32", scale=1.0, masks=None):
    """calls: [(first_block, nblocks, [d_c of the call, one float32 array per channel])]; the model's matrix of every call.  history: audio_model.History
    with K = Kp"""
    out = []
    for i, (first, nb, ds) in enumerate(calls):
        fr = history.front(first)
        a = [audio32(d, taps, up, down, louts[c], first, fmt, scale, fr[c]) for c, d in enumerate(ds)]
        out.append(matrix(a, louts, up, down, first, nb, None if masks is None else masks[i]))
        history.done(first, nb, ds)
    return out
