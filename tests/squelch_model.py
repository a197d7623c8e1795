"""The channel squelch (fdc_pipeline_set_squelch; include/fdc_amd.h CHANNEL SQUELCH) stated in numpy: THE DEFINITION the device is held to, byte for byte.

The setting: per-channel float32 thresholds open_c >= close_c >= 0 (finite) and one hang count of blocks, 0 .. 65535.  Per channel the state is
(open in {0, 1}, h in [0, hang]); it starts as (0, 0).  For block m of the stream, in order:
    p  = power[m][c]                     the float32 the levels hold (after fine tuning and the gain)
    g2 = f32(g_c g_c)                    g_c the channel gain in force, 1 while the gains are off
    To = f32(g2 open_c), Tc = f32(g2 close_c)
    if p >= To:              open = 1, h = hang
    elif open and p >= Tc:   h = hang
    elif open:               h -= 1 if h > 0, else open = 0
    mask[m][c] = open
Every comparison is an IEEE float32 >=: a NaN power or a NaN threshold product is below.
A state is READ as (open != 0, min(max(h, 0), hang in force)), and a closed state as (0, 0): h means nothing while the channel is closed, and it is
written as 0 then.

scan_mask is the same rule in the parallel form the kernel runs (three integer max-scans over the block index); tests/test_squelch_cpu.py proves the
two equal."""
import numpy as np

HANG_MAX = 65535
NEG = -(1 << 30)


def thresholds(gain, open_thr, close_thr):
    """(To, Tc) float32 [C]: the threshold products of the rule, each rounded once"""
    o = np.asarray(open_thr, dtype=np.float32).reshape(-1)
    c = np.asarray(close_thr, dtype=np.float32).reshape(-1)
    g = np.ones(o.size, np.float32) if gain is None else np.asarray(gain, dtype=np.float32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        g2 = (g * g).astype(np.float32)
        return (g2 * o).astype(np.float32), (g2 * c).astype(np.float32)


def classes(power, gain, open_thr, close_thr):
    """(strong, low) bool [M][C]: strong is p >= To; low is neither p >= To nor p >= Tc"""
    p = np.asarray(power, dtype=np.float32)
    To, Tc = thresholds(gain, open_thr, close_thr)
    with np.errstate(invalid="ignore"):
        strong = p >= To[None, :]
        low = ~strong & ~(p >= Tc[None, :])
    return strong, low


def read_state(state, C, hang):
    """the state as the rule reads it: int64 [C][2]"""
    st = np.zeros((C, 2), np.int64) if state is None else np.asarray(state, dtype=np.int64).reshape(C, 2).copy()
    st[:, 0] = st[:, 0] != 0
    st[:, 1] = np.where(st[:, 0] != 0, np.clip(st[:, 1], 0, hang), 0)
    return st


def run_classes(strong, low, hang, state=None):
    """the sequential rule over class sequences [M][C]: (mask uint8 [M][C], state int32 [C][2])"""
    strong, low = np.asarray(strong, bool), np.asarray(low, bool)
    M, C = strong.shape
    st = read_state(state, C, hang)
    mask = np.zeros((M, C), np.uint8)
    for c in range(C):
        o, h = int(st[c, 0]), int(st[c, 1])
        for m in range(M):
            if strong[m, c]:
                o, h = 1, hang
            elif o and not low[m, c]:
                h = hang
            elif o:
                if h > 0:
                    h -= 1
                else:
                    o = 0
            mask[m, c] = o
        st[c] = (o, h if o else 0)
    return mask, st.astype(np.int32)


def scan_classes(strong, low, hang, state=None):
    """the same in the scan form.  Block m is open iff a strong block lies at or before m and no run of hang + 1 consecutive low blocks has ended
    behind that strong block and at or before m.  Three max-scans over the block index: s = the last strong block, nl = the last block that is not low
    (m - nl is the length of the run of low blocks that ends at m), e = the last block at which that length reached hang + 1; open = s > e.  An open
    carried state (1, h) stands for a strong block at index -1 - (hang - h), with hang - h low blocks behind it"""
    strong, low = np.asarray(strong, bool), np.asarray(low, bool)
    M, C = strong.shape
    st = read_state(state, C, hang)
    idx = np.arange(M, dtype=np.int64)[:, None]
    s0 = np.where(st[:, 0] != 0, -1 - (hang - st[:, 1]), NEG)
    n0 = np.where(st[:, 0] != 0, s0, -1)
    s = np.maximum.accumulate(np.vstack([s0[None, :], np.where(strong, idx, NEG)]), axis=0)[1:]
    nl = np.maximum.accumulate(np.vstack([n0[None, :], np.where(~low, idx, NEG)]), axis=0)[1:]
    e = np.maximum.accumulate(np.vstack([np.full((1, C), NEG), np.where(idx - nl >= hang + 1, idx, NEG)]), axis=0)[1:]
    mask = (s > e).astype(np.uint8)
    out = np.zeros((C, 2), np.int32)
    if M:
        out[:, 0] = mask[-1]
        out[:, 1] = np.where(mask[-1] != 0, hang - ((M - 1) - nl[-1]), 0)
    else:
        out[:] = st
    return mask, out


def squelch(power, gain, open_thr, close_thr, hang, state=None):
    """the squelch of M blocks: power float32 [M][C] (the levels' first component), gain [C] or None -> (mask uint8 [M][C], state int32 [C][2])"""
    strong, low = classes(power, gain, open_thr, close_thr)
    return run_classes(strong, low, int(hang), state)


class Stream:
    """the state across calls as the handle keeps it: a call continues where its first_block is `next`, else it restarts at (0, 0)"""

    def __init__(self, C):
        self.C, self.state, self.next = C, None, -1

    def call(self, first_block, power, gain, open_thr, close_thr, hang):
        power = np.asarray(power, np.float32).reshape(-1, self.C)
        mask, self.state = squelch(power, gain, open_thr, close_thr, hang, self.state if first_block == self.next else None)
        self.next = first_block + power.shape[0]
        return mask


def db_thresholds(lout, open_db, close_db=None):
    """thresholds in the levels' unit (the sum over a row of re^2 + im^2 = mean power times lout_c) from dB of mean power: float32 [C] each"""
    lo = np.asarray(lout, dtype=np.float64).reshape(-1)
    o = np.broadcast_to(np.asarray(open_db, dtype=np.float64), lo.shape)
    c = o if close_db is None else np.broadcast_to(np.asarray(close_db, dtype=np.float64), lo.shape)
    return (lo * 10.0 ** (o / 10.0)).astype(np.float32), (lo * 10.0 ** (c / 10.0)).astype(np.float32)
