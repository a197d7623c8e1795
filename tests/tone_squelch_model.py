"""The tone squelch (fdc_pipeline_set_tone_squelch; include/fdc_amd.h TONE SQUELCH) stated in numpy, plain loops: THE DEFINITION the device is held to,
byte for byte.

The setting: per channel a tone index tone_c (-1: the channel is not tone-gated, else 0 .. T - 1), float32 thresholds open_c >= close_c >= 0 and a
float32 ratio_c >= 0, all finite; for all channels a guard 0 .. 63 and a hang count of frames 0 .. 65535.

The class of a completed frame f of channel c, from its row Z[f][c][0 .. T - 1] of the channel tones (tests/tones_model.py), sel = tone_c:
    e_t = f32(f32(re re) + f32(im im))
    e   = e_sel
    o   = the largest e_t over the t with |t - sel| > guard, from +0 by "e_t > o ? e_t : o" (a NaN is never taken, the order does not matter)
    R   = f32(ratio_c o)
    strong = e >= open_c and e >= R;   hold = e >= close_c and e >= R;   low = not strong and not hold
Every comparison is an IEEE >=, so a NaN is below.

Over the frames runs exactly the carrier squelch's state machine (squelch_model.run_classes) with frames in the place of blocks: the state is
(open, h), from (0, 0); dec[f][c] = open behind frame f.

The gate is CAUSAL.  Block m of a call stands in frame j = (fill + m) div W counted from the call's first frame, fill being the tones' own.  The
decision in force for it is the carried state's open for j = 0 and dec[j - 1][c] otherwise (frame j - 1 is always completed inside the call), and
mask[m][c] = carrier_mask[m][c] AND in force.  A channel with tone -1 keeps its carrier mask and has dec = 1; its state is written as (0, 0).

The stream: the tone squelch continues exactly where the tones continue; otherwise it restarts at (0, 0) with fill 0."""
import numpy as np

from squelch_model import read_state, run_classes, scan_classes  # noqa: F401  (scan_classes: the form the kernel runs, for the tests)

GUARD_MAX, HANG_MAX = 63, 65535


def energies(row):
    """e_t float32 [T] of one row (complex64 [T]): both products and the sum rounded on their own"""
    z = np.asarray(row, dtype=np.complex64).reshape(-1)
    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
    with np.errstate(all="ignore"):
        return ((re * re).astype(np.float32) + (im * im).astype(np.float32)).astype(np.float32)


def frame_class(row, sel, open_thr, close_thr, ratio, guard):
    """(strong, low, e, o) of one row for the selected tone sel >= 0"""
    e_t = energies(row)
    e = e_t[sel]
    o = np.float32(0.0)
    for t in range(e_t.size):
        if abs(t - sel) > guard and e_t[t] > o:
            o = e_t[t]
    with np.errstate(all="ignore"):
        R = np.float32(np.float32(ratio) * o)
        strong = bool(e >= np.float32(open_thr)) and bool(e >= R)
        hold = bool(e >= np.float32(close_thr)) and bool(e >= R)
    return strong, (not strong and not hold), e, o


def classes(Z, tone, open_thr, close_thr, ratio, guard):
    """(strong, low) bool [nf][C] of the rows Z complex64 [nf][C][T]; a channel with tone -1 is never strong and always low (its dec is set apart)"""
    Z = np.asarray(Z, dtype=np.complex64)
    nf, C = Z.shape[0], Z.shape[1]
    strong, low = np.zeros((nf, C), bool), np.ones((nf, C), bool)
    for c in range(C):
        if tone[c] < 0:
            continue
        for f in range(nf):
            strong[f, c], low[f, c] = frame_class(Z[f, c], int(tone[c]), open_thr[c], close_thr[c], ratio[c], int(guard))[:2]
    return strong, low


def decide(Z, tone, open_thr, close_thr, ratio, guard, hang, state=None):
    """the decisions of nf completed frames: (dec uint8 [nf][C], state int32 [C][2]).  No frame: the state as it is read"""
    tone = np.asarray(tone, dtype=np.int64).reshape(-1)
    C = tone.size
    Z = np.zeros((0, C, 1), np.complex64) if Z is None else np.asarray(Z, dtype=np.complex64)
    assert Z.ndim == 3 and Z.shape[1] == C
    strong, low = classes(Z, tone, open_thr, close_thr, ratio, guard)
    if Z.shape[0]:
        dec, st = run_classes(strong, low, int(hang), state)
    else:
        dec, st = np.zeros((0, C), np.uint8), read_state(state, C, int(hang)).astype(np.int32)
    for c in range(C):
        if tone[c] < 0:
            dec[:, c] = 1
            st[c] = (0, 0)
    return dec, st


def gate(carrier_mask, dec, tone, W, fill, state=None):
    """the causal expansion: mask uint8 [nb][C] = carrier_mask AND the decision in force at each block"""
    cm = np.asarray(carrier_mask, dtype=np.uint8)
    nb, C = cm.shape
    out = np.zeros((nb, C), np.uint8)
    for m in range(nb):
        j = (fill + m) // W
        for c in range(C):
            if tone[c] < 0:
                f = 1
            elif j == 0:
                f = 0 if state is None else int(np.asarray(state).reshape(C, 2)[c, 0] != 0)
            else:
                f = int(dec[j - 1, c] != 0)
            out[m, c] = cm[m, c] & f
    return out


def call(Z, carrier_mask, tone, open_thr, close_thr, ratio, guard, hang, W, fill=0, state=None):
    """one call: Z the (fill + nb) div W rows it completes, carrier_mask [nb][C] -> (dec, mask, new fill, new state)"""
    cm = np.asarray(carrier_mask, dtype=np.uint8)
    nb = cm.shape[0]
    dec, st = decide(Z, tone, open_thr, close_thr, ratio, guard, hang, state)
    assert dec.shape[0] == (fill + nb) // W
    return dec, gate(cm, dec, tone, W, fill, state), (fill + nb) % W, st


class Stream:
    """the state across calls as the handle keeps it: a call continues where its first_block is `next` (the tones' own position), else it restarts at
    (0, 0) with fill 0; a new setting (restart()) restarts the state only"""

    def __init__(self, C, W):
        self.C, self.W, self.state, self.fill, self.next = C, W, None, 0, -1

    def restart(self):
        self.state = None

    def call(self, first_block, Z, carrier_mask, tone, open_thr, close_thr, ratio, guard, hang):
        if first_block != self.next:
            self.state, self.fill = None, 0
        cm = np.asarray(carrier_mask, dtype=np.uint8).reshape(-1, self.C)
        dec, mask, self.fill, self.state = call(Z, cm, tone, open_thr, close_thr, ratio, guard, hang, self.W, self.fill, self.state)
        self.next = first_block + cm.shape[0]
        return dec, mask
