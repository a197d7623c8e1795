"""THE DEFINITION of the packed channel audio (fdc_pipeline_set_audio_packing; include/fdc_amd.h), in numpy with plain loops: the reference for bits.

The audio is on with decimation D and the squelch is on.  npb[c] = lout_c / D.  A CELL is (m, c): block m of the call, channel c; its weight is
w(m, c) = mask[m][c] * npb[c].  Cells are ordered ROW-MAJOR, m outer and c inner.  off(m, c) is the sum of w over all cells in front of (m, c) (for a
closed cell: where it would go); count is the sum over all cells.  packed[off(m, c) + i] = audio[m][aoff_c + i] for every OPEN cell and
0 <= i < npb[c], audio being the [nblocks][A] matrix the audio pass gives without packing (gated or not: both hold the same bits on open cells),
aoff_c the sum of npb over the channels in front of c.  Offsets start at 0 in every call: the packing has no stream state of its own."""
import numpy as np


def offsets(mask, npb, base=0):
    """(off int64 [nblocks][C], count): a double loop over the cells in their order"""
    mask = np.asarray(mask)
    nb, nc = mask.shape
    assert len(npb) == nc
    off = np.zeros((nb, nc), np.int64)
    run = int(base)
    for m in range(nb):
        for c in range(nc):
            off[m, c] = run
            if mask[m, c]:
                run += int(npb[c])
    return off, run


def pack(audio, mask, npb):
    """the packed array of a call: audio [nblocks][A] (any dtype), mask [nblocks][C].  Returns (packed 1-D of the audio's dtype, count)"""
    audio, mask = np.asarray(audio), np.asarray(mask)
    nb, nc = mask.shape
    assert audio.shape == (nb, int(sum(npb)))
    off, count = offsets(mask, npb)
    out = np.zeros(count, audio.dtype)
    for m in range(nb):
        aoff = 0
        for c in range(nc):
            if mask[m, c]:
                for i in range(int(npb[c])):
                    out[off[m, c] + i] = audio[m, aoff + i]
            aoff += int(npb[c])
    return out, count


def unpack(packed, mask, npb):
    """one 1-D array per channel: the channel's open blocks in order, mask[:, c].sum() * npb[c] samples"""
    packed, mask = np.asarray(packed), np.asarray(mask)
    nb, nc = mask.shape
    off, count = offsets(mask, npb)
    assert packed.shape == (count,)
    out = []
    for c in range(nc):
        seg = [packed[off[m, c]:off[m, c] + int(npb[c])] for m in range(nb) if mask[m, c]]
        out.append(np.concatenate(seg) if seg else np.zeros(0, packed.dtype))
    return out


def npb_of(lout, decim):
    assert all(int(lo) % int(decim) == 0 for lo in lout)
    return [int(lo) // int(decim) for lo in lout]
