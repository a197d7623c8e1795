"""Host-side counterpart of the reference's Python caller, python/FrequencyDomainChannelizer.py.

`FrequencyDomainChannelizer` takes the same constructor arguments as the reference hier block (:46-60),
derives the same channel parameters (:322-345) and lowers the throughput part of the flowgraph
(:200-231, :283-299) to ONE fused device pipeline behind the C-ABI (include/fdc_amd.h) instead of
4 + 6*C GNU Radio blocks.  `Pipeline` is the thin object over fdc_pipeline_* used by it, by the tests
and by bench.py.
"""
import ctypes as C
import math

import numpy as np

from . import _lib


class FREQMODE:                      # python/FrequencyDomainChannelizer.py:31-32
    normalized, basebandfs, centerfreqfs = range(3)


class VERBOSEMODE:                   # python/FrequencyDomainChannelizer.py:34-35
    NOLOG, LOGTOCONSOLE, LOGTOFILE = range(3)


class WINDOWTYPES:                   # lib/windows.h:28-32
    RECTANGULAR, HANN, RAMP = range(3)


def nextpow2(k):
    """Smallest power of two >= k (python/FrequencyDomainChannelizer.py:37-40); ValueError for k < 1."""
    if k < 1:
        raise ValueError('Cannot evaluate next power 2 of {}'.format(k))
    return 1 << int(math.ceil(math.log2(k)))


def get_opt_channelparams(blocksize, relinvovl, freq, bw):
    """(freq, bw) in INTERNAL units -> (f, l, lout, passband, stopband).

    Same decisions as the reference method (python/FrequencyDomainChannelizer.py:322-345): slice length =
    next power of two of the occupied bins with at least 20 % head-room, pass band 10 % wider than the
    signal, stop band at the slice edge unless the pass band is below 0.7, slice centred on the rounded
    carrier bin, wrapped below zero and clamped at the upper band edge."""
    occupied = blocksize * bw
    l = nextpow2(occupied)
    if l < 1.2 * occupied:
        l *= 2
    passband = float(occupied) / float(l) * 1.1
    stopband = 1.0
    if passband >= 1.0:
        passband = 1.0
    elif passband < 0.7:
        stopband = passband + 0.25
    # round(): the reference runs under Python 2 (half away from zero); Python 3's round() goes half to even
    centre = int(_round_half_away(freq * blocksize)) % blocksize
    first = centre - l / 2
    if first < 0:
        first = (first + blocksize) % blocksize
    if first + l > blocksize:
        first = blocksize - l
    return int(first), int(l), int(l) - int(l) // relinvovl, float(passband), float(stopband)


def _round_half_away(x):
    """Python 2's round() (and C's round()): to the nearest integer, ties away from zero — decided on the fraction itself,
    not on x + 0.5 (0.49999999999999994 + 0.5 rounds up to 1.0 in double; odd integers from 2^52 on would move too)."""
    ax = abs(x)
    r = math.floor(ax)
    if ax - r >= 0.5:
        r += 1.0
    return r if x >= 0 else -r


def freq_converters(freqmode, fs=1.0, centerfrequency=0.0):
    """(mode, get_freq, set_freq, get_bw, set_bw) of the three frequency conventions of the hier block
    (python/FrequencyDomainChannelizer.py:70-91): user frequency -> internal [0, 1) with DC at 0.5, and back.
    The mode may be given as the FREQMODE integer or as its name."""
    if freqmode in (FREQMODE.normalized, 'normalized'):
        return (FREQMODE.normalized, lambda f: (f + 0.5) % 1.0, lambda f: f - 0.5, lambda bw: bw % 1.0, lambda bw: bw)
    if freqmode in (FREQMODE.basebandfs, 'basebandfs'):
        return (FREQMODE.basebandfs, lambda f: (f / fs + 0.5) % 1.0, lambda f: (f - 0.5) * fs,
                lambda bw: (bw / fs) % 1.0, lambda bw: bw * fs)
    if freqmode in (FREQMODE.centerfreqfs, 'centerfreqfs'):
        return (FREQMODE.centerfreqfs, lambda f: ((f - centerfrequency) / fs + 0.5) % 1.0,
                lambda f: (f - 0.5) * fs + centerfrequency, lambda bw: (bw / fs) % 1.0, lambda bw: bw * fs)
    raise ValueError('Unknown Frequency mode. Exiting...')


def register_host(arr):
    """Pin a numpy array for fdc_pipeline_work (fdc_host_register): calls whose input / outputs are slices of pinned
    arrays are DMA'd in place.  Keep the array alive until unregister_host(arr)."""
    _lib.check(_lib.lib().fdc_host_register(arr.ctypes.data, arr.nbytes))


def unregister_host(arr):
    _lib.check(_lib.lib().fdc_host_unregister(arr.ctypes.data))


# Process-wide defaults for the kernel-choice fields of fdc_pipeline_cfg (flags, min_block_launch, host_sub_blocks) of pipelines
# created without them: how tests and A/B tools force a path.  Keys (the library itself reads no environment variable):
#   "FDC_FORCE_GENERIC" / "FDC_NO_POLY" / "FDC_NO_BLOCK" / "FDC_NO_FUSED" / "FDC_FULL_SPECTRUM" -> FDC_PIPE_* flags, "FDC_BLOCK_MIN_BLOCKS" -> min_block_launch,
#   "FDC_HOST_SUB" -> host_sub_blocks, "FDC_BLOCK_HINTS" (bit 0 nt stores, bit 1 nt loads)
defaults = {}


def _default_cfg_fields():
    flags = 0
    if defaults.get("FDC_FORCE_GENERIC"):
        flags |= _lib.FDC_PIPE_FORCE_GENERIC
    if defaults.get("FDC_NO_POLY"):
        flags |= _lib.FDC_PIPE_NO_POLY
    if defaults.get("FDC_NO_BLOCK"):
        flags |= _lib.FDC_PIPE_NO_BLOCK
    if defaults.get("FDC_FULL_SPECTRUM"):
        flags |= _lib.FDC_PIPE_FULL_SPECTRUM
    if defaults.get("FDC_WIDE_UNIFORM"):
        flags |= _lib.FDC_PIPE_WIDE_UNIFORM
    if defaults.get("FDC_NO_FUSED"):
        flags |= _lib.FDC_PIPE_NO_FUSED
    if "FDC_BLOCK_HINTS" in defaults:
        h = int(defaults["FDC_BLOCK_HINTS"])
        flags |= (0 if h & 1 else _lib.FDC_PIPE_PLAIN_STORES) | (_lib.FDC_PIPE_NT_LOADS if h & 2 else 0)
    return flags, int(defaults.get("FDC_BLOCK_MIN_BLOCKS", 0) or 0), int(defaults.get("FDC_HOST_SUB", 0) or 0)


def plan_preview(blocklen, relinvovl, channels, windowtype=WINDOWTYPES.HANN, max_blocks=64, flags=0):
    """fdc_pipeline_plan_preview: what fdc_pipeline_create would choose for this plan — (path, description, assignment) — without a device.
    assignment[c]: k >= 0 = bank k (one block-kernel launch each), -1 = the spectrum path, -2 - c0 = a copy of channel c0's output."""
    chans = [(int(f), int(l), float(p), float(s)) for (f, l, p, s) in channels]
    arr = (_lib.fdc_channel * max(1, len(chans)))()
    for i, (f, l, p, s) in enumerate(chans):
        arr[i].f, arr[i].l, arr[i].passbw, arr[i].stopbw = f, l, p, s
    cfg = _lib.fdc_pipeline_cfg(0, int(blocklen), int(relinvovl), int(windowtype), len(chans), arr, int(max_blocks), 0, 0, int(flags), 0, 0)
    buf = C.create_string_buffer(640)
    asg = (C.c_int32 * max(1, len(chans)))()
    rc = _lib.lib().fdc_pipeline_plan_preview(C.byref(cfg), buf, 640, asg)
    if rc == -1:
        raise ValueError(_lib.lib().fdc_last_error().decode())
    _lib.check(rc)
    return rc, buf.value.decode(), [int(asg[i]) for i in range(len(chans))]


IQ_SC16, IQ_SC8 = 1, 2          # FDC_IQ_SC16 / FDC_IQ_SC8 (include/fdc_amd.h)
IQ_FORMATS = {"sc16": IQ_SC16, "sc8": IQ_SC8}


def iq_format(x):
    """The C-ABI format of a complex integer array: int16 -> FDC_IQ_SC16, int8 -> FDC_IQ_SC8; other dtypes raise TypeError."""
    dt = np.asarray(x).dtype if not isinstance(x, np.dtype) else x
    if dt == np.int16:
        return IQ_SC16
    if dt == np.int8:
        return IQ_SC8
    raise TypeError("complex integer input is int16 (sc16) or int8 (sc8) interleaved I/Q, not %s" % dt)


def _iq_input(x, scale, H):
    """Checks of the _iq entries made before any library call: dtype (TypeError), shape (flat interleaved I/Q or (n, 2)), a whole number
    of (N - N/R)-sample items, a finite non-zero scale.  Returns (contiguous array, format, complex sample count, scale as float32)."""
    if not isinstance(x, np.ndarray):
        raise TypeError("complex integer input must be a numpy int16 or int8 array")
    fmt = iq_format(x)
    if x.ndim == 2:
        if x.shape[1] != 2:
            raise ValueError("complex integer input of shape (n, 2) holds I and Q in its columns; got shape %s" % (x.shape,))
    elif x.ndim != 1:
        raise ValueError("complex integer input is a flat interleaved array or one of shape (n, 2); got shape %s" % (x.shape,))
    elif x.size % 2:
        raise ValueError("a flat interleaved I/Q array has an even number of values")
    n = x.size // 2
    if H and n % H:
        raise ValueError("input must be a whole number of (N - N/R)-sample items")
    with np.errstate(over="ignore"):
        sc = np.float32(scale)
    if not np.isfinite(sc) or sc == 0:
        raise ValueError("scale must be finite and not zero (float32), got %r" % (scale,))
    return np.ascontiguousarray(x), fmt, n, sc


OQ_FC32 = 0                     # FDC_OQ_FC32; FDC_OQ_SC16 / FDC_OQ_SC8 are IQ_SC16 / IQ_SC8 (include/fdc_amd.h)
OQ_FORMATS = {None: OQ_FC32, "fc32": OQ_FC32, "sc16": IQ_SC16, "sc8": IQ_SC8}
_OQ_DTYPES = {IQ_SC16: np.int16, IQ_SC8: np.int8}


def _oq_format(fmt, scale):
    """Checks of set_output_format made before any library call: fmt in None / "fc32" / "sc16" / "sc8" (ValueError otherwise), a finite non-zero
    float32 scale.  Returns (format code, scale as float32)."""
    if not (fmt is None or isinstance(fmt, str)) or fmt not in OQ_FORMATS:
        raise ValueError("output format is None, 'fc32', 'sc16' or 'sc8', not %r" % (fmt,))
    try:
        with np.errstate(over="ignore"):
            sc = np.float32(scale)
    except (TypeError, ValueError):
        raise ValueError("scale must be a finite, non-zero number, got %r" % (scale,))
    if not np.isfinite(sc) or sc == 0:
        raise ValueError("scale must be finite and not zero (float32), got %r" % (scale,))
    return OQ_FORMATS[fmt], sc


def fine_tuning_increment(nu):
    """fdc_fine_tuning_increment: the 64-bit phase increment per output sample of a fine-tuning frequency nu (cycles per output sample, |nu| < 0.5):
    round_half_even(nu * 2**64) mod 2**64.  ValueError for NaN and |nu| >= 0.5.  Host only."""
    inc = C.c_uint64(0)
    rc = _lib.lib().fdc_fine_tuning_increment(float(nu), C.byref(inc))
    if rc == -1:
        raise ValueError(_lib.lib().fdc_last_error().decode())
    _lib.check(rc)
    return int(inc.value)


def fine_tuning_nu(blocksize, freq, f, l):
    """The fine-tuning frequency (cycles per output sample) that puts a carrier at `freq` (INTERNAL units: cycles per input sample, DC at 0.5) at DC of
    the channel cut at bins [f, f + l) of the blocksize-point spectrum: the carrier's distance from the slice centre in bins — wrapped to the nearest
    representative modulo blocksize, so that a slice wrapped below zero gets the small residual — over l."""
    d = float(freq) * blocksize - (f + l / 2.0)
    d -= blocksize * math.floor(d / blocksize + 0.5)
    return d / l


def _set_fine_tuning(fn, handle, nchan, nu):
    """Pipeline.set_fine_tuning / PipelineGroup.set_fine_tuning: nu None (off) or one C double per channel"""
    if nu is None:
        rc = fn(handle, None, nchan)
    else:
        arr = np.ascontiguousarray(nu, dtype=np.float64)
        if arr.ndim != 1:
            raise ValueError("fine tuning takes one frequency per channel")
        rc = fn(handle, arr.ctypes.data_as(C.POINTER(C.c_double)), int(arr.size))
    if rc == -1:
        raise ValueError(_lib.lib().fdc_last_error().decode())
    _lib.check(rc)


def _check_gains(nchan, g):
    """Pipeline.set_gains / PipelineGroup.set_gains: g None (off) or one finite value per channel; float32[C] or None.  Raises before any library call."""
    if g is None:
        return None
    with np.errstate(over="ignore"):            # (a value beyond float32 becomes infinite and is refused below)
        arr = np.ascontiguousarray(g, dtype=np.float32)
    if arr.ndim != 1 or arr.size != nchan:
        raise ValueError("gains takes one value per channel (%d)" % nchan)
    if not np.isfinite(arr).all():
        raise ValueError("gains must be finite (channel %d is not)" % int(np.flatnonzero(~np.isfinite(arr))[0]))
    return arr


def _set_gains(fn, handle, nchan, g):
    arr = _check_gains(nchan, g)
    rc = fn(handle, None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_float)), nchan)
    if rc == -1:
        raise ValueError(_lib.lib().fdc_last_error().decode())
    _lib.check(rc)


SQUELCH_MAX_HANG = 65535


def _squelch_args(nchan, open_thr, close_thr, hang):
    """Pipeline.set_squelch: (float32 open[C], float32 close[C], hang), (None, None, 0) for open_thr None.  A scalar broadcasts to the channels; close_thr
    None is open_thr.  Raises before any library call."""
    if open_thr is None:
        return None, None, 0
    with np.errstate(over="ignore"):            # (a value beyond float32 becomes infinite and is refused below)
        o = np.asarray(open_thr, dtype=np.float32)
        c = o if close_thr is None else np.asarray(close_thr, dtype=np.float32)
    if o.ndim > 1 or c.ndim > 1 or (o.ndim == 1 and o.size != nchan) or (c.ndim == 1 and c.size != nchan):
        raise ValueError("the squelch thresholds are one value per channel (%d) or a scalar" % nchan)
    o, c = np.ascontiguousarray(np.broadcast_to(o, (nchan,))), np.ascontiguousarray(np.broadcast_to(c, (nchan,)))
    if not (np.isfinite(o).all() and np.isfinite(c).all()) or (o < 0).any() or (c < 0).any():
        raise ValueError("the squelch thresholds must be finite and not negative")
    if (c > o).any():
        raise ValueError("a close threshold is above its open threshold (channel %d)" % int(np.flatnonzero(c > o)[0]))
    if isinstance(hang, bool) or not isinstance(hang, (int, np.integer)) or not 0 <= int(hang) <= SQUELCH_MAX_HANG:
        raise ValueError("the squelch hang count is an integer in 0 .. %d blocks" % SQUELCH_MAX_HANG)
    return o, c, int(hang)


def squelch_thresholds(lout, open_db, close_db=None):
    """Thresholds for Pipeline.set_squelch from dB of MEAN power per sample (0 dB: a mean |y|^2 of 1, in front of the channel gain): the levels' power
    is the sum over a row of re^2 + im^2, so the threshold of channel c is lout_c * 10^(dB / 10).  open_db / close_db: a scalar or one value per
    channel; close_db None: the open thresholds.  Returns (open, close), float32[C] each."""
    lo = np.asarray(lout, dtype=np.float64).reshape(-1)
    o = np.broadcast_to(np.asarray(open_db, dtype=np.float64), lo.shape)
    c = o if close_db is None else np.broadcast_to(np.asarray(close_db, dtype=np.float64), lo.shape)
    if (c > o).any():
        raise ValueError("a close level is above its open level")
    return (lo * 10.0 ** (o / 10.0)).astype(np.float32), (lo * 10.0 ** (c / 10.0)).astype(np.float32)


DEMOD_FM, DEMOD_MAG = 1, 2        # FDC_DEMOD_FM, FDC_DEMOD_MAG (include/fdc_amd.h)


def _demod_mode(mode, gain):
    """Pipeline.set_demod: (FDC_DEMOD_* code, float32 gain).  Raises before any library call."""
    if mode is None:
        return 0, np.float32(1.0)
    if not isinstance(mode, str) or mode.lower() not in ("fm", "mag"):
        raise ValueError("demod is None, 'fm' or 'mag'")
    with np.errstate(over="ignore"):
        g = np.float32(gain)
    if not np.isfinite(g) or g == 0:
        raise ValueError("the demodulation gain must be finite and not zero")
    return (DEMOD_FM if mode.lower() == "fm" else DEMOD_MAG), g


class _OutputFormat:
    """The channel outputs in the handle's output format (fdc_pipeline_set_output_format): complex64 arrays of nblocks*lout_c samples, or
    int16 / int8 arrays of shape (nblocks*lout_c, 2) (interleaved I/Q: sc16 / sc8); float32 arrays of nblocks*lout_c samples while the channel
    demodulation is on (Pipeline.set_demod, which excludes integer output)."""
    _oq = OQ_FC32
    _oq_scale = np.float32(1.0)
    _demod = 0

    def output_format(self):
        """(format name, scale): ("fc32", 1.0), ("sc16", s) or ("sc8", s)."""
        return ({OQ_FC32: "fc32", IQ_SC16: "sc16", IQ_SC8: "sc8"}[self._oq], float(self._oq_scale))

    def _new_outs(self, nb):
        if getattr(self, "_demod", 0):              # (getattr: the allocators are also called on stand-in objects that carry lout and _oq only)
            return [np.empty(nb * lo, dtype=np.float32) for lo in self.lout]
        if self._oq == OQ_FC32:
            return [np.empty(nb * lo, dtype=np.complex64) for lo in self.lout]
        return [np.empty((nb * lo, 2), dtype=_OQ_DTYPES[self._oq]) for lo in self.lout]

    def _check_outs(self, outs, nb):
        if outs is None:
            return self._new_outs(nb)
        if len(outs) != len(self.lout):
            raise ValueError("outs needs one array per channel")
        demod = bool(getattr(self, "_demod", 0))
        dt = np.float32 if demod else np.complex64 if self._oq == OQ_FC32 else _OQ_DTYPES[self._oq]
        per = 1 if demod or self._oq == OQ_FC32 else 2
        for o, lo in zip(outs, self.lout):
            if not isinstance(o, np.ndarray) or o.dtype != dt or not o.flags.c_contiguous or o.size != per * nb * lo:
                if demod:
                    raise ValueError("outs[c] must be contiguous float32 with nblocks*lout_c samples (the channel demodulation is on)")
                if self._oq == OQ_FC32:
                    raise ValueError("outs[c] must be contiguous complex64 with nblocks*lout_c samples")
                raise ValueError("outs[c] must be contiguous %s with nblocks*lout_c interleaved I/Q samples (the output format)" % np.dtype(dt).name)
        return outs


def _levels(fn, handle, nchan, last_nb, nblocks):
    """The (power, peak) pairs of the last work call as float32[nblocks, C, 2] (fdc_pipeline_levels / fdc_pipeline_group_levels)."""
    if nblocks is None:
        if last_nb is None:
            raise ValueError("levels(): no work call yet")
        nblocks = last_nb
    nblocks = int(nblocks)
    if nblocks < 0:
        raise ValueError("levels(): negative block count")
    out = np.empty((nblocks, nchan, 2), dtype=np.float32)
    _lib.check(fn(handle, out.ctypes.data_as(C.POINTER(C.c_float)), nblocks))
    return out


def _lag1(fn, handle, nchan, last_nb, nblocks):
    """The lag-1 correlation of the last work call as complex64[nblocks, C] (fdc_pipeline_lag1 / fdc_pipeline_group_lag1)."""
    if nblocks is None:
        if last_nb is None:
            raise ValueError("lag1(): no work call yet")
        nblocks = last_nb
    nblocks = int(nblocks)
    if nblocks < 0:
        raise ValueError("lag1(): negative block count")
    out = np.empty((nblocks, nchan), dtype=np.complex64)
    _lib.check(fn(handle, out.ctypes.data_as(C.POINTER(C.c_float)), nblocks))
    return out


def lag1_frequency(s):
    """The mean frequency a lag-1 correlation S (Pipeline.lag1, any shape) stands for: angle(S) / (2 pi) as float64, in cycles per output sample —
    the unit of set_fine_tuning, so adding it to the nu in force cancels the residual.  S = 0 gives 0."""
    return np.angle(np.asarray(s, dtype=np.complex128)) / (2.0 * np.pi)


AUDIO_MAX_DECIM, AUDIO_MAX_TAPS = 64, 256


AUDIO_F32, AUDIO_S16 = 0, 1       # FDC_AUDIO_F32, FDC_AUDIO_S16 (include/fdc_amd.h)
_AUDIO_FORMATS = {"f32": AUDIO_F32, "s16": AUDIO_S16}
_AUDIO_DTYPES = {AUDIO_F32: np.float32, AUDIO_S16: np.int16}


def _audio_args(decim, taps, fmt, scale):
    """Pipeline.set_audio: (decim, float32 taps, FDC_AUDIO_* code, float32 scale), (0, None, 0, 1) for decim None.  Raises before any library call."""
    if decim is None:
        return 0, None, AUDIO_F32, np.float32(1.0)
    if isinstance(decim, bool) or not isinstance(decim, (int, np.integer)) or not 1 <= int(decim) <= AUDIO_MAX_DECIM:
        raise ValueError("the audio decimation is an integer in 1 .. %d (None: off)" % AUDIO_MAX_DECIM)
    if taps is None:
        raise ValueError("the audio needs its taps (lowpass_taps)")
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if not 1 <= h.size <= AUDIO_MAX_TAPS:
        raise ValueError("the audio filter has 1 .. %d taps" % AUDIO_MAX_TAPS)
    if not np.isfinite(h).all():
        raise ValueError("the audio taps must be finite (tap %d is not)" % int(np.flatnonzero(~np.isfinite(h))[0]))
    if not isinstance(fmt, str) or fmt.lower() not in _AUDIO_FORMATS:
        raise ValueError("the audio format is 'f32' or 's16'")
    code = _AUDIO_FORMATS[fmt.lower()]
    with np.errstate(over="ignore"):
        sc = np.float32(scale)
    if code == AUDIO_S16 and (not np.isfinite(sc) or sc == 0):
        raise ValueError("the audio scale must be finite and not zero")
    return int(decim), h, code, sc if code == AUDIO_S16 else np.float32(1.0)


def audio_channels(mat, lout, decim):
    """The [nb, A] block-major audio matrix of a call (Pipeline.audio) as one array per channel: channel c owns the lout_c / decim columns from
    sum(lout_i / decim, i < c) on, and its stream is those columns of all rows, row after row."""
    mat = np.asarray(mat)
    per = [int(lo) // int(decim) for lo in lout]
    if mat.ndim != 2 or mat.shape[1] != sum(per):
        raise ValueError("the audio matrix has %d columns, one per audio sample of a block of every channel" % sum(per))
    at = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    return [np.ascontiguousarray(mat[:, at[c]:at[c + 1]]).reshape(-1) for c in range(len(per))]


def _pack_npb(mask, npb):
    """(uint8 mask [nblocks, C], int64 npb [C]) of the packed-audio helpers, checked"""
    mask = np.asarray(mask)
    if mask.ndim != 2:
        raise ValueError("the squelch mask is [nblocks, C]")
    per = np.asarray(npb, dtype=np.int64).reshape(-1)
    if per.size != mask.shape[1] or (per < 0).any():
        raise ValueError("npb is one count of audio samples per block for each of the mask's %d channels" % mask.shape[1])
    return mask != 0, per


def audio_pack_offsets(mask, npb):
    """Where every (block, channel) cell of a call lies in its packed audio (Pipeline.set_audio_packing): mask is the call's squelch mask [nblocks, C],
    npb[c] = lout_c / decim the audio samples of one block of channel c.  A cell weighs mask[m, c] * npb[c]; the cells are ordered row-major (block
    outer, channel inner); off[m, c] is the sum of the weights in front of (m, c), for a closed cell where it would go.  Returns (off int64
    [nblocks, C], count): count is the sum of all weights, the length of the packed array."""
    open_, per = _pack_npb(mask, npb)
    w = (open_ * per[None, :]).reshape(-1)
    end = np.cumsum(w, dtype=np.int64)
    return (end - w).reshape(open_.shape), int(end[-1]) if end.size else 0


def unpack_audio(packed, mask, npb):
    """The packed audio of a call (Pipeline.audio_packed) as one 1-D array per channel: the channel's open blocks in order, mask[:, c].sum() * npb[c]
    samples.  mask: the call's squelch mask [nblocks, C] (Pipeline.squelch), npb[c] = lout_c / decim."""
    packed = np.asarray(packed).reshape(-1)
    open_, per = _pack_npb(mask, npb)
    off, count = audio_pack_offsets(open_, per)
    if packed.size != count:
        raise ValueError("the packed audio has %d samples, the mask's open cells hold %d" % (packed.size, count))
    out = []
    for c in range(per.size):
        rows = np.flatnonzero(open_[:, c])
        idx = off[rows, c][:, None] + np.arange(per[c], dtype=np.int64)[None, :]
        out.append(packed[idx.reshape(-1)])
    return out


def lowpass_taps(decim, ntaps, cutoff=None):
    """A low-pass for decimating a demodulated port (Pipeline.set_demod) by `decim`, 1 .. 64: the taps of Pipeline.set_audio, which runs the filter on
    the device behind the demodulation (GNU Radio's fir_filter_fff). A
    Hamming-windowed sinc of ntaps taps, 1 .. 256, with its cutoff (the -6 dB point) at `cutoff` cycles per input sample (default 0.5 / decim, the
    output rate's Nyquist frequency), designed in float64, normalised to unit DC gain and returned as float32."""
    if isinstance(decim, bool) or not isinstance(decim, (int, np.integer)) or not 1 <= int(decim) <= AUDIO_MAX_DECIM:
        raise ValueError("the audio decimation is an integer in 1 .. %d" % AUDIO_MAX_DECIM)
    if isinstance(ntaps, bool) or not isinstance(ntaps, (int, np.integer)) or not 1 <= int(ntaps) <= AUDIO_MAX_TAPS:
        raise ValueError("ntaps is an integer in 1 .. %d" % AUDIO_MAX_TAPS)
    fc = 0.5 / int(decim) if cutoff is None else float(cutoff)
    if not 0.0 < fc <= 0.5:
        raise ValueError("the cutoff is in (0, 0.5] cycles per sample")
    n = np.arange(int(ntaps), dtype=np.float64) - (int(ntaps) - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * n) * np.hamming(int(ntaps))
    return (h / h.sum()).astype(np.float32)


RESAMPLER_MAX_UP, RESAMPLER_MAX_DOWN, RESAMPLER_MAX_PHASE_TAPS = 64, 128, 256       # include/fdc_amd.h (fdc_pipeline_set_audio_resampler)


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _resampler_ratio(up, down):
    """(up, down) of the audio resampler as ints, checked: 1 .. 64 over 1 .. 128, reduced"""
    if not _is_int(up) or not 1 <= int(up) <= RESAMPLER_MAX_UP:
        raise ValueError("the resampler's interpolation is an integer in 1 .. %d (None: off)" % RESAMPLER_MAX_UP)
    if not _is_int(down) or not 1 <= int(down) <= RESAMPLER_MAX_DOWN:
        raise ValueError("the resampler's decimation is an integer in 1 .. %d" % RESAMPLER_MAX_DOWN)
    g = math.gcd(int(up), int(down))
    if g != 1:
        raise ValueError("the ratio %d / %d is not reduced, which would leave tap phases unused: give %d / %d" % (up, down, int(up) // g, int(down) // g))
    return int(up), int(down)


def _resampler_args(up, down, taps, fmt, scale):
    """Pipeline.set_audio_resampler: (up, down, float32 taps, FDC_AUDIO_* code, float32 scale), (0, 0, None, 0, 1) for up None.  Raises before any
    library call."""
    if up is None:
        return 0, 0, None, AUDIO_F32, np.float32(1.0)
    up, down = _resampler_ratio(up, down)
    if taps is None:
        raise ValueError("the resampler needs its taps (resampler_taps)")
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if h.size < 1 or -(-h.size // up) > RESAMPLER_MAX_PHASE_TAPS:
        raise ValueError("the resampler's filter has 1 .. %d taps per phase: 1 .. %d taps at up = %d" % (RESAMPLER_MAX_PHASE_TAPS, RESAMPLER_MAX_PHASE_TAPS * up, up))
    if not np.isfinite(h).all():
        raise ValueError("the resampler's taps must be finite (tap %d is not)" % int(np.flatnonzero(~np.isfinite(h))[0]))
    if not isinstance(fmt, str) or fmt.lower() not in _AUDIO_FORMATS:
        raise ValueError("the audio format is 'f32' or 's16'")
    code = _AUDIO_FORMATS[fmt.lower()]
    with np.errstate(over="ignore"):
        sc = np.float32(scale)
    if code == AUDIO_S16 and (not np.isfinite(sc) or sc == 0):
        raise ValueError("the audio scale must be finite and not zero")
    return up, down, h, code, sc if code == AUDIO_S16 else np.float32(1.0)


def audio_block_counts(lout, up, down, first_block, nblocks):
    """How many resampled outputs each of the blocks first_block .. first_block + nblocks - 1 of a channel of lout samples per block owns (int64
    [nblocks]): block m owns the outputs ceil(m lout up / down) .. ceil((m + 1) lout up / down) - 1, W or W - 1 of them with W = ceil(lout up / down).
    A function of the ABSOLUTE block index alone, in exact integers (the library's fdc_audio_resampler_counts)."""
    up, down = _resampler_ratio(up, down)
    if not _is_int(lout) or int(lout) < 1:
        raise ValueError("lout is a positive integer")
    if not _is_int(first_block) or int(first_block) < 0 or not _is_int(nblocks) or int(nblocks) < 0:
        raise ValueError("first_block and nblocks are integers >= 0")
    step = int(lout) * up
    edge = [-((-(int(first_block) + i) * step) // down) for i in range(int(nblocks) + 1)]
    return np.array([edge[i + 1] - edge[i] for i in range(int(nblocks))], dtype=np.int64)


def audio_resampled_channels(mat, lout, up, down, first_block):
    """The [nb, A] block-major matrix of a resampled call (Pipeline.audio with set_audio_resampler on) as one array per channel holding the VALID samples
    only: channel c owns the W_c = ceil(lout_c up / down) columns from sum(W_i, i < c) on, row m holds the audio_block_counts(lout_c, ..)[m] outputs
    of block first_block + m and, where that is W_c - 1, one pad behind them, which is dropped here."""
    mat = np.asarray(mat)
    up, down = _resampler_ratio(up, down)
    per = [-(-int(lo) * up // down) for lo in lout]
    if mat.ndim != 2 or mat.shape[1] != sum(per):
        raise ValueError("the audio matrix has %d columns, ceil(lout_c up / down) for every channel" % sum(per))
    at = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    out = []
    for c, lo in enumerate(lout):
        cnt = audio_block_counts(int(lo), up, down, first_block, mat.shape[0])
        cell = mat[:, at[c]:at[c + 1]]
        out.append(np.ascontiguousarray(cell[np.arange(per[c])[None, :] < cnt[:, None]]).reshape(-1))
    return out


def resampler_taps(up, down, taps_per_phase=16, cutoff=None):
    """A prototype low-pass for Pipeline.set_audio_resampler(up, down, ...): a Hamming-windowed sinc of up * taps_per_phase taps with its cutoff (the
    -6 dB point) at `cutoff` cycles per UPSAMPLED sample (default 0.5 / max(up, down): the narrower of the input's and the output's Nyquist
    frequency), designed in float64, its sum normalised to `up` (unit gain through the interpolation) and returned as float32."""
    up, down = _resampler_ratio(up, down)
    if not _is_int(taps_per_phase) or not 1 <= int(taps_per_phase) <= RESAMPLER_MAX_PHASE_TAPS:
        raise ValueError("taps_per_phase is an integer in 1 .. %d" % RESAMPLER_MAX_PHASE_TAPS)
    fc = 0.5 / max(up, down) if cutoff is None else float(cutoff)
    if not 0.0 < fc <= 0.5:
        raise ValueError("the cutoff is in (0, 0.5] cycles per upsampled sample")
    ntaps = up * int(taps_per_phase)
    n = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * n) * np.hamming(ntaps)
    return (h * (up / h.sum())).astype(np.float32)


def audio_resample_ratio(rate_in, rate_out):
    """The exact reduced (up, down) with rate_out = rate_in * up / down, for rates given as integers, fractions.Fraction or floats that are exact
    ratios (25e3, 48000.0); ValueError where up does not fit 1 .. 64 or down 1 .. 128."""
    from fractions import Fraction
    try:
        fin, fout = Fraction(rate_in), Fraction(rate_out)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("the rates are finite numbers")
    if fin <= 0 or fout <= 0:
        raise ValueError("the rates are positive")
    r = fout / fin
    if not 1 <= r.numerator <= RESAMPLER_MAX_UP or not 1 <= r.denominator <= RESAMPLER_MAX_DOWN:
        raise ValueError("%s -> %s is the ratio %d / %d, beyond %d / %d" % (rate_in, rate_out, r.numerator, r.denominator, RESAMPLER_MAX_UP, RESAMPLER_MAX_DOWN))
    return int(r.numerator), int(r.denominator)


TONES_MAX, TONES_MAX_FRAME, TONE_TABLE = 64, 4096, 1024       # include/fdc_amd.h: tones per channel, blocks per frame, entries of the reference table


def _tones_args(nchan, inc, group, frame_blocks):
    """Pipeline.set_tones: (uint32 inc[C, T], S, W), (None, 0, 0) for inc None.  A 1-D inc is one row for all channels.  Raises before any library call."""
    if inc is None:
        return None, 0, 0
    a = np.asarray(inc)
    if a.dtype.kind not in "iu" or a.ndim not in (1, 2):
        raise ValueError("the tone increments are unsigned 32-bit integers, [T] for all channels or [C, T] (tone_increments)")
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError("a tone increment is outside 0 .. 2^32 - 1")
    if a.ndim == 1:
        a = np.broadcast_to(a[None, :], (nchan, a.size))
    if a.shape[0] != nchan:
        raise ValueError("the tone increments have %d rows for %d channels" % (a.shape[0], nchan))
    if not 1 <= a.shape[1] <= TONES_MAX:
        raise ValueError("there are 1 .. %d tones per channel" % TONES_MAX)
    for name, v, hi in (("group length", group, None), ("frame length", frame_blocks, TONES_MAX_FRAME)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1 or (hi is not None and int(v) > hi):
            raise ValueError("the tone %s is an integer of at least 1%s" % (name, "" if hi is None else " and at most %d" % hi))
    return np.ascontiguousarray(a, dtype=np.uint32), int(group), int(frame_blocks)


def tone_table():
    """fdc_tone_table: the 1024 float32 (cos, sin)(2 pi k / 1024) pairs of the tones' reference as the library holds them, [1024, 2]."""
    tab = np.empty((TONE_TABLE, 2), dtype=np.float32)
    _lib.check(_lib.lib().fdc_tone_table(tab.ctypes.data_as(C.POINTER(C.c_float))))
    return tab


def ctcss_tones():
    """The 50 standard CTCSS frequencies in Hz, 67.0 .. 254.1, ascending (float64)."""
    return np.array([67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3,
                     131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8, 196.6,
                     199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1])


def tone_increments(freqs_hz, chan_rate_hz, group):
    """Phase increments for Pipeline.set_tones: round(2^32 f S / r) mod 2^32 as uint32, f in Hz (any shape; negative frequencies wrap), r the channel's
    sample rate in Hz (a scalar, or one value per row of a [C, T] freqs_hz) and S the group length.  |f S / r| must stay at or below 0.5: above it the
    tone aliases at the group rate."""
    f = np.asarray(freqs_hz, dtype=np.float64)
    r = np.asarray(chan_rate_hz, dtype=np.float64)
    if r.ndim == 1 and f.ndim == 2:
        r = r[:, None]
    if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or int(group) < 1:
        raise ValueError("the tone group length is an integer of at least 1")
    if not np.isfinite(f).all() or not np.isfinite(r).all() or (r <= 0).any():
        raise ValueError("the frequencies must be finite and the channel rate positive")
    turns = f * int(group) / r
    if (np.abs(turns) > 0.5).any():
        raise ValueError("a tone lies beyond half the group rate (|f S / r| > 0.5)")
    return (np.rint(turns * 4294967296.0).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def tone_amplitude(Z, frame_samples, freqs_hz, chan_rate_hz, group):
    """The amplitude of a tone at freqs_hz in the demodulated stream from its frame rows Z (Pipeline.tones; the last axis is the tone): |Z| divided by
    frame_samples / 2 (frame_samples = W lout_c, the samples of a frame) and by the boxcar's droop sin(pi f S / r) / (S sin(pi f / r))."""
    f = np.asarray(freqs_hz, dtype=np.float64)
    r = float(chan_rate_hz)
    x = np.pi * f / r
    small = np.abs(np.sin(x)) < 1e-12
    droop = np.where(small, 1.0, np.sin(x * int(group)) / (int(group) * np.where(small, 1.0, np.sin(x))))
    return np.abs(np.asarray(Z)) / (float(frame_samples) / 2.0) / np.abs(droop)


TONE_SQUELCH_MAX_GUARD, TONE_SQUELCH_MAX_HANG = 63, 65535     # include/fdc_amd.h: the guard in tones, the hang count in frames


def tone_squelch_thresholds(amplitude, lout, W, S, f, rate):
    """Thresholds for Pipeline.set_tone_squelch from the AMPLITUDE of the tone in the demodulated stream: the |Z|^2 a tone of that amplitude at f Hz
    gives over a frame of W blocks of lout samples at `rate` Hz with groups of S, that is (amplitude W lout / 2 droop(f))^2 with the droop
    tone_amplitude divides by.  amplitude, lout and f broadcast against each other (one value per channel, or a scalar).  Returns float32."""
    a, lo, fr = np.broadcast_arrays(np.asarray(amplitude, np.float64), np.asarray(lout, np.float64), np.asarray(f, np.float64))
    if not (np.isfinite(a).all() and np.isfinite(fr).all()) or (a < 0).any() or float(rate) <= 0:
        raise ValueError("the amplitude must be finite and not negative, the frequency finite and the rate positive")
    x = np.pi * fr / float(rate)
    small = np.abs(np.sin(x)) < 1e-12
    droop = np.where(small, 1.0, np.sin(x * int(S)) / (int(S) * np.where(small, 1.0, np.sin(x))))
    return ((a * (float(W) * lo / 2.0) * np.abs(droop)) ** 2).astype(np.float32)


def _tone_squelch_args(nchan, tone, open_thr, close_thr, ratio, guard, hang):
    """Pipeline.set_tone_squelch: (int32 tone[C], float32 open[C], float32 close[C], float32 ratio[C], guard, hang), all None / 0 for tone None.  A scalar
    broadcasts to the channels; close_thr None is open_thr.  Raises before any library call (a tone index at or above the tones' T is the library's
    to refuse)."""
    if tone is None:
        return None, None, None, None, 0, 0
    t = np.asarray(tone)
    if t.dtype.kind not in "iu" or t.ndim > 1 or (t.ndim == 1 and t.size != nchan):
        raise ValueError("the selected tones are integers, one per channel (%d) or a scalar: -1 (not tone-gated) or a tone index" % nchan)
    if t.size and (t.min() < -1 or t.max() >= TONES_MAX):
        raise ValueError("a selected tone is outside -1 .. %d" % (TONES_MAX - 1))
    if open_thr is None:
        raise ValueError("the tone squelch needs open thresholds")
    with np.errstate(over="ignore"):            # (a value beyond float32 becomes infinite and is refused below)
        o = np.asarray(open_thr, dtype=np.float32)
        c = o if close_thr is None else np.asarray(close_thr, dtype=np.float32)
        r = np.asarray(ratio, dtype=np.float32)
    for v in (o, c, r):
        if v.ndim > 1 or (v.ndim == 1 and v.size != nchan):
            raise ValueError("the tone squelch's thresholds and ratios are one value per channel (%d) or a scalar" % nchan)
    t = np.ascontiguousarray(np.broadcast_to(t, (nchan,)), dtype=np.int32)
    o, c, r = (np.ascontiguousarray(np.broadcast_to(v, (nchan,))) for v in (o, c, r))
    if not (np.isfinite(o).all() and np.isfinite(c).all() and np.isfinite(r).all()) or (o < 0).any() or (c < 0).any() or (r < 0).any():
        raise ValueError("the tone squelch's thresholds and ratios must be finite and not negative")
    if (c > o).any():
        raise ValueError("a close threshold is above its open threshold (channel %d)" % int(np.flatnonzero(c > o)[0]))
    for name, v, hi in (("guard", guard, TONE_SQUELCH_MAX_GUARD), ("hang count", hang, TONE_SQUELCH_MAX_HANG)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= hi:
            raise ValueError("the tone squelch's %s is an integer in 0 .. %d" % (name, hi))
    return t, o, c, r, int(guard), int(hang)


class Pipeline(_OutputFormat):
    """fdc_pipeline handle: channels = [(f, l, passbw, stopbw), ...]."""
    _last_nb = None        # block count of the last work call that had blocks (levels())
    _call_nb = 0           # ... and of the last work call

    def __init__(self, blocklen, relinvovl, channels, windowtype=WINDOWTYPES.HANN, max_blocks=64,
                 device_id=0, chunk_blocks=0, keep_spectrum=False, flags=None, min_block_launch=None, host_sub_blocks=None):
        self._h = C.c_void_p()
        self.N, self.R = int(blocklen), int(relinvovl)
        self.channels = [(int(f), int(l), float(p), float(s)) for (f, l, p, s) in channels]
        arr = (_lib.fdc_channel * max(1, len(self.channels)))()
        for i, (f, l, p, s) in enumerate(self.channels):
            arr[i].f, arr[i].l, arr[i].passbw, arr[i].stopbw = f, l, p, s
        dflags, dmin, dsub = _default_cfg_fields()
        cfg = _lib.fdc_pipeline_cfg(device_id, self.N, self.R, int(windowtype), len(self.channels), arr,
                                    int(max_blocks), int(chunk_blocks), int(bool(keep_spectrum)),
                                    dflags if flags is None else int(flags), dmin if min_block_launch is None else int(min_block_launch),
                                    dsub if host_sub_blocks is None else int(host_sub_blocks))
        rc = _lib.lib().fdc_pipeline_create(C.byref(cfg), C.byref(self._h))
        if rc == -1:
            raise ValueError(_lib.lib().fdc_last_error().decode())
        _lib.check(rc)
        self.max_blocks = int(max_blocks)
        self.keep_spectrum = bool(keep_spectrum)
        self.ovl = self.N // self.R if self.N >= self.R else 0
        self.H = self.N - self.ovl
        self.lout = [_lib.lib().fdc_pipeline_channel_lout(self._h, c) for c in range(len(self.channels))]

    # -- sizes
    def output_samples(self, nblocks):
        return int(_lib.lib().fdc_pipeline_output_samples(self._h, nblocks))

    def channel_offset(self, c, nblocks):
        return int(_lib.lib().fdc_pipeline_channel_offset(self._h, c, nblocks))

    def set_output_format(self, fmt, scale=1.0):
        """fdc_pipeline_set_output_format: fmt None / "fc32" (complex64, the default), "sc16" or "sc8".  While sc16 / sc8 is set, work*, work_span*
        and work_iq* return int16 / int8 arrays of shape (n, 2), one per channel: each component saturate(rint(y * scale)) of the complex64 value y
        the float output would have (NaN -> 0, +-Inf -> the limits); process_device* take device buffers of that format.  A setting, not a latch:
        it applies from the next call, survives reset(), and does not touch the stream.  UHD's sc16 convention is scale = 32768."""
        code, sc = _oq_format(fmt, scale)
        _lib.check(_lib.lib().fdc_pipeline_set_output_format(self._h, code, float(sc)))
        self._oq, self._oq_scale = code, sc if code else np.float32(1.0)

    def set_fine_tuning(self, nu):
        """fdc_pipeline_set_fine_tuning: nu[c] in cycles per OUTPUT sample of channel c, |nu| < 0.5 (an array of C doubles, one per channel), or None /
        all zeros to switch it off.  While it is on, sample t of channel c's stream (counted from the last reset()) comes out times
        exp(-2j pi frac(inc_c t / 2**64)), inc_c = fine_tuning_increment(nu[c]): a carrier nu_c above the slice centre lands at DC.  A setting like
        set_output_format: it applies from the next call and survives reset(); the sink, spectrum-item, group-power and waterfall entries are
        refused while it is on.  ValueError for a wrong count, NaN or |nu| >= 0.5 (nothing changes)."""
        _set_fine_tuning(_lib.lib().fdc_pipeline_set_fine_tuning, self._h, len(self.channels), nu)

    def set_levels(self, on=True):
        """fdc_pipeline_set_levels: with levels on, every call also sums, on the device, power = sum(re^2 + im^2) and peak = max(|re|, |im|) of each
        (block, channel) row of the complex64 samples it writes — after fine tuning, before the sc16 / sc8 narrowing, so peak * |scale| >= 32767.5
        (127.5) says a row saturated.  A setting like set_output_format: it applies from the next call and survives reset(); the sink,
        spectrum-item, group-power and waterfall entries are refused while it is on."""
        _lib.check(_lib.lib().fdc_pipeline_set_levels(self._h, int(bool(on))))

    def levels(self, nblocks=None):
        """fdc_pipeline_levels: float32[nblocks of the last call, C, 2], [m, c] = (power, peak) of block m of channel c.  nblocks: the last call's
        block count where it did not go through this object's work methods (process_device, work_raw)."""
        return _levels(_lib.lib().fdc_pipeline_levels, self._h, len(self.channels), self._last_nb, nblocks)

    def set_gains(self, g):
        """fdc_pipeline_set_gains: g[c] (converted to float32, any finite value: zero mutes, negative inverts) multiplies every sample of channel c's
        stream on the device, each component rounded once: (y.view(float32) * g).view(complex64) of what the call writes with gains off.  Order: cut,
        fine tuning, gain, levels, sc16 / sc8 narrowing — the levels are those of the gained samples, integer output is oq(gained * scale).  None, or
        all ones, switches it off.  A setting like set_output_format: it applies from the next call and survives reset(); the sink, spectrum-item,
        group-power and waterfall entries are refused while it is on.  ValueError for a wrong count, NaN or Inf (nothing changes)."""
        _set_gains(_lib.lib().fdc_pipeline_set_gains, self._h, len(self.channels), g)

    def gains(self):
        """fdc_pipeline_gains: the gains in force, float32[C] (ones while off)."""
        out = np.empty(len(self.channels), dtype=np.float32)
        _lib.check(_lib.lib().fdc_pipeline_gains(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), int(out.size)))
        return out

    def levels_device(self):
        """fdc_pipeline_levels_device: the device address of the levels ([block][C] float2), None while levels are off."""
        return _lib.lib().fdc_pipeline_levels_device(self._h)

    def set_lag1(self, on=True):
        """fdc_pipeline_set_lag1: with it on, every call also sums, on the device, S = sum_j y[j] conj(y[j - 1]) over the samples of each (block,
        channel) row of the complex64 samples it writes — after fine tuning and the gain, before the sc16 / sc8 narrowing; the product across the
        block boundary is not taken.  lag1_frequency(S) is the row's mean frequency in the unit of set_fine_tuning (the measurement of an AFC).  A
        setting like set_levels: it applies from the next call and survives reset(); the sink, spectrum-item, group-power and waterfall entries are
        refused while it is on."""
        _lib.check(_lib.lib().fdc_pipeline_set_lag1(self._h, int(bool(on))))

    def lag1(self, nblocks=None):
        """fdc_pipeline_lag1: complex64[nblocks of the last call, C], [m, c] = S of block m of channel c.  nblocks: the last call's block count
        where it did not go through this object's work methods (process_device, work_raw)."""
        return _lag1(_lib.lib().fdc_pipeline_lag1, self._h, len(self.channels), self._last_nb, nblocks)

    def lag1_device(self):
        """fdc_pipeline_lag1_device: the device address of the lag-1 correlation ([block][C] float2), None while it is off."""
        return _lib.lib().fdc_pipeline_lag1_device(self._h)

    def set_demod(self, mode, gain=1.0):
        """fdc_pipeline_set_demod: mode None (off), "fm" or "mag"; gain (converted to float32) finite and not zero.  While it is on, work*, work_span*
        and work_iq* return float32 arrays of nblocks*lout_c samples, one per channel, and process_device* take device buffers of 4-byte samples:
        "fm": gain * atan2 of y[t] conj(y[t - 1]) (the FM discriminator; gain = 1 / (2 pi) gives cycles per output sample, the unit of
        set_fine_tuning and lag1_frequency), "mag": gain * |y[t]| (bit for bit numpy's float32 statement), y the complex64 sample the call writes
        with it off, after fine tuning and the gain.  FM's sample in front of a call's first is the last one of the call before where the call goes on
        at the next block, zero at a stream start (after create, reset(), a switch of mode, a device or span call elsewhere in the stream).  A setting
        like set_output_format: it applies from the next call and survives reset(); it excludes sc16 / sc8 output, and the sink, spectrum-item,
        group-power and waterfall entries are refused while it is on.  ValueError for an unknown mode or a gain that is zero or not finite, FdcError
        where the library refuses (integer output set, a pipelined sinks batch inside); nothing changes then."""
        code, g = _demod_mode(mode, gain)
        _lib.check(_lib.lib().fdc_pipeline_set_demod(self._h, code, float(g)))
        self._demod = code

    def demod_device(self, mode, gain, d_in, d_out, nblocks, d_carry_in=None, d_carry_out=None, stream=None):
        """fdc_pipeline_demod_device: the demodulating pass alone on device buffers of the caller (d_in: complex64 in process_device's layout, d_out:
        float32 at the same element offsets; "fm": d_carry_in, C complex64 or None, is read and d_carry_out, C complex64, written).  The handle's
        own setting, carry and stream position are not touched."""
        code, g = _demod_mode(mode, gain)
        if code == 0:
            raise ValueError("demod_device takes 'fm' or 'mag'")
        _lib.check(_lib.lib().fdc_pipeline_demod_device(self._h, code, float(g), d_in, d_out, d_carry_in, d_carry_out, int(nblocks), stream))

    def demod(self):
        """fdc_pipeline_demod: (mode, gain) in force: (None, 1.0), ("fm", g) or ("mag", g)."""
        mode, gain = C.c_int32(0), C.c_float(0)
        _lib.check(_lib.lib().fdc_pipeline_demod(self._h, C.byref(mode), C.byref(gain)))
        return ({0: None, DEMOD_FM: "fm", DEMOD_MAG: "mag"}[mode.value], float(gain.value))

    _audio = 0             # the decimation set_audio switched on (0: off): the early refusal of outs= only; sizes are asked of the library at every call

    def set_audio(self, decim, taps=None, fmt="f32", scale=1.0):
        """fdc_pipeline_set_audio: decim None switches it off; else decim 1 .. 64 that divides every lout_c, taps (converted to float32; 1 .. 256,
        finite; lowpass_taps), fmt "f32" or "s16", scale (s16 only) finite and not zero.  It needs the demodulation (set_demod) and runs behind it, on
        the device: a[n] = sum over k of taps[k] d[n decim - k] in float32, k ascending from +0, every product and sum rounded on its own; "s16":
        saturate(rint(a * scale)) as int16 (NaN -> 0).  While it is on, work*, work_span* and work_iq* return one AUDIO array per channel, nblocks *
        lout_c / decim samples of float32 or int16, and take no outs=; process_device* write the demodulated ports as before and the audio is fetched
        with audio() or read at audio_device().  The K - 1 demodulated samples in front of a call's first are the tail of the call before where the
        call goes on at the next block, zeros at a stream start (after create, reset(), a new decim or taps, a switch of demodulation mode, a device
        or span call elsewhere in the stream); a new fmt, scale or demodulation gain keeps them.  A setting like set_demod: it applies from the next
        call and survives reset().  ValueError for arguments out of range (nothing reaches the library), FdcError where the library refuses
        (demodulation off, decim does not divide a channel's lout, a pipelined sinks batch inside); nothing changes then."""
        d, h, code, sc = _audio_args(decim, taps, fmt, scale)
        _lib.check(_lib.lib().fdc_pipeline_set_audio(self._h, d, None if h is None else h.ctypes.data_as(C.POINTER(C.c_float)), 0 if h is None else int(h.size),
                                                     code, float(sc)))
        self._audio = d

    def set_audio_resampler(self, up, down=None, taps=None, fmt="f32", scale=1.0):
        """fdc_pipeline_set_audio_resampler: up None switches it off; else the reduced ratio up 1 .. 64 over down 1 .. 128, taps (converted to float32;
        finite, at most 256 per phase: resampler_taps), fmt and scale as set_audio.  The second form of the channel audio, which replaces the decimating
        one (and set_audio(decim) replaces it): a[n] = sum over k of taps[k up + (n down mod up)] d[(n down div up) - k] with n and the sample index
        counted from the stream's block 0, in set_audio's arithmetic (tests/resample_model.py).  While it is on, work*, work_span* and work_iq* return
        one array per channel with the VALID samples of the call (audio_block_counts says how many each block gives) and take no outs=; audio() gives
        the padded matrix [nblocks, sum of ceil(lout_c up / down)] (audio_resampled_channels slices it).  The history is set_audio's, of
        ceil(ntaps / up) - 1 samples per channel; a new ratio or other taps restart the stream.  ValueError for arguments out of range (nothing
        reaches the library), FdcError where the library refuses (demodulation off, the audio packing on, a pipelined sinks batch inside)."""
        u, d, h, code, sc = _resampler_args(up, down, taps, fmt, scale)
        _lib.check(_lib.lib().fdc_pipeline_set_audio_resampler(self._h, u, d, None if h is None else h.ctypes.data_as(C.POINTER(C.c_float)),
                                                               0 if h is None else int(h.size), code, float(sc)))
        self._audio = u if u else (0 if self.audio_setting() is None else self._audio)

    def audio_resampler_setting(self):
        """fdc_pipeline_audio_resampler_setting: None while off, else (up, down, float32 taps, "f32" / "s16", scale): what the library has in force now."""
        u, d, k, f, sc = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_float(0)
        lib = _lib.lib()
        _lib.check(lib.fdc_pipeline_audio_resampler_setting(self._h, C.byref(u), C.byref(d), C.byref(k), C.byref(f), C.byref(sc), None, 0))
        if u.value == 0:
            return None
        taps = np.zeros(k.value, dtype=np.float32)
        _lib.check(lib.fdc_pipeline_audio_resampler_setting(self._h, None, None, None, None, None, taps.ctypes.data_as(C.POINTER(C.c_float)), int(taps.size)))
        return int(u.value), int(d.value), taps, {AUDIO_F32: "f32", AUDIO_S16: "s16"}[f.value], float(sc.value)

    def audio_first_block(self):
        """fdc_pipeline_audio_first_block: the absolute index of row 0 of the audio the handle holds, -1 where there is none."""
        return int(_lib.lib().fdc_pipeline_audio_first_block(self._h))

    def audio_resampler_pass_device(self, d_in, d_out, first_block, nblocks, d_hist_in=None, d_hist_out=None, d_mask=None, stream=None):
        """fdc_pipeline_audio_resampler_pass_device: the resampling pass alone on device buffers of the caller, with the setting in force (d_in: float32
        in process_device's layout, d_out: nblocks * A elements, d_hist_in: C (Kp - 1) float32 or None, d_hist_out: another such buffer, None only
        where Kp = 1, d_mask: nblocks * C bytes or None).  The handle's own history and stream position are not touched."""
        _lib.check(_lib.lib().fdc_pipeline_audio_resampler_pass_device(self._h, d_in, d_out, d_hist_in, d_hist_out, int(first_block), int(nblocks), d_mask, stream))

    def _audio_form(self):
        """the audio form in force, asked of the library: None, ("decim", decim, fmt) or ("resampled", up, down, fmt)"""
        s = self.audio_setting()
        if s is not None:
            return ("decim", s[0], s[2])
        r = self.audio_resampler_setting()
        return None if r is None else ("resampled", r[0], r[1], r[3])

    def audio_setting(self):
        """fdc_pipeline_audio_setting: None while off, else (decim, float32 taps, "f32" / "s16", scale): what the library has in force now."""
        d, k, f, sc = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_float(0)
        taps = np.zeros(AUDIO_MAX_TAPS, dtype=np.float32)
        _lib.check(_lib.lib().fdc_pipeline_audio_setting(self._h, C.byref(d), C.byref(k), C.byref(f), C.byref(sc), taps.ctypes.data_as(C.POINTER(C.c_float))))
        if d.value == 0:
            return None
        return int(d.value), taps[:k.value].copy(), {AUDIO_F32: "f32", AUDIO_S16: "s16"}[f.value], float(sc.value)

    def audio(self, nblocks=None):
        """fdc_pipeline_audio: the audio of the last call, [nblocks, A] float32 or int16, A = sum of lout_c / decim: row m is block m of the call, channel
        c its columns from sum(lout_i / decim, i < c) on (audio_channels slices it).  nblocks: the last call's block count where it did not go
        through this object's work methods (process_device, work_raw).  The array is sized from what the library says its setting is now, and the
        library is told that size."""
        if nblocks is None:
            if self._last_nb is None:
                raise ValueError("audio(): no work call yet")
            nblocks = self._last_nb
        nblocks = int(nblocks)
        if nblocks < 0:
            raise ValueError("audio(): negative block count")
        if getattr(self, "_packing", False):
            raise ValueError("audio(): the audio packing is on, there is no matrix: audio_packed() (set_audio_packing)")
        form = self._audio_form()
        if form is None:
            raise ValueError("audio(): the channel audio is off (set_audio, set_audio_resampler)")
        out = np.empty((nblocks, int(_lib.lib().fdc_pipeline_audio_row(self._h))), dtype=_AUDIO_DTYPES[_AUDIO_FORMATS[form[-1]]])
        if out.size:
            _lib.check(_lib.lib().fdc_pipeline_audio(self._h, out.ctypes.data, out.nbytes, nblocks))
        return out

    def audio_device(self):
        """fdc_pipeline_audio_device: the device address of the audio ([block of the last call][A] float32 / int16), None while it is off."""
        return _lib.lib().fdc_pipeline_audio_device(self._h)

    def audio_pass_device(self, d_in, d_out, nblocks, d_hist_in=None, d_hist_out=None, stream=None):
        """fdc_pipeline_audio_pass_device: the audio pass alone on device buffers of the caller, with the setting in force (d_in: float32 in
        process_device's layout, d_out: nblocks * A elements, d_hist_in: C (K - 1) float32 or None, d_hist_out: another such buffer, None only where
        K = 1).  The handle's own history and stream position are not touched."""
        _lib.check(_lib.lib().fdc_pipeline_audio_pass_device(self._h, d_in, d_out, d_hist_in, d_hist_out, int(nblocks), stream))

    def set_audio_packing(self, on):
        """fdc_pipeline_set_audio_packing: with the channel audio (set_audio) and the squelch (set_squelch) on, only the audio of open (block, channel)
        cells leaves the device: audio_packed() gives them one behind the other, block-major (tests/audio_pack_model.py), squelch() the mask that says
        whose they are, and the work methods return one array per channel with its open blocks (unpack_audio).  audio() raises while it is on.  A
        setting: it applies from the next call and survives reset(); the packing carries no state from call to call.  FdcError where the library
        refuses (audio or squelch off, a pipelined sinks batch inside); nothing changes then.  At full occupancy it costs a second synchronise per
        host call and saves nothing: leave it off on a band whose channels are mostly open."""
        if not isinstance(on, (bool, np.bool_, int, np.integer)):
            raise ValueError("set_audio_packing(on): on is a bool")
        _lib.check(_lib.lib().fdc_pipeline_set_audio_packing(self._h, 1 if on else 0))
        self._packing = bool(on)

    def audio_packing(self):
        """fdc_pipeline_audio_packing: whether the library has the packing on now."""
        return _lib.lib().fdc_pipeline_audio_packing(self._h) == 1

    def audio_packed(self, nblocks=None):
        """fdc_pipeline_audio_packed: the packed audio of the last call, a 1-D array of `count` float32 or int16 (the audio setting's format): the
        samples of the open (block, channel) cells in block-major order (unpack_audio slices it by squelch()).  nblocks: the last call's block count
        where it did not go through this object's work methods.  The library is asked for the count first and told the array's size."""
        if nblocks is None:
            if self._last_nb is None:
                raise ValueError("audio_packed(): no work call yet")
            nblocks = self._last_nb
        nblocks = int(nblocks)
        if nblocks < 0:
            raise ValueError("audio_packed(): negative block count")
        if not getattr(self, "_packing", False):
            raise ValueError("audio_packed(): the audio packing is off (set_audio_packing)")
        setting = self.audio_setting()
        if setting is None:
            raise ValueError("audio_packed(): the channel audio is off (set_audio)")
        if nblocks == 0 or not self.channels:          # (nothing was packed: the library keeps no call of no blocks)
            return np.empty(0, dtype=_AUDIO_DTYPES[_AUDIO_FORMATS[setting[2]]])
        count = C.c_int64(0)
        _lib.check(_lib.lib().fdc_pipeline_audio_packed(self._h, None, 0, nblocks, C.byref(count)))
        out = np.empty(int(count.value), dtype=_AUDIO_DTYPES[_AUDIO_FORMATS[setting[2]]])
        if out.size:
            _lib.check(_lib.lib().fdc_pipeline_audio_packed(self._h, out.ctypes.data, out.nbytes, nblocks, C.byref(count)))
        return out

    def audio_pack_offsets_device(self, d_mask, d_off, d_total_out, nblocks, d_base_in=None, stream=None):
        """fdc_pipeline_audio_pack_offsets_device: the packed audio's offsets alone on device buffers of the caller, with the handle's channel table and
        the audio's decimation (d_mask: nblocks * C bytes, d_off: nblocks * C uint32, d_total_out: one int64, d_base_in: one int64 added to every
        offset and the total, or None).  Nothing of the handle's state is read or written."""
        _lib.check(_lib.lib().fdc_pipeline_audio_pack_offsets_device(self._h, d_mask, d_base_in, d_off, d_total_out, int(nblocks), stream))

    def set_squelch(self, open_thr, close_thr=None, hang=0):
        """fdc_pipeline_set_squelch: open_thr None switches it off; else thresholds in the levels' unit (the sum over a row of re^2 + im^2 in front of
        the channel gain; squelch_thresholds converts from dB of mean power), one per channel or a scalar for all, close_thr (default: open_thr) not
        above open_thr, both finite and >= 0, and hang 0 .. 65535 blocks.  It needs the levels (set_levels) and decides on them, on the device: a
        channel opens at a block whose power reaches open_thr, stays open while it reaches close_thr, and closes at the (hang + 1)-th consecutive
        block below (tests/squelch_model.py).  squelch() gives the mask of the last call; with the audio on (set_audio) the audio of closed blocks is
        zero and is not filtered.  The state of every channel is kept on the device from call to call and starts closed after create, reset(),
        switching it on, or a device or span call elsewhere in the stream; new thresholds or a new hang keep which channels are open.  A setting: it
        applies from the next call and survives reset().  ValueError for arguments out of range (nothing reaches the library), FdcError where the
        library refuses (levels off, a pipelined sinks batch inside); nothing changes then."""
        o, c, h = _squelch_args(len(self.channels), open_thr, close_thr, hang)
        if o is not None and o.size == 0:         # (a plan without channels: pointers that are not NULL, which means off)
            o = c = np.zeros(1, np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(_lib.lib().fdc_pipeline_set_squelch(self._h, None if o is None else o.ctypes.data_as(fp), None if c is None else c.ctypes.data_as(fp),
                                                       len(self.channels), h))

    def squelch_setting(self):
        """fdc_pipeline_squelch_setting: None while off, else (float32 open[C], float32 close[C], hang): what the library has in force now."""
        hang = C.c_int32(0)
        _lib.check(_lib.lib().fdc_pipeline_squelch_setting(self._h, None, None, C.byref(hang)))
        if hang.value < 0:
            return None
        o, c = np.zeros(max(1, len(self.channels)), np.float32), np.zeros(max(1, len(self.channels)), np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(_lib.lib().fdc_pipeline_squelch_setting(self._h, o.ctypes.data_as(fp), c.ctypes.data_as(fp), None))
        return o[:len(self.channels)], c[:len(self.channels)], int(hang.value)

    def squelch(self, nblocks=None):
        """fdc_pipeline_squelch: the mask of the last call, uint8 [nblocks, C]: 1 where the channel is open at that block.  nblocks: the last call's
        block count where it did not go through this object's work methods (process_device, work_raw)."""
        if nblocks is None:
            if self._last_nb is None:
                raise ValueError("squelch(): no work call yet")
            nblocks = self._last_nb
        nblocks = int(nblocks)
        if nblocks < 0:
            raise ValueError("squelch(): negative block count")
        if self.squelch_setting() is None:
            raise ValueError("squelch(): the channel squelch is off (set_squelch)")
        out = np.empty((nblocks, len(self.channels)), dtype=np.uint8)
        if out.size:
            _lib.check(_lib.lib().fdc_pipeline_squelch(self._h, out.ctypes.data, out.nbytes, nblocks))
        return out

    def squelch_device(self):
        """fdc_pipeline_squelch_device: the device address of the mask ([block of the last call][C] bytes), None while it is off."""
        return _lib.lib().fdc_pipeline_squelch_device(self._h)

    def squelch_pass_device(self, d_levels, d_mask, nblocks, d_state_in=None, d_state_out=None, stream=None):
        """fdc_pipeline_squelch_pass_device: the decision alone on device buffers of the caller, with the setting and the gains in force (d_levels:
        [nblocks][C] float32 pairs, d_mask: nblocks * C bytes, d_state_in: C int32 pairs (open, h) or None, d_state_out: another such buffer).  The
        handle's own state and stream position are not touched."""
        _lib.check(_lib.lib().fdc_pipeline_squelch_pass_device(self._h, d_levels, d_mask, d_state_in, d_state_out, int(nblocks), stream))

    def set_tones(self, inc, group=16, frame_blocks=32):
        """fdc_pipeline_set_tones: inc None switches it off; else uint32 phase increments [C, T] (or [T] for all channels; tone_increments), T 1 .. 64,
        a group length that divides every lout_c and a frame length of 1 .. 4096 blocks.  It needs the demodulation (set_demod) and runs behind it, on
        the device: per channel and tone a correlator over the sums of `group` consecutive demodulated samples, integrated over frame_blocks blocks
        (tests/tones_model.py); tones() gives the frame rows the last call completed.  The open frame is kept on the device from call to call and
        starts anew after create, reset(), a new setting, a switch of demodulation mode, or a device or span call elsewhere in the stream; a new
        demodulation gain keeps it.  A setting: it applies from the next call and survives reset().  ValueError for arguments out of range (nothing
        reaches the library), FdcError where the library refuses (demodulation off, group does not divide a channel's lout, a pipelined sinks
        batch inside); nothing changes then."""
        a, s, w = _tones_args(len(self.channels), inc, group, frame_blocks)
        if a is not None and a.size == 0:         # (a plan without channels: a pointer that is not NULL, which means off)
            a = np.zeros((1, a.shape[1]), np.uint32)
        _lib.check(_lib.lib().fdc_pipeline_set_tones(self._h, None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32)), len(self.channels),
                                                     0 if a is None else int(a.shape[1]), s, w))

    def tones_setting(self):
        """fdc_pipeline_tones_setting: None while off, else (uint32 inc[C, T], group, frame_blocks): what the library has in force now."""
        t, s, w = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.lib().fdc_pipeline_tones_setting(self._h, C.byref(t), C.byref(s), C.byref(w), None))
        if t.value == 0:
            return None
        inc = np.zeros((max(1, len(self.channels)), t.value), dtype=np.uint32)
        _lib.check(_lib.lib().fdc_pipeline_tones_setting(self._h, None, None, None, inc.ctypes.data_as(C.POINTER(C.c_uint32))))
        return inc[:len(self.channels)], int(s.value), int(w.value)

    def tones(self, nblocks=None):
        """fdc_pipeline_tones: the frame rows the last call completed, complex64 [nf, C, T] (nf may be 0: the call ended inside a frame).  nblocks: the
        last call's block count where it did not go through this object's work methods (process_device, work_raw)."""
        if nblocks is None:
            if self._last_nb is None:
                raise ValueError("tones(): no work call yet")
            nblocks = self._last_nb
        nblocks = int(nblocks)
        if nblocks < 0:
            raise ValueError("tones(): negative block count")
        setting = self.tones_setting()
        if setting is None:
            raise ValueError("tones(): the channel tones are off (set_tones)")
        inc, _, w = setting
        out = np.empty(((nblocks + w - 1) // w, len(self.channels), inc.shape[1]), dtype=np.complex64)     # (the most a call of nblocks can complete)
        nf = C.c_int32(0)
        if nblocks:
            _lib.check(_lib.lib().fdc_pipeline_tones(self._h, out.ctypes.data, out.nbytes, nblocks, C.byref(nf)))
        return out[:nf.value].copy()

    def tones_device(self):
        """fdc_pipeline_tones_device: the device address of the frame rows ([frame of the last call][C][T] float32 pairs), None while it is off."""
        return _lib.lib().fdc_pipeline_tones_device(self._h)

    def tones_pass_device(self, d_in, d_frames, nblocks, first_block=0, fill=0, d_carry_in=None, d_carry_out=None, stream=None):
        """fdc_pipeline_tones_pass_device: the tones pass alone on device buffers of the caller, with the setting in force (d_in: float32 in
        process_device's layout, blocks first_block .. of a stream with `fill` blocks already in the open frame; d_frames: ((fill + nblocks) // W) C T
        float32 pairs; d_carry_in: C T pairs or None, d_carry_out: another such buffer).  The handle's own state and stream position are not touched."""
        _lib.check(_lib.lib().fdc_pipeline_tones_pass_device(self._h, d_in, d_frames, d_carry_in, d_carry_out, int(first_block), int(fill), int(nblocks), stream))

    def set_tone_squelch(self, tone, open_thr=None, close_thr=None, ratio=0.0, guard=0, hang=0):
        """fdc_pipeline_set_tone_squelch: tone None switches it off; else per channel (or a scalar for all) the index of the selected tone among the
        tones' T (-1: the channel is not tone-gated), thresholds on |Z|^2 of that tone's frame rows (tone_squelch_thresholds converts from an
        amplitude), close_thr (default: open_thr) not above open_thr, and a ratio the selected tone must keep over the strongest tone more than
        `guard` places away; hang 0 .. 65535 FRAMES.  It needs the tones (set_tones) and the squelch (set_squelch) and decides on the device, per
        completed frame, by the squelch's own state machine (tests/tone_squelch_model.py); the decision of the frame BEFORE gates the carrier mask, so
        squelch(), the gated audio and the packed audio see carrier AND tone.  tone_squelch() gives the decisions of the frames the last call
        completed.  The state goes on exactly where the tones' stream does; a new setting restarts it.  A setting: it applies from the next call and
        survives reset().  ValueError for arguments out of range (nothing reaches the library), FdcError where the library refuses (tones or squelch
        off, a tone index at or above T, a pipelined sinks batch inside); nothing changes then."""
        t, o, c, r, g, h = _tone_squelch_args(len(self.channels), tone, open_thr, close_thr, ratio, guard, hang)
        if t is not None and t.size == 0:         # (a plan without channels: pointers that are not NULL, which means off)
            t, o = np.zeros(1, np.int32), np.zeros(1, np.float32)
            c = r = o
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        if t is None:
            _lib.check(_lib.lib().fdc_pipeline_set_tone_squelch(self._h, None, None, None, None, len(self.channels), 0, 0))
        else:
            _lib.check(_lib.lib().fdc_pipeline_set_tone_squelch(self._h, t.ctypes.data_as(ip), o.ctypes.data_as(fp), c.ctypes.data_as(fp), r.ctypes.data_as(fp),
                                                                len(self.channels), g, h))

    def tone_squelch_setting(self):
        """fdc_pipeline_tone_squelch_setting: None while off, else (int32 tone[C], float32 open[C], float32 close[C], float32 ratio[C], guard, hang):
        what the library has in force now."""
        g, h = C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.lib().fdc_pipeline_tone_squelch_setting(self._h, None, None, None, None, C.byref(g), C.byref(h)))
        if h.value < 0:
            return None
        n = len(self.channels)
        t, o, c, r = np.zeros(max(1, n), np.int32), np.zeros(max(1, n), np.float32), np.zeros(max(1, n), np.float32), np.zeros(max(1, n), np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(_lib.lib().fdc_pipeline_tone_squelch_setting(self._h, t.ctypes.data_as(C.POINTER(C.c_int32)), o.ctypes.data_as(fp), c.ctypes.data_as(fp),
                                                                r.ctypes.data_as(fp), None, None))
        return t[:n], o[:n], c[:n], r[:n], int(g.value), int(h.value)

    def tone_squelch(self, nblocks=None):
        """fdc_pipeline_tone_squelch: the decisions of the frames the last call completed, uint8 [nf, C]: 1 where the channel's tone squelch is open
        behind that frame (nf may be 0).  nblocks: the last call's block count where it did not go through this object's work methods."""
        if nblocks is None:
            if self._last_nb is None:
                raise ValueError("tone_squelch(): no work call yet")
            nblocks = self._last_nb
        nblocks = int(nblocks)
        if nblocks < 0:
            raise ValueError("tone_squelch(): negative block count")
        if self.tone_squelch_setting() is None:
            raise ValueError("tone_squelch(): the tone squelch is off (set_tone_squelch)")
        w = self.tones_setting()[2]
        out = np.empty(((nblocks + w - 1) // w, len(self.channels)), dtype=np.uint8)       # (the most a call of nblocks can complete)
        nf = C.c_int32(0)
        if nblocks:
            _lib.check(_lib.lib().fdc_pipeline_tone_squelch(self._h, out.ctypes.data, out.nbytes, nblocks, C.byref(nf)))
        return out[:nf.value].copy()

    def tone_squelch_device(self):
        """fdc_pipeline_tone_squelch_device: the device address of the decisions ([frame of the last call][C] bytes), None while it is off."""
        return _lib.lib().fdc_pipeline_tone_squelch_device(self._h)

    def tone_squelch_pass_device(self, d_frames, d_dec, nblocks, fill=0, d_state_in=None, d_state_out=None, d_mask=None, stream=None):
        """fdc_pipeline_tone_squelch_pass_device: the decision and the gate alone on device buffers of the caller, with the setting in force (d_frames:
        ((fill + nblocks) // W) C T float32 pairs, d_dec: that many times C bytes, d_state_in: C int32 pairs (open, h) or None, d_state_out: another such
        buffer, d_mask: nblocks C bytes ANDed in place, or None for the decision alone).  The handle's own state is not touched."""
        _lib.check(_lib.lib().fdc_pipeline_tone_squelch_pass_device(self._h, d_frames, d_dec, d_state_in, d_state_out, d_mask, int(fill), int(nblocks), stream))

    def _host_outs(self, outs, nb):
        """(outs, ptrs) of a host call.  While the channel audio is on — asked of the library at this call — the entries write no port: (None, None),
        and outs= is refused."""
        if outs is not None and getattr(self, "_audio", 0):
            raise ValueError("outs= cannot go with the channel audio: the call returns the audio arrays (set_audio)")
        if getattr(self, "_h", None) and self._audio_form() is not None:
            if outs is not None:
                raise ValueError("outs= cannot go with the channel audio: the call returns the audio arrays (set_audio)")
            return None, None
        outs = self._check_outs(outs, nb)
        return outs, (C.c_void_p * max(1, len(outs)))(*[o.ctypes.data for o in outs])

    def _host_results(self, outs, nb):
        """what a host call returns: its outs, or (the audio on: _host_outs gave None) one audio array per channel, sliced from the matrix"""
        if outs is not None:
            return outs
        form = self._audio_form()
        if form[0] == "resampled":
            # the valid samples only: the rows are cut by the counts at the call's first block, as the library reports it
            first = self.audio_first_block()
            return audio_resampled_channels(self.audio(nb), self.lout, form[1], form[2], max(first, 0))
        decim = form[1]
        if getattr(self, "_packing", False):
            # the packing on: one array per channel with its open blocks of this call; which they are: squelch()
            per = [int(lo) // decim for lo in self.lout]
            if nb <= 0:
                return unpack_audio(np.empty(0, _AUDIO_DTYPES[_AUDIO_FORMATS[self.audio_setting()[2]]]), np.zeros((0, len(per)), np.uint8), per)
            return unpack_audio(self.audio_packed(nb), self.squelch(nb), per)
        return audio_channels(self.audio(nb), self.lout, decim)

    def _ran(self, nb):
        self._call_nb = int(nb)
        if nb > 0:
            self._last_nb = int(nb)

    # -- host path (what sync_block::work() would call)
    def work(self, x, want_spectrum=False, sinks=None, outs=None):
        """sinks: a gr_fdc_amd.Sinks bank fed from the device-resident spectrum of this call (needs keep_spectrum).
        outs: optional caller-owned arrays, one per channel with nblocks*lout_c samples of the output format (complex64 unless
        set_output_format chose sc16 / sc8; e.g. slices of buffers pinned with register_host); allocated here when None."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if x.size % self.H:
            raise ValueError("input must be a whole number of (N - N/R)-sample items")
        nb = x.size // self.H
        outs, ptrs = self._host_outs(outs, nb)
        spec = np.empty(nb * self.N, dtype=np.complex64) if want_spectrum else None
        if sinks is not None:
            _lib.check(_lib.lib().fdc_pipeline_work_sinks(self._h, x.ctypes.data, nb, ptrs,
                                                         spec.ctypes.data if spec is not None else None, sinks._h))
        else:
            _lib.check(_lib.lib().fdc_pipeline_work(self._h, x.ctypes.data, nb, ptrs,
                                                   spec.ctypes.data if spec is not None else None))
        self._ran(nb)
        outs = self._host_results(outs, nb)
        return (outs, spec) if want_spectrum else outs

    def work_waterfall(self, x, waterfall):
        """fdc_pipeline_work_waterfall: the channel outputs as work(), and the gr_fdc_amd.Waterfall rows this call finished (Rows of
        mean power, colour index and RGB per pixel).  N = 4096 in one launch stays in one launch (path 5)."""
        from .waterfall import Rows, WIDTH
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if x.size % self.H:
            raise ValueError("input must be a whole number of (N - N/R)-sample items")
        nb = x.size // self.H
        outs = [np.empty(nb * lo, dtype=np.complex64) for lo in self.lout]
        ptrs = (C.c_void_p * max(1, len(outs)))(*[o.ctypes.data for o in outs])
        cap = waterfall.rows_for(nb)
        rows, idx, rgb = np.empty((cap, WIDTH), np.float32), np.empty((cap, WIDTH), np.uint16), np.empty((cap, WIDTH, 3), np.uint8)
        n = C.c_int32(0)
        _lib.check(_lib.lib().fdc_pipeline_work_waterfall(self._h, waterfall._h, x.ctypes.data, nb, ptrs, rows.ctypes.data, idx.ctypes.data,
                                                          rgb.ctypes.data, cap, C.byref(n)))
        return outs, Rows(rows[:n.value], idx[:n.value], rgb[:n.value])

    def flush_sinks(self, sinks):
        """fdc_pipeline_flush_sinks: the pipelined form (a bank made with lookahead=True) hands out the oldest batch still inside;
        returns its block count, 0 when nothing is left.  The PDUs are then the bank's current ones (sinks.pdus())."""
        return _lib.check(_lib.lib().fdc_pipeline_flush_sinks(self._h, sinks._h))

    def sinks_latency(self, sinks):
        """Calls between an item going in and its PDUs coming out of work(..., sinks=sinks): 0 serial, 1 or 2 pipelined."""
        return int(_lib.lib().fdc_pipeline_sinks_latency(self._h, sinks._h))

    def work_sinks_raw(self, in_ptr, nblocks, out_ptrs, sinks):
        """fdc_pipeline_work_sinks on raw addresses (timing the C entry itself; the PDUs stay with the bank)."""
        return _lib.check(_lib.lib().fdc_pipeline_work_sinks(self._h, in_ptr, int(nblocks), out_ptrs, None, sinks._h))

    def work_real(self, x, want_spectrum=False):
        """Real input stream (float32 items; fdc_pipeline_work_real): the block's imaginary part is zero."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.size % self.H:
            raise ValueError("input must be a whole number of (N - N/R)-sample items")
        nb = x.size // self.H
        outs, ptrs = self._host_outs(None, nb)
        spec = np.empty(nb * self.N, dtype=np.complex64) if want_spectrum else None
        _lib.check(_lib.lib().fdc_pipeline_work_real(self._h, x.ctypes.data, nb, ptrs,
                                                    spec.ctypes.data if spec is not None else None))
        self._ran(nb)
        outs = self._host_results(outs, nb)
        return (outs, spec) if want_spectrum else outs

    def work_iq(self, x, scale=1.0, want_spectrum=False, outs=None):
        """Complex integer input (fdc_pipeline_work_iq): x is int16 (sc16) or int8 (sc8), a flat interleaved I/Q array or one of shape (n, 2).
        Sample k is (I_k * scale, Q_k * scale) in float32; the outputs are bit-identical to work() on that complex64 input.  scale defaults to
        1.0 as GNU Radio's interleaved_short_to_complex; UHD's sc16 -> fc32 is scale = 1/32768.  The first work call after create / reset
        latches the handle's input form (float, or this format and scale): a call in another form raises FdcError.  outs: as work()."""
        x, fmt, n, sc = _iq_input(x, scale, self.H)
        nb = n // self.H
        outs, ptrs = self._host_outs(outs, nb)
        spec = np.empty(nb * self.N, dtype=np.complex64) if want_spectrum else None
        _lib.check(_lib.lib().fdc_pipeline_work_iq(self._h, fmt, float(sc), x.ctypes.data, nb, ptrs,
                                                  spec.ctypes.data if spec is not None else None))
        self._ran(nb)
        outs = self._host_results(outs, nb)
        return (outs, spec) if want_spectrum else outs

    def work_span_iq(self, halo, x, first_block, scale=1.0, want_spectrum=False):
        """fdc_pipeline_work_span_iq: one span of a longer integer stream; halo = the N/R integer samples in front of it (None = zeros)."""
        x, fmt, n, sc = _iq_input(x, scale, self.H)
        hp = None
        if halo is not None:
            halo, hfmt, hn, _ = _iq_input(halo, scale, 0)
            if hfmt != fmt or hn != self.ovl:
                raise ValueError("halo: N/R samples of the input's format")
            hp = halo.ctypes.data
        nb = n // self.H
        outs, ptrs = self._host_outs(None, nb)
        spec = np.empty(nb * self.N, dtype=np.complex64) if want_spectrum else None
        _lib.check(_lib.lib().fdc_pipeline_work_span_iq(self._h, fmt, float(sc), hp, x.ctypes.data, int(first_block), nb, ptrs,
                                                       spec.ctypes.data if spec is not None else None))
        self._ran(nb)
        outs = self._host_results(outs, nb)
        return (outs, spec) if want_spectrum else outs

    def work_raw(self, in_ptr, nblocks, out_ptrs):
        """fdc_pipeline_work on raw addresses (out_ptrs: ctypes array of c_void_p, one per channel) — for callers that
        keep their buffers and want no per-call Python work, e.g. timing the C entry itself."""
        rc = _lib.check(_lib.lib().fdc_pipeline_work(self._h, in_ptr, int(nblocks), out_ptrs, None))
        self._ran(int(nblocks))
        return rc

    def work_spectrum(self, spec_items, want_spectrum=False, sinks=None):
        """Items that are already transformed (unnormalised, fftshifted): hier block with inpveclen > 1."""
        spec_items = np.ascontiguousarray(spec_items, dtype=np.complex64)
        if spec_items.size % self.N:
            raise ValueError("input must be a whole number of N-sample spectrum items")
        nb = spec_items.size // self.N
        outs = [np.empty(nb * lo, dtype=np.complex64) for lo in self.lout]
        ptrs = (C.c_void_p * max(1, len(outs)))(*[o.ctypes.data for o in outs])
        spec = np.empty(nb * self.N, dtype=np.complex64) if want_spectrum else None
        _lib.check(_lib.lib().fdc_pipeline_work_spectrum(self._h, spec_items.ctypes.data, nb, ptrs,
                                                        spec.ctypes.data if spec is not None else None,
                                                        sinks._h if sinks is not None else None))
        return (outs, spec) if want_spectrum else outs

    def reset(self):
        _lib.lib().fdc_pipeline_reset(self._h)

    # -- device path
    def process_device(self, d_ring, first_block, nblocks, d_out, d_spectrum=None, stream=None, d_group_power=None):
        """d_group_power: device buffer of nblocks * N/16 float32 for the power of the spectrum's 16-bin groups (fdc_pipeline_process_device_power:
        what Sinks.prepare(..., from_groups=True) sums a bank's power cells from)."""
        if d_group_power:
            _lib.check(_lib.lib().fdc_pipeline_process_device_power(self._h, d_ring, int(first_block), int(nblocks), d_out, d_spectrum,
                                                                   d_group_power, stream))
        else:
            _lib.check(_lib.lib().fdc_pipeline_process_device(self._h, d_ring, int(first_block), int(nblocks), d_out,
                                                             d_spectrum, stream))
            self._ran(int(nblocks))

    def process_device_iq(self, fmt, scale, d_ring, first_block, nblocks, d_out, d_spectrum=None, stream=None):
        """fdc_pipeline_process_device_iq: a device ring of complex integers (fmt: "sc16" / "sc8" or IQ_SC16 / IQ_SC8; d_ring 4-byte aligned).
        Stateless, as process_device."""
        fmt = IQ_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else int(fmt)
        if fmt not in (IQ_SC16, IQ_SC8):
            raise ValueError("fmt is 'sc16' or 'sc8'")
        _lib.check(_lib.lib().fdc_pipeline_process_device_iq(self._h, fmt, float(np.float32(scale)), d_ring, int(first_block), int(nblocks),
                                                            d_out, d_spectrum, stream))
        self._ran(int(nblocks))

    def synchronize(self):
        _lib.check(_lib.lib().fdc_pipeline_synchronize(self._h))

    def reserve_compute_units(self, n):
        """Leave n compute units out of the persistent block kernels' grids (kernels of another stream run beside them); returns the
        number of workgroups they launch on: launch groups should hold a multiple of it in blocks."""
        return _lib.check(_lib.lib().fdc_pipeline_reserve_compute_units(self._h, int(n)))

    def stream(self):
        return _lib.lib().fdc_pipeline_stream(self._h)

    def enable_timing(self, on=True):
        _lib.check(_lib.lib().fdc_pipeline_enable_timing(self._h, int(on)))

    def last_kernel_ms(self):
        """[ms pass A, ms pass B, ms channel kernels, launch groups] summed since enable/last readout."""
        ms = (C.c_float * 4)()
        _lib.check(_lib.lib().fdc_pipeline_last_kernel_ms(self._h, ms, 4))
        return [float(v) for v in ms]

    def path(self):
        """0 generic kernels, 1 radix-16 kernels with a spectrum in memory, 2 uniform-plan two-stage path."""
        return int(_lib.lib().fdc_pipeline_path(self._h))

    def describe(self):
        """fdc_pipeline_describe: which kernels the plan was given, in words."""
        buf = C.create_string_buffer(512)
        _lib.lib().fdc_pipeline_describe(self._h, buf, 512)
        return buf.value.decode()

    def chunk_blocks(self):
        return int(_lib.lib().fdc_pipeline_chunk_blocks(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib().fdc_pipeline_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PipelineGroup(_OutputFormat):
    """fdc_pipeline_group handle: one work() spread over several devices (contiguous spans of the call's blocks, one per
    member, run concurrently).  devices: HIP ordinals, repeats allowed (virtual members on one GPU).  Same work() / work_real()
    as Pipeline; state (overlap history, block counter) is kept once, by the group."""

    def __init__(self, blocklen, relinvovl, channels, devices, windowtype=WINDOWTYPES.HANN, max_blocks=64, min_span_blocks=0,
                 chunk_blocks=0, keep_spectrum=False, flags=None, min_block_launch=None, host_sub_blocks=None):
        self._h = C.c_void_p()
        self.N, self.R = int(blocklen), int(relinvovl)
        self.channels = [(int(f), int(l), float(p), float(s)) for (f, l, p, s) in channels]
        self.devices = [int(d) for d in devices]
        arr = (_lib.fdc_channel * max(1, len(self.channels)))()
        for i, (f, l, p, s) in enumerate(self.channels):
            arr[i].f, arr[i].l, arr[i].passbw, arr[i].stopbw = f, l, p, s
        dflags, dmin, dsub = _default_cfg_fields()
        cfg = _lib.fdc_pipeline_cfg(0, self.N, self.R, int(windowtype), len(self.channels), arr,
                                    int(max_blocks), int(chunk_blocks), int(bool(keep_spectrum)),
                                    dflags if flags is None else int(flags), dmin if min_block_launch is None else int(min_block_launch),
                                    dsub if host_sub_blocks is None else int(host_sub_blocks))
        devs = (C.c_int32 * max(1, len(self.devices)))(*self.devices)
        rc = _lib.lib().fdc_pipeline_group_create(C.byref(cfg), devs, len(self.devices), int(min_span_blocks), C.byref(self._h))
        if rc == -1:
            raise ValueError(_lib.lib().fdc_last_error().decode())
        _lib.check(rc)
        self.max_blocks = int(max_blocks)
        self.keep_spectrum = bool(keep_spectrum)
        self.ovl = self.N // self.R if self.N >= self.R else 0
        self.H = self.N - self.ovl
        m0 = _lib.lib().fdc_pipeline_group_member(self._h, 0)
        self.lout = [_lib.lib().fdc_pipeline_channel_lout(m0, c) for c in range(len(self.channels))]

    def set_output_format(self, fmt, scale=1.0):
        """fdc_pipeline_group_set_output_format: Pipeline.set_output_format for every member."""
        code, sc = _oq_format(fmt, scale)
        _lib.check(_lib.lib().fdc_pipeline_group_set_output_format(self._h, code, float(sc)))
        self._oq, self._oq_scale = code, sc if code else np.float32(1.0)

    def set_fine_tuning(self, nu):
        """fdc_pipeline_group_set_fine_tuning: Pipeline.set_fine_tuning for every member."""
        _set_fine_tuning(_lib.lib().fdc_pipeline_group_set_fine_tuning, self._h, len(self.channels), nu)

    _last_nb = None        # block count of the last work call that had blocks (levels())
    _call_nb = 0           # ... and of the last work call

    def set_levels(self, on=True):
        """fdc_pipeline_group_set_levels: Pipeline.set_levels for every member."""
        _lib.check(_lib.lib().fdc_pipeline_group_set_levels(self._h, int(bool(on))))

    def set_gains(self, g):
        """fdc_pipeline_group_set_gains: Pipeline.set_gains for every member."""
        _set_gains(_lib.lib().fdc_pipeline_group_set_gains, self._h, len(self.channels), g)

    def levels(self, nblocks=None):
        """fdc_pipeline_group_levels: Pipeline.levels of the last group call, the members' spans put together in block order."""
        return _levels(_lib.lib().fdc_pipeline_group_levels, self._h, len(self.channels), self._last_nb, nblocks)

    def set_lag1(self, on=True):
        """fdc_pipeline_group_set_lag1: Pipeline.set_lag1 for every member."""
        _lib.check(_lib.lib().fdc_pipeline_group_set_lag1(self._h, int(bool(on))))

    def lag1(self, nblocks=None):
        """fdc_pipeline_group_lag1: Pipeline.lag1 of the last group call, the members' spans put together in block order."""
        return _lag1(_lib.lib().fdc_pipeline_group_lag1, self._h, len(self.channels), self._last_nb, nblocks)

    def _run(self, fn, x, nb, want_spectrum, outs):
        outs = self._check_outs(outs, nb)
        ptrs = (C.c_void_p * max(1, len(outs)))(*[o.ctypes.data for o in outs])
        spec = np.empty(nb * self.N, dtype=np.complex64) if want_spectrum else None
        _lib.check(fn(self._h, x.ctypes.data, nb, ptrs, spec.ctypes.data if spec is not None else None))
        self._call_nb = int(nb)
        if nb > 0:
            self._last_nb = int(nb)
        return (outs, spec) if want_spectrum else outs

    def work(self, x, want_spectrum=False, outs=None):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if x.size % self.H:
            raise ValueError("input must be a whole number of (N - N/R)-sample items")
        return self._run(_lib.lib().fdc_pipeline_group_work, x, x.size // self.H, want_spectrum, outs)

    def work_real(self, x, want_spectrum=False):
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.size % self.H:
            raise ValueError("input must be a whole number of (N - N/R)-sample items")
        return self._run(_lib.lib().fdc_pipeline_group_work_real, x, x.size // self.H, want_spectrum, None)

    def work_iq(self, x, scale=1.0, want_spectrum=False, outs=None):
        """Complex integer input (fdc_pipeline_group_work_iq): the arguments and the bytes of Pipeline.work_iq."""
        x, fmt, n, sc = _iq_input(x, scale, self.H)
        lib = _lib.lib()
        return self._run(lambda h, xp, nb, ptrs, sp: lib.fdc_pipeline_group_work_iq(h, fmt, float(sc), xp, nb, ptrs, sp), x, n // self.H,
                         want_spectrum, outs)

    def work_raw(self, in_ptr, nblocks, out_ptrs):
        rc = _lib.check(_lib.lib().fdc_pipeline_group_work(self._h, in_ptr, int(nblocks), out_ptrs, None))
        if int(nblocks) > 0:
            self._last_nb = int(nblocks)
        return rc

    def reset(self):
        _lib.lib().fdc_pipeline_group_reset(self._h)

    def size(self):
        return int(_lib.lib().fdc_pipeline_group_size(self._h))

    def member_path(self, i=0):
        return int(_lib.lib().fdc_pipeline_path(_lib.lib().fdc_pipeline_group_member(self._h, i)))

    def path(self):
        return self.member_path(0)

    def member_max_blocks(self):
        return int(_lib.lib().fdc_pipeline_group_member_max_blocks(self._h))

    def last_spans(self):
        """[(first_block, nblocks)] per member for the last call (nblocks 0 = the member was idle)."""
        n = self.size()
        fb, nb = (C.c_int64 * n)(), (C.c_int32 * n)()
        _lib.check(_lib.lib().fdc_pipeline_group_last_spans(self._h, fb, nb, n))
        return [(int(fb[i]), int(nb[i])) for i in range(n)]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib().fdc_pipeline_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrequencyDomainChannelizer:
    """Same constructor as FDC.FrequencyDomainChannelizer (python/FrequencyDomainChannelizer.py:46-60).

    work(samples) takes a whole number of (blocksize - blocksize/relinvovl)-sample items of the input
    stream and returns the list of hier-block output ports: [spectrum (only if debug)] + one stream per
    throughput channel (:292-299, :314-315).  State (overlap history, window phase) carries over calls.
    """

    def __init__(self, inptype, inpveclen, blocksize, relinvovl,
                 throughput_channels,
                 activity_controlled_channels,
                 act_contr_threshold,
                 fs, centerfrequency, freqmode,
                 windowtype,
                 msgoutput, fileoutput, outputpath,
                 threaded,
                 activity_detection_segments, act_det_threshold, minchandist,
                 act_det_deactivation_delay, minchanflankpuffer, verbose,
                 pow_act_deactivation_delay,
                 pow_act_maxblocks, act_det_maxblocks,
                 debug, device_id=0, max_blocks=64, devices=None, pipelined=False, waterfall=None, iq_input=None, iq_scale=1.0,
                 iq_output=None, iq_output_scale=1.0, fine_tuning=False, *, payload_format=None, payload_scale=1.0, levels=False, gains=None, lag1=False,
                 demod=None, demod_gain=1.0, audio_decim=None, audio_taps=None, audio_format="f32", audio_scale=1.0, squelch_db=None, squelch_close_db=None,
                 squelch_hang=0, audio_packed=False, audio_up=None, audio_down=None, tones=None, tone_group=16, tone_frame=32, tone_squelch=None, tone_open=None,
                 tone_close=None, tone_ratio=0.0, tone_guard=0, tone_hang=0):
        # pipelined (not an argument of the reference): the sink blocks run beside the front end of the FOLLOWING work() calls, as the
        # thread-per-block scheduler runs them beside the FFT in the reference (fdc_pipeline_work_sinks on a look-ahead bank,
        # include/fdc_amd.h): same PDUs, handed out one or two work() calls later; flush() at the end of the stream
        self.pipelined = bool(pipelined)
        self.verbose = int(verbose)
        # payload_format / payload_scale (not arguments of the reference): the PDU payloads of the sink blocks as "sc16" / "sc8", narrowed on the
        # device (fdc_sinks_set_payload_format); messages then carry int16[n, 2] / int8[n, 2] arrays and the files the narrow bytes
        from .sinks import _check_face_payload
        self._payload_code = _check_face_payload(payload_format, self.verbose)
        self.itemsize = inptype
        self.debug = bool(debug)
        if self.itemsize not in (8, 4):
            raise ValueError('Unknown input type. ')            # :205-210 (there only gr_complex is reachable; the Float
        #                                                         input type of the GRC block, itemsize 4, is served here
        #                                                         by the fft_vfc front end the reference meant at :207-208)

        # frequency conventions (:70-91): everything is stored normalised to [0, 1) with DC at 0.5
        self.freqmode, self.get_freq, self.set_freq, self.get_bw, self.set_bw = freq_converters(freqmode, fs, centerfrequency)

        self.throughput_channels = self._convert(throughput_channels, self.get_channel, 'Throughput channels')
        self.activity_controlled_channels = self._convert(activity_controlled_channels, self.get_channel,
                                                          'Activity controlled channels')
        self.activity_detection_segments = self._convert(activity_detection_segments, self.get_segment,
                                                         'Activity detection segments')

        self.inpveclen = int(inpveclen) if int(inpveclen) > 0 else 1
        self.blocksize = nextpow2(blocksize)                    # :138
        self.relinvovl = nextpow2(relinvovl)                    # :139
        self.ovllen = self.blocksize // self.relinvovl          # :140
        self.inpblocklen = self.blocksize - self.ovllen         # :141
        if self.inpveclen != 1 and self.inpveclen != self.blocksize:
            raise ValueError("inpveclen must be 1 (sample stream) or blocksize (items already transformed, :284-290)")
        if self.itemsize == 4:
            # Float input is the fft_vfc front end on a sample stream; items that are already spectra are complex, and the sink
            # blocks hang on the complex chain only — refuse here, not at the first work() call
            if self.inpveclen != 1:
                raise ValueError("Float input (itemsize 4) needs inpveclen 1: pre-transformed items are complex spectra")
            if self.activity_controlled_channels or self.activity_detection_segments:
                raise ValueError("Float input (itemsize 4) cannot feed activity-controlled channels or detection segments")
        # iq_input (not an argument of the reference): "sc16" / "sc8" — work() takes interleaved int16 / int8 I/Q as a radio source delivers it
        # (UHD sc16 with iq_scale = 1/32768; the default 1.0 is GNU Radio's interleaved_short_to_complex) and converts it inside the device's
        # loads (Pipeline.work_iq).  The restrictions of the Float input: a sample stream, no sink blocks, no waterfall.
        if iq_input is not None and iq_input not in IQ_FORMATS:
            raise ValueError("iq_input is None, 'sc16' or 'sc8'")
        self.iq_input, self.iq_scale = iq_input, float(iq_scale)
        if iq_input is not None:
            if self.itemsize != 8:
                raise ValueError("iq_input replaces the complex input type (itemsize 8)")
            if self.inpveclen != 1:
                raise ValueError("iq_input needs inpveclen 1: pre-transformed items are complex spectra")
            if activity_controlled_channels or activity_detection_segments:
                raise ValueError("iq_input cannot feed activity-controlled channels or detection segments")
            if waterfall is not None:
                raise ValueError("iq_input cannot feed a waterfall")
            with np.errstate(over="ignore"):
                sc = np.float32(iq_scale)
            if not np.isfinite(sc) or sc == 0:
                raise ValueError("iq_scale must be finite and not zero")
        # iq_output (not an argument of the reference): "sc16" / "sc8" — the channel ports come back as int16 / int8 arrays of shape (n, 2), narrowed on
        # the device (Pipeline.set_output_format; UHD's sc16 convention is iq_output_scale = 32768).  The restrictions of iq_input; combines with it
        # and with the Float input type.
        if iq_output is not None and iq_output not in ("sc16", "sc8"):
            raise ValueError("iq_output is None, 'sc16' or 'sc8'")
        self.iq_output, self.iq_output_scale = iq_output, float(iq_output_scale)
        if iq_output is not None:
            if self.inpveclen != 1:
                raise ValueError("iq_output needs inpveclen 1: the pre-transformed item entry writes complex outputs only")
            if activity_controlled_channels or activity_detection_segments:
                raise ValueError("iq_output cannot go with activity-controlled channels or detection segments")
            if waterfall is not None:
                raise ValueError("iq_output cannot go with a waterfall")
            _oq_format(iq_output, iq_output_scale)

        # fine_tuning (not an argument of the reference): every throughput channel comes out centred on its requested carrier, not on the bin its slice
        # was rounded, wrapped or clamped to (Pipeline.set_fine_tuning with fine_tuning_nu of each channel, kept in self.fine_nu).  The PDUs of the sink
        # blocks carry rel_cfreq themselves.
        self.fine_tuning = bool(fine_tuning)
        self.fine_nu = None
        if self.fine_tuning:
            if self.inpveclen != 1:
                raise ValueError("fine_tuning needs inpveclen 1: the pre-transformed item entry writes the channels as they are cut")
            if activity_controlled_channels or activity_detection_segments:
                raise ValueError("fine_tuning cannot go with activity-controlled channels or detection segments")
            if waterfall is not None:
                raise ValueError("fine_tuning cannot go with a waterfall")
            self.fine_nu = []
            for (fr, bw) in self.throughput_channels:
                f, l = get_opt_channelparams(self.blocksize, self.relinvovl, fr, bw)[:2]
                nu = fine_tuning_nu(self.blocksize, fr, f, l)
                if not abs(nu) < 0.5:
                    raise ValueError("fine_tuning: the carrier %r lies outside its slice [%d, %d) (a slice clamped at the band edge)" % (fr, f, f + l))
                self.fine_nu.append(nu)

        # levels (not an argument of the reference): after every work() self.levels is float32[items, throughput channels, 2], (power, peak) of every
        # block of every port as the device summed them (Pipeline.set_levels): of the float samples, after fine tuning and before iq_output narrows them
        self.levels_on = bool(levels)
        self.levels = None
        if self.levels_on:
            if self.inpveclen != 1:
                raise ValueError("levels needs inpveclen 1: the pre-transformed item entry gives no channel levels")
            if activity_controlled_channels or activity_detection_segments:
                raise ValueError("levels cannot go with activity-controlled channels or detection segments")
            if waterfall is not None:
                raise ValueError("levels cannot go with a waterfall")

        # lag1 (not an argument of the reference): after every work() self.lag1 is complex64[items, throughput channels], the lag-1 correlation of every
        # block of every port as the device summed it (Pipeline.set_lag1): of the float samples, after fine tuning and the gain, before iq_output narrows
        self.lag1_on = bool(lag1)
        self.lag1 = None
        if self.lag1_on:
            if self.inpveclen != 1:
                raise ValueError("lag1 needs inpveclen 1: the pre-transformed item entry gives no channel lag-1 correlation")
            if activity_controlled_channels or activity_detection_segments:
                raise ValueError("lag1 cannot go with activity-controlled channels or detection segments")
            if waterfall is not None:
                raise ValueError("lag1 cannot go with a waterfall")

        # demod / demod_gain (not arguments of the reference): "fm" / "mag" — the channel ports come back as float32 arrays, the FM discriminator's output
        # (gain * angle of y[t] conj(y[t - 1]): quadrature_demod_cf behind every port) or the envelope (complex_to_mag), computed on the device behind
        # fine tuning and the gains (Pipeline.set_demod); levels and lag1 stay those of the complex samples.  The refusals of lag1, and iq_output
        self.demod, self.demod_gain = demod, float(demod_gain)
        if demod is not None:
            _demod_mode(demod, demod_gain)
            if self.inpveclen != 1:
                raise ValueError("demod needs inpveclen 1: the pre-transformed item entry writes complex outputs only")
            if activity_controlled_channels or activity_detection_segments:
                raise ValueError("demod cannot go with activity-controlled channels or detection segments")
            if waterfall is not None:
                raise ValueError("demod cannot go with a waterfall")
            if iq_output is not None:
                raise ValueError("demod cannot go with iq_output: the demodulated ports are float32")
            if devices is not None and len(devices) > 1:
                raise ValueError("demod needs one device: the group entries do not serve the channel demodulation")

        # audio_decim / audio_taps / audio_format / audio_scale (not arguments of the reference): the decimating low-pass behind every demodulated port
        # (fir_filter_fff with decimation audio_decim), on the device (Pipeline.set_audio): the ports come back at the audio rate, lout_c / audio_decim
        # samples per block, as float32 or ("s16") int16.  It needs demod and its taps (lowpass_taps), and carries the refusals of demod
        self.audio_decim, self.audio_taps, self.audio_format, self.audio_scale = audio_decim, audio_taps, audio_format, float(audio_scale)
        if audio_decim is not None:
            if demod is None:
                raise ValueError("audio_decim needs demod: the audio filter runs behind the channel demodulation")
            if audio_taps is None:
                raise ValueError("audio_decim needs audio_taps (lowpass_taps)")
            _audio_args(audio_decim, audio_taps, audio_format, audio_scale)
        # audio_up / audio_down (not arguments of the reference): the rational resampler in the decimating low-pass's place (Pipeline.set_audio_resampler):
        # the ports come back at the channel rate times audio_up / audio_down, the valid samples of every call.  audio_taps: the prototype taps
        # (default: resampler_taps(audio_up, audio_down)); audio_format and audio_scale as above
        self.audio_up, self.audio_down = audio_up, audio_down
        if audio_up is not None or audio_down is not None:
            if audio_decim is not None:
                raise ValueError("audio_decim and audio_up / audio_down are the two forms of the channel audio: give one of them")
            if audio_up is None or audio_down is None:
                raise ValueError("audio_up and audio_down go together")
            if demod is None:
                raise ValueError("audio_up / audio_down need demod: the resampler runs behind the channel demodulation")
            if audio_taps is None:
                self.audio_taps = resampler_taps(audio_up, audio_down)
            _resampler_args(audio_up, audio_down, self.audio_taps, audio_format, audio_scale)
        elif audio_decim is None and audio_taps is not None:
            raise ValueError("audio_taps needs audio_decim or audio_up / audio_down")

        # squelch_db / squelch_close_db / squelch_hang (not arguments of the reference): a carrier-operated squelch per throughput channel, decided on the
        # device from the levels (Pipeline.set_squelch): the channel opens at a block whose mean power in front of the gain reaches squelch_db (dB; a scalar
        # or one value per channel), stays open while it reaches squelch_close_db (default: squelch_db) and closes after squelch_hang + 1 blocks below.
        # After every work() self.squelch is uint8[items, throughput channels]; with audio_decim the audio of closed blocks is zero.  It needs levels
        self.squelch_db, self.squelch_close_db, self.squelch_hang = squelch_db, squelch_close_db, squelch_hang
        self.squelch = None
        if squelch_db is not None:
            if not self.levels_on:
                raise ValueError("squelch_db needs levels=True: the squelch decides on the channel levels")
            if devices is not None and len(devices) > 1:
                raise ValueError("squelch_db needs one device: the group entries do not serve the channel squelch")
            # (the thresholds take the channels' lout, which the handle knows: the checks that do not are made here)
            _squelch_args(len(self.throughput_channels), *squelch_thresholds(np.ones(len(self.throughput_channels)), squelch_db, squelch_close_db), squelch_hang)
        elif squelch_close_db is not None or squelch_hang:
            raise ValueError("squelch_close_db and squelch_hang need squelch_db")

        # audio_packed (not an argument of the reference): with audio_decim and squelch_db, only the audio of open (item, channel) cells leaves the
        # device (Pipeline.set_audio_packing): work() returns per channel the audio of its open items of the call, self.squelch says which they are
        if not isinstance(audio_packed, (bool, np.bool_)):
            raise ValueError("audio_packed is a bool")
        self.audio_packed = bool(audio_packed)
        if self.audio_packed and (audio_decim is None or squelch_db is None):
            raise ValueError("audio_packed needs audio_decim and squelch_db: it packs the channel audio by the squelch's mask")

        # tones / tone_group / tone_frame (not arguments of the reference): a tone bank per throughput channel behind the demodulation, on the device
        # (Pipeline.set_tones): tones are the uint32 phase increments, [T] for all channels or [C, T] (tone_increments), tone_group the samples summed in
        # front of the correlators, tone_frame the items per frame.  After every work() self.tones is complex64 [frames the call completed, throughput
        # channels, T]; a call that ends inside a frame completes none, and the frame goes on in the next call.  It needs demod
        self.tone_inc, self.tone_group, self.tone_frame = tones, tone_group, tone_frame
        self.tones = None
        if tones is not None:
            if demod is None:
                raise ValueError("tones needs demod: the tone bank runs behind the channel demodulation")
            self.tone_inc = _tones_args(len(self.throughput_channels), tones, tone_group, tone_frame)[0]

        # tone_squelch / tone_open / tone_close / tone_ratio / tone_guard / tone_hang (not arguments of the reference): a tone squelch per throughput
        # channel, decided on the device from the tones' frame rows (Pipeline.set_tone_squelch): tone_squelch is the index of the selected tone per
        # channel (or one for all; -1: not tone-gated), tone_open / tone_close thresholds on |Z|^2 (tone_squelch_thresholds), tone_ratio what the tone
        # must keep over the strongest tone more than tone_guard places away, tone_hang the hang count in frames.  self.squelch is then carrier AND
        # tone, and after every work() self.tone_squelch_dec is uint8 [frames the call completed, throughput channels].  It needs tones and squelch_db
        self.tone_squelch = None
        self.tone_squelch_dec = None
        if tone_squelch is not None:
            if tones is None or squelch_db is None:
                raise ValueError("tone_squelch needs tones and squelch_db: it decides on the tones' frame rows and gates the squelch's mask")
            self.tone_squelch = _tone_squelch_args(len(self.throughput_channels), tone_squelch, tone_open, tone_close, tone_ratio, tone_guard, tone_hang)
            if self.tone_squelch[0].size and int(self.tone_squelch[0].max()) >= self.tone_inc.shape[1]:
                raise ValueError("tone_squelch selects tone %d of %d" % (int(self.tone_squelch[0].max()), self.tone_inc.shape[1]))
        elif tone_open is not None or tone_close is not None or tone_ratio or tone_guard or tone_hang:
            raise ValueError("tone_open, tone_close, tone_ratio, tone_guard and tone_hang need tone_squelch")

        # gains (not an argument of the reference): one output gain per throughput channel, applied on the device behind fine tuning and in front of the
        # levels and of iq_output's narrowing (Pipeline.set_gains); set_gains() changes them between work() calls (an AGC fed from self.levels)
        self.gains = None if gains is None else _check_gains(len(self.throughput_channels), gains)
        self._gains_refusal = None
        if self.inpveclen != 1:
            self._gains_refusal = "gains needs inpveclen 1: the pre-transformed item entry writes the channels as they are cut"
        elif activity_controlled_channels or activity_detection_segments:
            self._gains_refusal = "gains cannot go with activity-controlled channels or detection segments"
        elif waterfall is not None:
            self._gains_refusal = "gains cannot go with a waterfall"
        if self.gains is not None and self._gains_refusal:
            raise ValueError(self._gains_refusal)

        if self.verbose:                                        # runtime information, :176-193
            bar = '\n' + '#' * 32 + '\n'
            for ln in (bar, '# gr-FDC Frequency Domain Channelizer Runtime Information', bar,
                       'Blocksize     = {}'.format(self.blocksize), 'InputVecLen   = {}'.format(self.inpveclen),
                       'Relinvovl     = {}'.format(self.relinvovl), 'Ovllen        = {}'.format(self.ovllen),
                       'MsgOutput     = {}'.format(msgoutput), 'FileOutput    = {}'.format(fileoutput),
                       'Outputpath    = {}'.format(outputpath), 'Threaded      = {}'.format(threaded),
                       'Debugoutput   = {}'.format(self.debug), bar,
                       '# Throughput channels:         {}'.format(str(self.throughput_channels)),
                       '# Activity control channels:   {}'.format(str(self.activity_controlled_channels)),
                       '# Activity detection segments: {}'.format(str(self.activity_detection_segments)), bar):
                self.log(ln)
        self.channel_params = [get_opt_channelparams(self.blocksize, self.relinvovl, fr, bw)
                               for (fr, bw) in self.throughput_channels]
        if self.verbose:                                        # :223-224 (dec = blocksize / l)
            for i, (f, l, lout, pbw, sbw) in enumerate(self.channel_params):
                self.log('# Throughput Channel {}: dec={}, f={}, l={}, lout={}, bw=({}, {})'.format(
                    i, self.blocksize / l, f, l, lout, pbw, sbw))
        # activity-controlled channels (:237-251) and detection segments (:261-278) share one spectrum on the device
        self.msgoutput, self.fileoutput, self.outputpath = bool(msgoutput), bool(fileoutput), str(outputpath)
        self.sinks = None
        if self.activity_controlled_channels or self.activity_detection_segments:
            from .sinks import Sinks
            pad = int(pow_act_deactivation_delay) if int(pow_act_deactivation_delay) >= 0 else 0
            add = int(act_det_deactivation_delay) if int(act_det_deactivation_delay) >= 0 else 0
            puf = float(minchanflankpuffer) if 0.0 <= float(minchanflankpuffer) else 0.2
            self.sinks = Sinks(self.blocksize, self.relinvovl,
                               pac=[(cf, bw, i) for i, (cf, bw) in enumerate(self.activity_controlled_channels)],
                               pac_thresh=float(act_contr_threshold), pac_maxblocks=int(pow_act_maxblocks), pac_delay=pad,
                               segments=[tuple(sg) for sg in self.activity_detection_segments],
                               det_thresh=float(act_det_threshold), det_maxblocks=int(act_det_maxblocks),
                               minchandist=self.get_bw(minchandist) if self.activity_detection_segments else 0.005,
                               det_delay=add, puffer=puf, max_blocks=max_blocks, device_id=device_id,
                               det_variant=1,      # the hier block instantiates SegmentDetection (:25, :261-278)
                               verbose=self.verbose, lookahead=self.pipelined and self.inpveclen == 1)
            if self._payload_code != 0:                         # before the first call, serial and pipelined form alike
                self.sinks.set_payload_format(payload_format, payload_scale)
        # devices = [ordinals]: the throughput chain of one work() call spread over several GPUs (fdc_pipeline_group); the sink
        # blocks stay on ONE device's spectrum, so a hier block with sinks keeps the single-device handle
        if devices is not None and len(devices) > 1 and self.sinks is None and self.inpveclen == 1:
            self.pipeline = PipelineGroup(self.blocksize, self.relinvovl,
                                          [(f, l, p, s) for (f, l, _lo, p, s) in self.channel_params], devices,
                                          windowtype=int(windowtype), max_blocks=max_blocks, keep_spectrum=self.debug)
        else:
            self.pipeline = Pipeline(self.blocksize, self.relinvovl,
                                     [(f, l, p, s) for (f, l, _lo, p, s) in self.channel_params],
                                     windowtype=int(windowtype), max_blocks=max_blocks,
                                     device_id=devices[0] if devices else device_id,
                                     keep_spectrum=self.debug or self.sinks is not None)
        if iq_output is not None:
            self.pipeline.set_output_format(iq_output, iq_output_scale)
        if self.fine_tuning:
            self.pipeline.set_fine_tuning(np.asarray(self.fine_nu, dtype=np.float64))
        if self.levels_on:
            self.pipeline.set_levels(True)
        if self.gains is not None:
            self.pipeline.set_gains(self.gains)
        if self.lag1_on:
            self.pipeline.set_lag1(True)
        if self.demod is not None:
            self.pipeline.set_demod(self.demod, self.demod_gain)
        if self.audio_decim is not None:
            self.pipeline.set_audio(self.audio_decim, self.audio_taps, self.audio_format, self.audio_scale)
        if self.audio_up is not None:
            self.pipeline.set_audio_resampler(self.audio_up, self.audio_down, self.audio_taps, self.audio_format, self.audio_scale)
        if self.squelch_db is not None:
            self.set_squelch(self.squelch_db, self.squelch_close_db, self.squelch_hang)
        if self.audio_packed:
            self.pipeline.set_audio_packing(True)
        if self.tone_inc is not None:
            self.pipeline.set_tones(self.tone_inc, self.tone_group, self.tone_frame)
        if self.tone_squelch is not None:
            self.pipeline.set_tone_squelch(*self.tone_squelch)
        self.N_throughput_channelizers = len(self.channel_params)
        # waterfall (not an argument of the reference, whose example flowgraph wires the spectrum to complex_to_mag_squared and
        # FDC.WaterfallMsgTagging outside the hier block): a gr_fdc_amd.Waterfall fed from the spectrum on the device; work() then
        # returns (ports, rows)
        self.waterfall = waterfall
        if waterfall is not None:
            if not isinstance(self.pipeline, Pipeline) or self.sinks is not None or self.inpveclen != 1 or self.itemsize != 8 or self.debug:
                raise ValueError("a waterfall needs a complex sample stream on one device, without sink blocks and without the debug port")
            if waterfall.blocklen != self.blocksize or waterfall.max_items < int(max_blocks):
                raise ValueError("the waterfall needs blocklen = blocksize and max_items >= max_blocks")
        self.messages = []          # PDUs published on "msgout" by the last work() call

    @staticmethod
    def _convert(lst, conv, what):
        out = []
        if lst is None:
            return out
        if not isinstance(lst, (list, tuple)):
            raise ValueError('{} are invalid. Exiting...'.format(what))
        for k in lst:
            c = conv(k)
            if c is None:
                raise ValueError('Cannot convert {} to channel/segment. must be list or tuple of two numbers. '.format(k))
            out.append(c)
        return out

    def get_opt_channelparams(self, freq, bw):
        return get_opt_channelparams(self.blocksize, self.relinvovl, freq, bw)

    def log(self, s):                                           # :359-371
        if self.verbose == VERBOSEMODE.LOGTOCONSOLE:
            print(str(s))
        elif self.verbose == VERBOSEMODE.LOGTOFILE:
            if not hasattr(self, 'logfile'):
                self.logfile = 'gr-FDC.FreqDomChan.log'
                with open(self.logfile, 'w') as fh:
                    fh.write('\n')
            with open(self.logfile, 'a') as fh:
                fh.write(str(s) + '\n')

    def get_channel(self, c):                                   # :349-352
        if not isinstance(c, (list, tuple)) or len(c) != 2:
            return None
        return [self.get_freq(c[0]), self.get_bw(c[1])]

    def get_segment(self, c):                                   # :354-357
        if not isinstance(c, (list, tuple)) or len(c) != 2:
            return None
        return [self.get_freq(c[0]), self.get_freq(c[1])]

    def work(self, samples):
        """Returns the hier block's stream ports; PDUs of the sink blocks ("msgout", :166-168) are left in
        self.messages as (dict, complex64 array) pairs.  Detection segments run as SegmentDetection instances, like in
        the reference hier block (:261-278)."""
        if self.iq_input is not None:
            if iq_format(samples) != IQ_FORMATS[self.iq_input]:
                raise TypeError("this block takes %s input (%s)" % (self.iq_input, "int16" if self.iq_input == "sc16" else "int8"))
            res = self.pipeline.work_iq(samples, scale=self.iq_scale, want_spectrum=self.debug)
        elif self.inpveclen == 1 and self.itemsize == 4:
            if self.sinks is not None:
                raise ValueError("real input with sink blocks is not supported")
            res = self.pipeline.work_real(samples, want_spectrum=self.debug)
        elif self.waterfall is not None:
            return self.pipeline.work_waterfall(samples, self.waterfall)
        elif self.inpveclen == 1 and self.sinks is None:
            res = self.pipeline.work(samples, want_spectrum=self.debug)
        elif self.inpveclen == 1:
            res = self.pipeline.work(samples, want_spectrum=self.debug, sinks=self.sinks)
        else:       # the front end (stream_to_vector, overlap_save, fft_vcc) is the caller's: :201, :284-290
            res = self.pipeline.work_spectrum(samples, want_spectrum=self.debug, sinks=self.sinks)
        self.messages = []
        if self.sinks is not None:
            self._publish()
        if self.levels_on:
            # (a call without items leaves the handle's previous result in place: this call's array is empty)
            self.levels = self.pipeline.levels() if self.pipeline._call_nb > 0 else np.empty((0, len(self.channel_params), 2), dtype=np.float32)
        if self.lag1_on:
            self.lag1 = self.pipeline.lag1() if self.pipeline._call_nb > 0 else np.empty((0, len(self.channel_params)), dtype=np.complex64)
        if self.squelch_db is not None:
            self.squelch = self.pipeline.squelch() if self.pipeline._call_nb > 0 else np.empty((0, len(self.channel_params)), dtype=np.uint8)
        if self.tone_inc is not None:
            self.tones = (self.pipeline.tones() if self.pipeline._call_nb > 0
                          else np.empty((0, len(self.channel_params), self.tone_inc.shape[1]), dtype=np.complex64))
        if self.tone_squelch is not None:
            self.tone_squelch_dec = (self.pipeline.tone_squelch() if self.pipeline._call_nb > 0
                                     else np.empty((0, len(self.channel_params)), dtype=np.uint8))
        if self.debug:
            outs, spec = res
            return [spec] + outs
        return res

    def _publish(self):
        """The bank's current PDUs -> files and self.messages (appended)"""
        from .sinks import _pac_pdu, _det_pdu, _write_files
        raw = self.sinks._collect()
        pac = [_pac_pdu(m, d) for (m, d) in raw if m["kind"] == 0]
        det = [_det_pdu(m, d) for (m, d) in raw if m["kind"] == 1]
        if self.fileoutput:
            _write_files(self.outputpath, pac, True)
            _write_files(self.outputpath, det, False)
        if self.msgoutput:
            self.messages += pac + det

    def set_gains(self, g):
        """New gains (one per throughput channel, or None: off) from the next work() call on: Pipeline.set_gains, with the constructor's refusals."""
        arr = _check_gains(len(self.throughput_channels), g)
        if arr is not None and self._gains_refusal:
            raise ValueError(self._gains_refusal)
        self.pipeline.set_gains(arr)
        self.gains = arr

    def set_squelch(self, open_db, close_db=None, hang=0):
        """New squelch levels (dB of mean power in front of the gain: a scalar or one per throughput channel; None: off) and hang count from the next
        work() call on: Pipeline.set_squelch over squelch_thresholds; which channels are open is kept.  It needs levels=True and one device."""
        if open_db is None:
            self.pipeline.set_squelch(None)
        else:
            if not self.levels_on or not isinstance(self.pipeline, Pipeline):
                raise ValueError("the squelch needs levels=True and one device")
            self.pipeline.set_squelch(*squelch_thresholds(self.pipeline.lout, open_db, close_db), hang=hang)
        self.squelch_db, self.squelch_close_db, self.squelch_hang = open_db, close_db, hang

    def set_tones(self, inc, group=16, frame=32):
        """A new tone bank (uint32 increments [T] or [throughput channels, T]; None: off), group length and frame length in items from the next work()
        call on: Pipeline.set_tones; the open frame starts anew.  It needs demod and one device."""
        if inc is None:
            self.pipeline.set_tones(None)
            self.tone_inc, self.tones = None, None
            return
        if self.demod is None or not isinstance(self.pipeline, Pipeline):
            raise ValueError("the tones need demod and one device")
        a = _tones_args(len(self.throughput_channels), inc, group, frame)[0]
        self.pipeline.set_tones(a, group, frame)
        self.tone_inc, self.tone_group, self.tone_frame = a, group, frame

    def flush(self):
        """End of the stream (what the block's stop() does): the pipelined form still holds the PDUs of the last one or two work()
        calls; they are published here, batch by batch in stream order, and left in self.messages.  Serial form: nothing to do."""
        self.messages = []
        if self.sinks is not None and self.pipelined and self.inpveclen == 1:
            while self.pipeline.flush_sinks(self.sinks) > 0:
                self._publish()
        return self.messages
