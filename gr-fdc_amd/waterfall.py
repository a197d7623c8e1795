"""FDC.WaterfallMsgTagging (python/WaterfallMsgTagging.py) without Qt: the per-block arithmetic runs on the device (include/fdc_amd.h,
fdc_waterfall_*), the picture is a numpy array.

Waterfall        the block's data path: power vectors of blocklen in, finished rows out (mean power, colour index, RGB888 per pixel)
WaterfallImage   the widget's pixel array and its PDU rectangles (:85-110 msg_handler, :153-241 pxupdate / draw_*), height given instead of
                 the widget geometry
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib

WIDTH = 1024                          # :43 normwidth

Rows = namedtuple("Rows", "power index rgb")      # float32 [n, 1024], uint16 [n, 1024], uint8 [n, 1024, 3]


def _cfg(blocklen, blockdecimation, loginput, minvaldb, maxvaldb, colorscheme):
    return _lib.fdc_waterfall_cfg(int(blocklen), int(blockdecimation), int(bool(loginput)), float(minvaldb), float(maxvaldb),
                                  int(colorscheme))


def check_config(blocklen, blockdecimation=1, loginput=0, minvaldb=-45.0, maxvaldb=-20.0, colorscheme=0):
    """The configuration the library would use (blockdecimation <= 0 -> 1, :37) as a dict; ValueError for a block length the
    reference cannot reshape (neither a multiple nor a divisor of 1024).  Host only."""
    src, out = _cfg(blocklen, blockdecimation, loginput, minvaldb, maxvaldb, colorscheme), _lib.fdc_waterfall_cfg()
    rc = _lib.lib().fdc_waterfall_check(C.byref(src), C.byref(out))
    if rc == -1:
        raise ValueError(_lib.lib().fdc_last_error().decode())
    _lib.check(rc)
    return {k: getattr(out, k) for k, _t in out._fields_}


def color_table(scheme):
    """(1024 x 3 uint8 colours, frame colour) of a scheme (cr_colorscheme, :276-312); unknown schemes are scheme 0.  Host only."""
    t, fr = np.empty((WIDTH, 3), np.uint8), np.empty(3, np.uint8)
    _lib.check(_lib.lib().fdc_waterfall_color_table(int(scheme), t.ctypes.data, fr.ctypes.data))
    return t, fr


def edges(loginput, minvaldb, maxvaldb):
    """The 1023 float64 edges the colour index is counted against (:285-287).  Host only."""
    e = np.empty(WIDTH - 1, np.float64)
    _lib.check(_lib.lib().fdc_waterfall_edges(int(bool(loginput)), float(minvaldb), float(maxvaldb), e.ctypes.data))
    return e


class Waterfall:
    """Same constructor as FDC.WaterfallMsgTagging (:32).  samp_rate, relinvovl and tagmode are kept for the signature, as there
    (only the widget's geometry used them).  max_items: the most blocks one call of the pipeline entry carries (and the blocks per
    internal pass of work())."""

    def __init__(self, blocklen, samp_rate, relinvovl, blockdecimation, loginput, minvaldb, maxvaldb, colorscheme, tagmode,
                 device_id=0, max_items=64):
        c = check_config(blocklen, blockdecimation, loginput, minvaldb, maxvaldb, colorscheme)
        self.blocklen, self.blockdecimation = c["blocklen"], c["blockdecimation"]
        self.samp_rate, self.relinvovl, self.tagmode = float(samp_rate), int(relinvovl), tagmode
        self.loginput, self.minvaldb, self.maxvaldb, self.colorscheme = bool(loginput), float(minvaldb), float(maxvaldb), int(colorscheme)
        self.device_id, self.max_items = int(device_id), int(max_items)
        self._h = C.c_void_p()
        cfg = _cfg(blocklen, blockdecimation, loginput, minvaldb, maxvaldb, colorscheme)
        _lib.check(_lib.lib().fdc_waterfall_create(self.device_id, C.byref(cfg), self.max_items, C.byref(self._h)))

    def rows_for(self, nitems):
        """An upper bound of the rows a call of nitems finishes"""
        return (nitems + self.blockdecimation - 1) // self.blockdecimation

    def _outs(self, nitems):
        cap = self.rows_for(nitems)
        return cap, np.empty((cap, WIDTH), np.float32), np.empty((cap, WIDTH), np.uint16), np.empty((cap, WIDTH, 3), np.uint8)

    def work(self, power):
        """power: nitems x blocklen float32 (the output of complex_to_mag_squared).  Returns the Rows this call finished."""
        x = np.ascontiguousarray(power, dtype=np.float32).reshape(-1)
        if x.size % self.blocklen:
            raise ValueError("input must be a whole number of blocklen-sample vectors")
        nb = x.size // self.blocklen
        cap, rows, idx, rgb = self._outs(nb)
        n = C.c_int32(0)
        _lib.check(_lib.lib().fdc_waterfall_work(self._h, x.ctypes.data, nb, rows.ctypes.data, idx.ctypes.data, rgb.ctypes.data, cap,
                                                 C.byref(n)))
        return Rows(rows[:n.value], idx[:n.value], rgb[:n.value])

    def reset(self):
        _lib.lib().fdc_waterfall_reset(self._h)

    def rows_done(self):
        return int(_lib.lib().fdc_waterfall_rows_done(self._h))

    def set_minvaldb(self, minvaldb):                       # :264-270, the GRC callbacks
        self.minvaldb = float(minvaldb)
        _lib.check(_lib.lib().fdc_waterfall_set_levels(self._h, self.minvaldb, self.maxvaldb))

    def set_maxvaldb(self, maxvaldb):
        self.maxvaldb = float(maxvaldb)
        _lib.check(_lib.lib().fdc_waterfall_set_levels(self._h, self.minvaldb, self.maxvaldb))

    def set_colorscheme(self, colorscheme):                 # :272-274
        self.colorscheme = int(colorscheme)
        _lib.check(_lib.lib().fdc_waterfall_set_colorscheme(self._h, self.colorscheme))

    def close(self):
        if self._h:
            _lib.lib().fdc_waterfall_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WaterfallImage:
    """The widget's picture (height x 1024 x 3 uint8, newest row at the bottom) and its PDU marks, without Qt.

    append(rgb_rows) scrolls rows in (python/WaterfallMsgTagging.py:166-170) and then marks the pending PDUs (:172-194); msg(meta) queues the
    metadata of a PDU — a dict with blockstart, blockend, rel_cfreq, rel_bw, e.g. the first element of a gr_fdc_amd.Sinks PDU pair — as the
    msgin handler does (:85-110).  Block counters start as the widget's do after one resize to `height` (:64-65, :112-124).

    Geometry.  The picture shows blocks (min_block, max_block].  Block b is at row  height - ceil((max_block - b) / D)  as the upper edge of a
    mark and  height - trunc((max_block - b) / D)  as its lower edge (:198-199, :214, :222); a PDU spans columns  [int(1024 (cf - bw / 2)),
    ceil(1024 (cf + bw / 2))]  (:105-106).  Three cases (:181-193):
      inside           (min_block < start, end < max_block): a closed frame, its lower edge one row up if it would fall below the picture;
      begun before     (start <= min_block): the lower edge, and the two sides up to four rows above it;
      not yet ended    (end >= max_block): the upper edge, kept for the next append (the sides below the end are outside the picture).
    Marks are clipped to the picture."""

    def __init__(self, height, blockdecimation=1, colorscheme=0):
        self.height = int(height)
        if self.height < 1:
            raise ValueError("height must be positive")
        self.D = int(blockdecimation) if int(blockdecimation) > 0 else 1
        self.frame = color_table(colorscheme)[1]
        self.min_block = -1 + (1 - self.height) * self.D
        self.max_block = 0
        self.image = np.zeros((self.height, WIDTH, 3), np.uint8)
        self.pending = []

    def msg(self, meta):
        if isinstance(meta, tuple):
            meta = meta[0]
        if not isinstance(meta, dict):
            return
        start, end = int(meta.get("blockstart", -1024)), int(meta.get("blockend", -1024))
        cf, bw = float(meta.get("rel_cfreq", -1.0)), float(meta.get("rel_bw", -1.0))
        if -1024 in (start, end) or cf < 0.0 or bw < 0.0:
            return
        self.pending.append((start, end, int(WIDTH * (cf - bw / 2.0)), int(np.ceil(WIDTH * (cf + bw / 2.0)))))

    def append(self, rgb_rows):
        new = np.asarray(rgb_rows, np.uint8).reshape(-1, WIDTH, 3)
        n = min(new.shape[0], self.height)
        if new.shape[0] == 0:
            return
        self.image = np.concatenate([self.image[n:], new[-n:]])
        self.min_block += new.shape[0] * self.D
        self.max_block += new.shape[0] * self.D
        keep = []
        for pdu in reversed(self.pending):                 # newest first, as the reference walks its list
            if self._mark(*pdu):
                keep.append(pdu)
        self.pending = keep[::-1]

    # ---- geometry
    def _upper(self, block):
        return self.height - int(np.ceil((self.max_block - block) / self.D))

    def _lower(self, block):
        return self.height - int(float(self.max_block - block) / self.D)

    def _paint(self, r0, r1, c0, c1):
        r0, r1, c0, c1 = max(r0, 0), min(r1, self.height), max(c0, 0), min(c1, WIDTH)
        if r0 < r1 and c0 < c1:
            self.image[r0:r1, c0:c1] = self.frame

    def _sides(self, r0, r1, left, right):
        self._paint(r0, r1, left, left + 1)
        self._paint(r0, r1, right, right + 1)

    def _mark(self, start, end, left, right):
        """marks one PDU; True = keep it for later"""
        if end <= self.min_block:                          # scrolled out
            return False
        if start >= self.max_block:                        # not yet on the picture
            return True
        if self.min_block < start and end < self.max_block:
            top, bottom = self._upper(start), self._lower(end)
            bottom = min(bottom, self.height - 1)
            self._sides(top, bottom, left, right)
            self._paint(top, top + 1, left, right)
            self._paint(bottom, bottom + 1, left, right)
            return False
        if start <= self.min_block:
            y = self._lower(end)
            edge = self.height - max(self.height - y, 1)
            self._paint(edge, edge + 1, left, right)
            self._sides(y - min(4, y), y, left, right)
            return False
        edge = self.height - max(self.height - self._lower(start), 1)
        self._paint(edge, edge + 1, left, right)
        y = self._lower(end)
        self._sides(y, y + min(4, self.height - y), left, right)
        return True
