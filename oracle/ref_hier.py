"""TEST INFRASTRUCTURE — the reference's hier block, python/FrequencyDomainChannelizer.py, EXECUTED to its last line.

The file is imported unmodified from where it lies, over Python stand-ins for `gnuradio.gr`, `gnuradio.blocks`, `gnuradio.fft`,
`FDC` and `pmt` that live in this module.  The stand-ins are written from GNU Radio's public interfaces and hold nothing of the
reference; `FDC.*` are the reference's own compiled blocks (oracle/_ref/libref_chain.so and libref_sinks.so behind oracle.py).
What the reference's __init__ builds and connects is recorded (constructor calls, stream edges, message edges) and then RUN by
run(): the recorded edges, item by item in topological order, from the hier block's input to its output ports.

What that pins: which blocks the hier block builds, with which arguments, in which order they are wired, which port carries
what (lines 200-315), and the three chain blocks' own work().  What it does not pin, because they are stand-ins written from
their documentation: fft_vcc (evaluated in double and rounded to float32 once, like ref_standins/gnuradio/fft/fft.h),
multiply_const_cc / _ff (a float32 multiply by gr_complex(k), as VOLK's generic kernel does it), stream_to_vector /
vector_to_stream, and the scheduler (here: whole items, one block after the other; the order of messages AMONG different sink
blocks is the scheduler's in a real flowgraph and is not modelled: PDUs are returned per block).

The reference is Python-2 code.  `round` of the imported module's namespace is Python 2's (half away from zero; py2_round of
tests/golden/make_params_from_reference.py), `/` stays Python 3's true division.

Nothing in gr-fdc_amd/ or bench.py may import this module.
"""
import contextlib
import importlib.util
import math
import os
import sys
import types

import numpy as np

import oracle as O

REF = "/root/reference/python/FrequencyDomainChannelizer.py"
_NAMES = ("gnuradio", "gnuradio.gr", "gnuradio.blocks", "gnuradio.fft", "FDC", "pmt")


def have_reference():
    return os.path.exists(REF) and O.have_ref_chain() and O.have_ref_sinks()


def py2_round(x):
    """Python 2's round(): half away from zero, decided on the fraction itself; returns float."""
    ax = abs(x)
    r = math.floor(ax)
    if ax - r >= 0.5:
        r += 1.0
    return float(r) * (1.0 if x >= 0 else -1.0)


# ---------------------------------------------------------------------------------------------------------------- gnuradio.gr
class io_signature:
    """gr.io_signature(min_streams, max_streams, sizeof_stream_item[, second item size]): what GNU Radio's make / make2 keep."""

    def __init__(self, min_streams, max_streams, *sizes):
        self.min_streams, self.max_streams, self.sizes = int(min_streams), int(max_streams), [int(s) for s in sizes]

    def sizeof_stream_item(self, port):
        """make2's rule: the last size given serves every further port"""
        return self.sizes[min(port, len(self.sizes) - 1)]


class _Recorded:
    """one constructed block: what made it, its arguments, and work(flat input array) -> flat output array"""

    def __init__(self, graph, name, args, in_size, out_size, fn=None, sink=None):
        self.name, self.args, self.in_size, self.out_size, self.fn, self.sink = name, tuple(args), in_size, out_size, fn, sink
        self.index = sum(b.name == name for b in graph.blocks)
        graph.blocks.append(self)
        graph.calls.append((name, tuple(args)))

    def label(self):
        return "%s[%d]" % (self.name, self.index)


class Graph:
    """what one construction of the hier block recorded"""

    def __init__(self):
        self.blocks, self.calls, self.edges, self.msg_edges, self.msg_ports, self.signatures = [], [], [], [], [], None


_graph = None       # the graph under construction (set by build())


class hier_block2:
    """gr.hier_block2: records connect / msg_connect / message_port_register_hier_out.  __init__ may run more than once (the
    reference calls it at :147 and again at :160); the signatures of the last call are kept."""

    def __init__(self, name, input_signature, output_signature):
        self._name = name
        _graph.signatures = (input_signature, output_signature)
        _graph.hier = self

    @staticmethod
    def _endpoint(p):
        return (p[0], int(p[1])) if isinstance(p, tuple) else (p, 0)

    def connect(self, *points):
        """connect(a, b, c, ...): each point a block (port 0) or a (block, port) pair; consecutive points are wired"""
        pts = [self._endpoint(p) for p in points]
        for a, b in zip(pts[:-1], pts[1:]):
            _graph.edges.append((a, b))

    def msg_connect(self, src, srcport, dst, dstport):
        _graph.msg_edges.append((src, srcport, dst, dstport))

    def message_port_register_hier_out(self, port_id):
        _graph.msg_ports.append(port_id)


# ---------------------------------------------------------------------------------------------------------------- gnuradio.blocks / fft
def _whole(x, per, what):
    if x.size % per:
        raise ValueError("%s: %d values are not a whole number of %d-value items" % (what, x.size, per))
    return x


def _stream_to_vector(itemsize, nitems_per_block):
    """blocks.stream_to_vector: nitems_per_block stream items become one vector item; the bytes are the same bytes"""
    return _Recorded(_graph, "stream_to_vector", (itemsize, nitems_per_block), itemsize, itemsize * nitems_per_block,
                     lambda x: _whole(x, nitems_per_block, "stream_to_vector"))


def _vector_to_stream(itemsize, nitems_per_block):
    return _Recorded(_graph, "vector_to_stream", (itemsize, nitems_per_block), itemsize * nitems_per_block, itemsize, lambda x: x)


def _multiply_const_cc(k, vlen=1):
    """blocks.multiply_const_cc(k, vlen): every sample times gr_complex(k), the full complex product in float32 in the order of
    VOLK's generic volk_32fc_s32fc_multiply_32fc (re = a.re k.re - a.im k.im, im = a.re k.im + a.im k.re), no contraction"""
    kc = np.complex64(k)

    def fn(x):
        x = np.asarray(x, dtype=np.complex64)
        re = x.real * kc.real - x.imag * kc.imag
        im = x.real * kc.imag + x.imag * kc.real
        out = np.empty(x.shape, np.complex64)
        out.real, out.imag = re, im
        return out
    return _Recorded(_graph, "multiply_const_cc", (k, vlen), 8 * vlen, 8 * vlen, fn)


def _multiply_const_ff(k, vlen=1):
    kf = np.float32(k)
    return _Recorded(_graph, "multiply_const_ff", (k, vlen), 4 * vlen, 4 * vlen, lambda x: (np.asarray(x, dtype=np.float32) * kf).astype(np.float32))


def _rectangular(ntaps):
    """fft.window.rectangular(ntaps): ntaps ones"""
    return [1.0] * int(ntaps)


def _fft_vcc(fft_size, forward, window, shift=False, nthreads=1):
    """fft.fft_vcc(fft_size, forward, window, shift, nthreads), from its documentation: an unnormalised DFT of every fft_size-sample
    item.  forward: the item is multiplied by the window (if one is given), transformed with exp(-j...), and with `shift` the
    output is arranged with DC in the middle.  Reverse: with `shift` the INPUT is taken as arranged with DC in the middle, and
    transformed with exp(+j...); the window is a forward-transform feature.  Evaluated in double, rounded to float32 once."""
    n = int(fft_size)
    win = np.asarray(window, dtype=np.float32).astype(np.float64) if window is not None and len(window) else None
    if win is not None and win.size != n:
        raise ValueError("fft_vcc: the window must have fft_size taps")
    if shift and n % 2:
        raise ValueError("fft_vcc stand-in: shift is written for even sizes")

    def fn(x):
        v = _whole(np.asarray(x, dtype=np.complex64), n, "fft_vcc").astype(np.complex128).reshape(-1, n)
        if forward:
            if win is not None:
                v = v * win
            v = np.fft.fft(v, axis=1)
            if shift:
                v = np.fft.fftshift(v, axes=1)
        else:
            if shift:
                v = np.fft.ifftshift(v, axes=1)
            v = np.fft.ifft(v, axis=1) * n
        return v.reshape(-1).astype(np.complex64)
    return _Recorded(_graph, "fft_vcc", (n, bool(forward), "rectangular" if win is not None and np.all(win == 1.0) else window, bool(shift), nthreads),
                     8 * n, 8 * n, fn)


# ---------------------------------------------------------------------------------------------------------------- FDC: the compiled reference
def _overlap_save(itemsize, outputlen, overlaplen):
    blk = O.RefOverlapSave(itemsize, outputlen, overlaplen)
    return _Recorded(_graph, "overlap_save", (itemsize, outputlen, overlaplen), itemsize * (outputlen - overlaplen), itemsize * outputlen, blk.work)


def _vector_cut_vxx(itemsize, veclen, offset, blocklen):
    blk = O.RefVectorCut(itemsize, veclen, offset, blocklen)
    return _Recorded(_graph, "vector_cut_vxx", (itemsize, veclen, offset, blocklen), itemsize * veclen, itemsize * blocklen, blk.work)


def _phase_shifting_windowing_vcc(blocklen, numphasestates, shifts, passbw, stopbw, windowtype):
    blk = O.RefPhaseWindow(blocklen, numphasestates, shifts, passbw, stopbw, windowtype)
    return _Recorded(_graph, "phase_shifting_windowing_vcc", (blocklen, numphasestates, shifts, passbw, stopbw, windowtype), 8 * blocklen, 8 * blocklen,
                     blk.work)


def _sink_flags(msg, fileoutput, verbose):
    if not msg or fileoutput or verbose:
        raise NotImplementedError("the compiled sink blocks are driven with message output on, file output off and verbose 0")


def _PowerActivationChannel(blocklen, cfreq, bw, relinvovl, thresh, maxblocks, deactivation_delay, msg, fileoutput, path, verbose, ID):
    _sink_flags(msg, fileoutput, verbose)
    blk = O.RefPowerActivationChannel(blocklen, cfreq, bw, relinvovl, thresh, maxblocks, deactivation_delay, ID)
    return _Recorded(_graph, "PowerActivationChannel", (blocklen, cfreq, bw, relinvovl, thresh, maxblocks, deactivation_delay, msg, fileoutput, path,
                                                        verbose, ID), 8 * blocklen, 0, sink=blk)


def _SegmentDetection(ID, blocklen, relinvovl, seg_start, seg_stop, thresh, minchandist, window_flank_puffer, maxblocks, deactivation_delay, msg,
                      fileoutput, path, threads, verbose):
    _sink_flags(msg, fileoutput, verbose)
    blk = O.RefSegmentDetection(ID, blocklen, relinvovl, seg_start, seg_stop, thresh, minchandist, window_flank_puffer, maxblocks, deactivation_delay,
                                threads=threads)
    return _Recorded(_graph, "SegmentDetection", (ID, blocklen, relinvovl, seg_start, seg_stop, thresh, minchandist, window_flank_puffer, maxblocks,
                                                  deactivation_delay, msg, fileoutput, path, threads, verbose), 8 * blocklen, 0, sink=blk)


def _standin_modules():
    mods = {n: types.ModuleType(n) for n in _NAMES}
    gr, blocks, fft = mods["gnuradio.gr"], mods["gnuradio.blocks"], mods["gnuradio.fft"]
    mods["gnuradio"].gr, mods["gnuradio"].blocks, mods["gnuradio"].fft = gr, blocks, fft
    gr.hier_block2, gr.io_signature = hier_block2, io_signature
    gr.io_signature_make = lambda lo, hi, size: io_signature(lo, hi, size)
    gr.io_signature_make2 = lambda lo, hi, size1, size2: io_signature(lo, hi, size1, size2)
    gr.sizeof_gr_complex, gr.sizeof_float = 8, 4
    blocks.stream_to_vector, blocks.vector_to_stream = _stream_to_vector, _vector_to_stream
    blocks.multiply_const_cc, blocks.multiply_const_ff = _multiply_const_cc, _multiply_const_ff
    fft.fft_vcc = _fft_vcc
    fft.window = types.SimpleNamespace(rectangular=_rectangular)
    f = mods["FDC"]
    f.overlap_save, f.vector_cut_vxx, f.phase_shifting_windowing_vcc = _overlap_save, _vector_cut_vxx, _phase_shifting_windowing_vcc
    f.PowerActivationChannel, f.SegmentDetection = _PowerActivationChannel, _SegmentDetection
    mods["pmt"].intern = lambda s: str(s)
    return mods


@contextlib.contextmanager
def standins_installed():
    """The stand-in modules in sys.modules for the time of the import, and whatever was there before back in place afterwards: no
    other test may find a fake gnuradio."""
    before = {n: sys.modules.get(n) for n in _NAMES}
    sys.modules.update(_standin_modules())
    try:
        yield
    finally:
        for n, m in before.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


_module = None


def reference_module():
    """python/FrequencyDomainChannelizer.py, imported once from where it lies (not entered into sys.modules), Python 2's round in its namespace"""
    global _module
    if _module is None:
        with standins_installed():
            spec = importlib.util.spec_from_file_location("ref_fdc_hier", REF)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        mod.round = py2_round
        _module = mod
    return _module


class Built:
    """One executed construction: .obj the reference's instance (channel lists, blocksize, relinvovl, inpblocklen, ...), .graph what
    it recorded."""

    def __init__(self, obj, graph):
        self.obj, self.graph = obj, graph
        self.order = _topological(graph)

    # -- what the construction decided, read off the recorded constructor calls
    def channel_params(self):
        """(f, l, lout, passbw, stopbw) per throughput channel, from the arguments the blocks were BUILT with: f and l of the first
        vector_cut_vxx, pass / stop band of the phase window, lout of the second cut (whose offset must be l - lout)"""
        cuts = [c[1] for c in self.graph.calls if c[0] == "vector_cut_vxx"]
        wins = [c[1] for c in self.graph.calls if c[0] == "phase_shifting_windowing_vcc"]
        out = []
        for i, w in enumerate(wins):
            first, second = cuts[2 * i], cuts[2 * i + 1]
            out.append((first[2], first[3], second[3], w[3], w[4]))
        return out

    def calls(self, name):
        return [c[1] for c in self.graph.calls if c[0] == name]

    def nports(self):
        return self.graph.signatures[1].max_streams

    def run(self, x, per_call=1):
        """x: the hier block's input, flat (complex64 or float32 stream items; spectrum items when inpveclen = blocksize), a whole number
        of items of the first block's vector length.  The recorded edges are run `per_call` vector items at a time (0: all at once), every
        block in topological order.  Returns (list of output ports as flat arrays, {sink label: its PDUs in its own order})."""
        g = self.graph
        insig, outsig = g.signatures
        dtype = np.float32 if insig.sizes[0] == 4 else np.complex64
        x = np.ascontiguousarray(x, dtype=dtype)
        hier = g.hier
        feeds = {}                      # (block, port) -> (source block, port)
        for (a, b) in g.edges:
            if b in feeds:
                raise ValueError("two sources on one input")
            feeds[b] = a
        nout = outsig.max_streams
        for p in range(nout):
            if (hier, p) not in feeds:
                raise ValueError("output port %d of the hier block is not connected" % p)
        if any(b[0] is hier and b[1] >= nout for b in feeds):
            raise ValueError("a connection to an output port the signature does not have")
        first = [b for (a, b) in g.edges if a[0] is hier]
        fb = first[0][0]                # one "item" of a call: a vector behind stream_to_vector, or the input item itself
        per_item = (fb.out_size if fb.name == "stream_to_vector" else fb.in_size) // np.dtype(dtype).itemsize
        _whole(x, per_item, "hier block input")
        nitems = x.size // per_item
        step = nitems if per_call <= 0 else per_call
        ports = [[] for _ in range(nout)]
        pdus = {b.label(): [] for b in g.blocks if b.sink is not None}
        # whatever source port msg_connect recorded: the stand-in blocks keep every message they publish in one list (oracle.py); a block is
        # heard when one of its message edges ends in a registered out port of the hier block
        listened = {e[0] for e in g.msg_edges if e[2] is hier and e[3] in g.msg_ports}
        for at in range(0, nitems, max(step, 1)):
            n = min(step, nitems - at)
            val = {(hier, 0): x[at * per_item:(at + n) * per_item]}
            for blk in self.order:
                src = feeds.get((blk, 0))
                if src is None:
                    raise ValueError("%s has no input" % blk.label())
                inp = val[src]
                if inp.nbytes % blk.in_size:
                    raise ValueError("item size mismatch in front of %s" % blk.label())
                if blk.sink is not None:
                    got = blk.sink.work(inp)
                    if blk in listened:
                        pdus[blk.label()] += got
                else:
                    val[(blk, 0)] = blk.fn(inp)
            for p in range(nout):
                ports[p].append(val[feeds[(hier, p)]])
        outs = [np.concatenate(p) if p else np.zeros(0, np.complex64) for p in ports]
        return outs, pdus


def _topological(g):
    hier = g.hier
    deps = {b: set() for b in g.blocks}
    for (a, b) in g.edges:
        if b[0] is not hier and a[0] is not hier:
            deps[b[0]].add(a[0])
    order, done = [], set()
    connected = {e[1][0] for e in g.edges} | {e[0][0] for e in g.edges}
    todo = [b for b in g.blocks if b in connected]
    while todo:
        ready = [b for b in todo if deps[b] <= done]
        if not ready:
            raise ValueError("the recorded graph has a cycle")
        for b in ready:
            order.append(b)
            done.add(b)
        todo = [b for b in todo if b not in done]
    return order


def build(*args):
    """FrequencyDomainChannelizer(*args) of the reference, executed to its last line.  Raises what the reference raises."""
    global _graph
    mod = reference_module()
    _graph = Graph()
    try:
        obj = mod.FrequencyDomainChannelizer(*args)
        return Built(obj, _graph)
    finally:
        _graph = None
