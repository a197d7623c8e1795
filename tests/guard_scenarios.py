"""What tests/test_guard_bands_gpu.py runs inside guard bands: a table of named scenarios in four groups.  A scenario creates its handles, makes its
calls, closes its handles, and records every describe() string and every output (as a digest of its bytes) in the Run it is given; after EVERY call, and
again after the handles are closed, Run.step() asserts that no guard byte of any live or freed allocation has changed (tests/cpp/hip_guard_alloc.c).
The file is also the child process of that test:  python guard_scenarios.py GROUP FIRST LAST [SHIM]  runs scenarios FIRST .. LAST - 1 of GROUP, plain
(no SHIM) or inside the bands under poison 0xFF and then 0x00, and prints one JSON line of digests.

Plans, streams and settings are the suite's own, imported from the test files that own them.  max_blocks is 4 unless a scenario says otherwise.  The guard
of a scenario is tests/footprint.py's guard_bytes() of one further block of its largest per-block unit, a complex64 spectrum of 8 N bytes (every other
per-block unit of a handle — H samples of the ring, sum_lout samples of d_out, N / 256 rows of d_g — is smaller), set before the handles are created.

WHICH BUFFERS EACH GROUP ALLOCATES (members of csrc/fdc_pipeline.hpp unless another file is named)

routes    every plan table of create (d_tw, d_wins, d_tw256, d_tw1024, d_twf, Bank::d_cbt / d_shn / d_slot_off / d_tab, d_tw512, d_twq512, d_tw1k, d_twq1k,
          d_t2g, d_rgroups, d_twq, d_f4rows, d_ftwq, d_fcbt, d_fshn, d_fslot, d_chans, d_groups, d_keep, d_wtasks: uploaded once, read by the kernels);
          written by kernels: d_g (the two-launch plans, and the banks' short launch groups at the default threshold), d_fscr (k_blk256's parked half), d_big (channels wider than 4096 bins), d_tmp and d_spec (the
          spectrum paths), d_ring, d_out and pin_out[2] (host entries), d_iq (work_iq), d_iqw (process_device_iq on the widening plans), d_oq (integer
          output of the host entries), d_real and d_specfull (work_real, and work with a spectrum), pin_tab (registered outputs: mapped, not banded,
          see below).
fused     d_f4rows, d_ftwq, d_fcbt, d_fshn, d_fslot of every row class of k_f4096, with d_ring / d_out / pin_out.
tail      d_carry[2], d_ataps, d_ahist[2], d_aoff, d_audio / pin_audio, d_sqthr[2], d_sqstate[2], d_mask / pin_mask, d_packoff, d_packtotal /
          pin_packtotal, d_tinc, d_ttab, d_tcarry[2], d_tones / pin_tones, d_tsqtone, d_tsqthr[3], d_tsqstate[2], d_tdec / pin_tdec; the regrow scenario
          frees and reallocates the ones set_audio, set_tones and set_tone_squelch size (their old blocks are checked at the free).
around    csrc/fdc_sinks_state.hpp: d_spec, d_wins, d_tw, d_tw256, d_cells, d_power and d_gpow of a bank, d_spec_ahead / d_power_ahead / d_gpow_ahead of
          a look-ahead bank fed by Pipeline.work(x, sinks=...), d_wide (an 8192-bin extraction); the host engine's d_tasks, d_ext, h_ext; the device
          engine's Dev members (d_task_base ... d_sorted, d_sum / h_sum, h_pdus, d_land[2] / h_land[2], and d_nland[2] / h_nland[2] with sc16 payloads);
          the members of a SinksGroup.  csrc/fdc_group.hip: the members of a PipelineGroup and its pinned staging.  csrc/fdc_waterfall.hip: the raw
          allocations d_edges, d_table, d_blk, d_carry[2], d_rows, d_index, d_rgb, d_pow (Waterfall.work) and d_gpow (Pipeline.work_waterfall on a plan
          that sums 16-bin groups; d_specfull is the spectrum there).  csrc/fdc_faces.hip: d_ring / d_out of overlap_save (and nr / no while it grows,
          over calls of 2, 5 and 3 items), d_in / d_out of vector_cut, d_win / d_in / d_out of phase_window, d_in / d_out / d_tmp / d_tw of
          fdc_fft_vcc's cache.  The hier block's pipeline with the whole tail on.

NOT REACHED, and why
* d_lag1 / pin_lag1, d_gain, d_fine, d_f4fine, d_fstep (set_lag1, set_gains, set_fine_tuning): the group that ran levels, lag-1, gains and fine tuning
  over every cut of a nine-block stream passed three times on its own and then ended in trouble once inside a run of the whole suite (a signal, its
  time limit or an illegal-address text: the output of that run was lost).  The cause was not found, so the group is left out until it is; d_levels /
  pin_levels are reached by `tail`, which has the levels on throughout.
* pin_tab (MappedBuf) is hipHostMallocMapped: the shim passes every flag but hipHostMallocDefault through (the library takes the table's device
  address), so the scatter table has no bands.  The scatter kernels that read it run in `routes` (registered outputs); their stores go to the caller's
  arrays, which tests/test_footprint_gpu.py bands.
* The timing events vector and the streams are not memory a kernel writes.
* fdc_fft_vcc's cache lives as long as the process: its guards are checked after every call, never at a free.
* The multi-device form of the two groups is run on one device twice (devices [0, 0]), as the suite runs it.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Run:
    """one pass over some scenarios: plain (shim None) or inside the bands under one poison byte"""

    def __init__(self, shim=None, poison=None):
        self.shim, self.poison = shim, poison
        self.items = {}
        self.scenario = ""
        self.first_counts = None

    def guard(self, block_bytes):
        """before a scenario creates its handles: guards of one further block of block_bytes (at least 64 KiB, a multiple of 256)"""
        import footprint as F
        if self.shim is not None:
            self.shim.set(F.guard_bytes(block_bytes), self.poison)

    def step(self, what, *handles):
        """after a call: no guard byte of any allocation, live or freed, has changed"""
        if self.shim is None:
            return
        if self.first_counts is None:
            self.first_counts = self.shim.counts()
        total, first, text = self.shim.check()
        if total != 0:
            d = "; ".join(h.describe() for h in handles if hasattr(h, "describe"))
            raise AssertionError("GUARD %s: %s, poison 0x%02X: %d guard bytes (status -1: the runtime refused a copy); %s [ordinal, payload bytes, first, "
                                 "last, count = %r]; %s" % (self.scenario, what, self.poison, total, text, first, d))

    def out(self, name, value):
        """an output of the scenario: an array, a list of arrays, a string, or a list of PDUs (meta, samples)"""
        key = "%s: %s" % (self.scenario, name)
        assert key not in self.items, key
        h = hashlib.sha1()
        feed(h, value)
        self.items[key] = h.hexdigest()

    def done(self, what, handle, value):
        """the usual end of a call: guards, then the outputs and the handle's describe()"""
        self.step(what, handle)
        self.out(what, value)
        if hasattr(handle, "describe"):
            self.out(what + ": describe", handle.describe())


def feed(h, v):
    if isinstance(v, str):
        h.update(v.encode())
    elif isinstance(v, np.ndarray):
        h.update(("%s%r" % (v.dtype.str, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, dict):
        h.update(repr(sorted(v.items())).encode())
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d" % len(v))
        for a in v:
            feed(h, a)
    elif v is None:
        h.update(b"None")
    else:
        h.update(repr(v).encode())


# ---- the suite's tables (imported when the child runs, behind the shim) -------------------------------------------------------------------------------------

def suite():
    """the test modules the scenarios borrow from, imported once (they import pytest and the package, nothing of the device)"""
    global G, F, FP, TT, TS, FR
    import gr_fdc_amd as G
    G.defaults.setdefault("FDC_BLOCK_MIN_BLOCKS", "1")          # as tests/conftest.py: the block kernels at any block count
    import footprint as F
    import test_footprint_gpu as FP
    import test_tones_gpu as TT
    import test_tone_squelch_gpu as TS
    import test_fine_tuning_routes_gpu as FR
    return G


def device_call(run, dev, p, x, nb, what, fmt=None, in_fmt=None, spectrum=False, first=0):
    """process_device / process_device_iq of nb blocks from block `first` of the stream x on a ring and a d_out of the test's own (exact size)"""
    per = 2 if in_fmt else 1
    ring = np.concatenate([np.zeros(per * p.ovl, x.dtype), x])[per * first * p.H:per * ((first + nb) * p.H + p.ovl)] if first else FP.ring_of(x, nb, p, in_fmt)[0]
    ssz = FP.SAMPLE_BYTES[fmt]
    n = p.output_samples(nb)
    d_ring, d_out = dev.put(np.ascontiguousarray(ring)), dev.put(np.zeros(n * ssz, np.uint8))
    d_spec = dev.put(np.zeros(8 * nb * p.N, np.uint8)) if spectrum else None
    if in_fmt:
        p.process_device_iq(in_fmt, FP.IN_SCALE[in_fmt], d_ring, first, nb, d_out, d_spec)
    else:
        p.process_device(d_ring, first, nb, d_out, d_spec)
    p.synchronize()
    got = [dev.get(d_out, n * ssz, np.uint8)]
    if spectrum:
        got.append(dev.get(d_spec, 8 * nb * p.N, np.uint8))
    run.done(what, p, got)
    return got


# ---- a. routes ----------------------------------------------------------------------------------------------------------------------------------------------

def route_plan(k):
    def scenario(run):
        case = FP.PLANS[k]
        name, N, R, chans, flags, _r_in, keep = case
        run.guard(8 * N)
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=4, flags=flags, keep_spectrum=keep)
        H = p.H
        counts = FP.float_counts(N)
        x = FP.signal(max(counts) * H, 700 + k)
        with FR.DeviceBuffers() as dev:
            # float in, float out: the host entry (nblocks <= max_blocks) and the device entry
            first = None
            for nb in (1, 3, 4):
                p.reset()
                o = p.work(x[:nb * H])
                first = first or o
                run.done("work, %d blocks" % nb, p, o)
            for nb in counts:
                device_call(run, dev, p, x, nb, "process_device, %d blocks" % nb)
            # integer output alone on float input
            p.set_output_format("sc16", FR.int_scale(first, np.int16))
            p.reset()
            run.done("work, sc16 out, 4 blocks", p, p.work(x[:4 * H]))
            for nb in (1, 3, 4):
                device_call(run, dev, p, x, nb, "process_device, sc16 out, %d blocks" % nb, fmt="sc16")
            # integer input with the matching integer output: sc16 on every plan, sc8 where the kernels read the integers in their own loads
            for in_fmt in ("sc16", "sc8") if FP.input_route(case) == "fused" else ("sc16",):
                xi = FP.iq(4 * H, FP.ODT[in_fmt], 100 + k)
                p.set_output_format(None)
                p.reset()
                o = p.work_iq(xi[:2 * H], scale=FP.IN_SCALE[in_fmt])
                run.done("work_iq %s, float out, 1 block" % in_fmt, p, o)
                device_call(run, dev, p, xi, 3, "process_device_iq %s, float out, 3 blocks" % in_fmt, in_fmt=in_fmt)
                p.set_output_format(in_fmt, FR.int_scale(o, FP.ODT[in_fmt]))
                for nb in (1, 3, 4):
                    p.reset()
                    run.done("work_iq %s, %s out, %d blocks" % (in_fmt, in_fmt, nb), p, p.work_iq(xi[:2 * nb * H], scale=FP.IN_SCALE[in_fmt]))
                    device_call(run, dev, p, xi, nb, "process_device_iq %s, %s out, %d blocks" % (in_fmt, in_fmt, nb), fmt=in_fmt, in_fmt=in_fmt)
        p.close()
        run.step("closed")
    return "route: " + FP.PLANS[k][0], scenario


def chunked(j):
    def scenario(run):
        name, N, R, chans, flags, _r_in, keep = FP.CHUNKED[j]
        run.guard(8 * N)
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=5, chunk_blocks=2, flags=flags, keep_spectrum=keep)
        assert p.chunk_blocks() == 2
        x = FP.signal(5 * p.H, 750 + j)
        run.done("work, 5 blocks", p, p.work(x))
        with FR.DeviceBuffers() as dev:
            device_call(run, dev, p, x, 5, "process_device, 5 blocks")
        p.close()
        run.step("closed")
    return "launch groups of two: " + FP.CHUNKED[j][0], scenario


def work_real(j):
    def scenario(run):
        name, N, chans = FP.HOST_PLANS[j]
        run.guard(8 * N)
        p = G.Pipeline(N, 2, chans, max_blocks=5)
        xr = FP.signal(5 * p.H, 620 + j).real.copy()
        o = p.work_real(xr)
        run.done("work_real", p, o)
        p.set_output_format("sc16", FR.int_scale(o, np.int16))
        p.reset()
        run.done("work_real, sc16 out", p, p.work_real(xr))
        p.close()
        q = G.Pipeline(N, 2, chans, max_blocks=5, keep_spectrum=True)
        run.done("work_real with a spectrum", q, list(q.work_real(xr, want_spectrum=True)))
        q.close()
        run.step("closed")
    return "work_real: " + FP.HOST_PLANS[j][0], scenario


def with_spectrum(j):
    def scenario(run):
        name, N, R, chans, flags, _r_in, _keep = FP.KEEP[j]
        run.guard(8 * N)
        p = G.Pipeline(N, R, chans, windowtype=1, max_blocks=4, flags=flags, keep_spectrum=True)
        x = FP.signal(5 * p.H, 500)
        for nb in (1, 3, 4):
            p.reset()
            run.done("work with a spectrum, %d blocks" % nb, p, list(p.work(x[:nb * p.H], want_spectrum=True)))
        with FR.DeviceBuffers() as dev:
            for nb in (1, 3, 5):
                device_call(run, dev, p, x, nb, "process_device with a spectrum, %d blocks" % nb, spectrum=True)
        p.close()
        run.step("closed")
    return "spectrum: " + FP.KEEP[j][0], scenario


def short_groups(j):
    """the library's default threshold (min_block_launch = 96; the suite runs with 1): launch groups of 1 to 9 blocks of a uniform bank take the two-launch
    form through the scratch d_g (stage 1 + stage 2; the generic pair for another width, the specialised stage 2 at N = 65536), or, with keep_spectrum,
    the tiled forward transform and the pass over the spectrum"""
    def scenario(run):
        name, N, chans, keep = SHORT[j]
        run.guard(8 * N)
        p = G.Pipeline(N, 2, chans, windowtype=1, max_blocks=4, min_block_launch=96, keep_spectrum=keep)
        x = FP.signal(9 * p.H, 760 + j)
        for nb in (1, 3, 4):
            p.reset()
            run.done("work, %d blocks" % nb, p, list(p.work(x[:nb * p.H], want_spectrum=True)) if keep else p.work(x[:nb * p.H]))
        with FR.DeviceBuffers() as dev:
            for nb in FP.float_counts(N):
                device_call(run, dev, p, x, nb, "process_device, %d blocks" % nb, spectrum=keep)
        p.close()
        run.step("closed")
    return "short launch groups at the default threshold: " + SHORT[j][0], scenario


def spectrum_items(run):
    """a plan that takes spectrum items: d_specfull is the whole-call spectrum where no sink bank's buffer takes it"""
    N, R, nb = 4096, 2, 4
    run.guard(8 * N)
    p = G.Pipeline(N, R, FP.EXAMPLE, max_blocks=nb, keep_spectrum=True)
    items = FP.signal(nb * N, 77)
    run.done("work_spectrum", p, list(p.work_spectrum(items, want_spectrum=True)))
    p.close()
    run.step("closed")


def registered(j):
    def scenario(run):
        name, N, chans = FP.HOST_PLANS[j]
        run.guard(8 * N)
        for sub in (0, 2):
            p = G.Pipeline(N, 2, chans, max_blocks=5, host_sub_blocks=sub or None)
            x = FP.signal(5 * p.H, 600 + j)
            scale = FR.int_scale(p.work(x), np.int16)
            for fmt in (None, "sc16"):
                p.set_output_format(fmt, scale)
                outs = [np.zeros((5 * lo, 2), np.int16) if fmt else np.zeros(5 * lo, np.complex64) for lo in p.lout]
                for o in outs:
                    G.register_host(o)
                try:
                    p.reset()
                    p.work(x, outs=outs)
                    run.done("registered outs, %s, sub-batches of %d" % (fmt or "fc32", sub), p, outs)
                finally:
                    for o in outs:
                        G.unregister_host(o)
            p.close()
        run.step("closed")
    return "registered outputs: " + FP.HOST_PLANS[j][0], scenario


def sub_batches(run):
    """the handle's own sub-batch rule (csrc/fdc_work.hip, work_io_setup: 8 MiB of input, 512 blocks at H = 2048): 1025 blocks are 512 + 512 + 1"""
    N, R, nb = 4096, 2, 1025
    run.guard(8 * N)
    p = G.Pipeline(N, R, FP.EXAMPLE, max_blocks=nb)
    assert (8 << 20) // (8 * p.H) == 512
    x = FP.signal(nb * p.H, 640)
    run.done("work, 1025 blocks", p, p.work(x))
    p.close()
    run.step("closed")


# ---- b. the row classes of the one-launch kernel --------------------------------------------------------------------------------------------------------

def fused(k, R):
    def scenario(run):
        name, chans = FP.F4[k]
        run.guard(8 * 4096)
        p = G.Pipeline(4096, R, chans, windowtype=1, max_blocks=4)
        x = FP.signal(5 * p.H, 200 + k + R)
        with FR.DeviceBuffers() as dev:
            for nb in (1, 2, 5):
                if nb <= 4:
                    p.reset()
                    run.done("work, %d blocks" % nb, p, p.work(x[:nb * p.H]))
                device_call(run, dev, p, x, nb, "process_device, %d blocks" % nb)
        p.close()
        run.step("closed")
    return "k_f4096, R = %d: %s" % (R, FP.F4[k][0]), scenario


# ---- c. the cuts of a handle's calls the tail scenarios share ------------------------------------------------------------------------------------------

HANDLE_KW = (dict(host_sub_blocks=2), dict(chunk_blocks=2), dict(chunk_blocks=2, host_sub_blocks=3))


# ---- d. the demodulation tail ------------------------------------------------------------------------------------------------------------------------------

AUDIO = [(8, 64, "f32"), (1, 256, "s16"), (64, 1, "f32"), (8, 64, "s16"), (1, 256, "f32"), (64, 1, "s16")]     # (D, K) of the issue in both formats
TAIL_CUTS = ((9,), (4, 5), (1, 1, 7), (3, 3, 3))


def audio_args(j):
    D, K, fmt = AUDIO[j % len(AUDIO)]
    taps = G.lowpass_taps(D, K) if K > 1 else np.array([0.75], np.float32)
    return (D, taps, fmt, 9000.0 if fmt == "s16" else 1.0)


def tail_outputs(p, nb, o, packed, tones, tsq):
    got = [o, p.levels(nb), p.squelch(nb) if p.squelch_setting() is not None else None]
    if p.audio_setting() is not None:
        got.append(p.audio_packed(nb) if packed else p.audio(nb))
    if tones:
        got.append(p.tones(nb))
    if tsq:
        got.append(p.tone_squelch(nb))
    return got


def demod_alone(k):
    def scenario(run):
        name, N, chans, flags = TT.PLANS[k]
        run.guard(8 * N)
        H = N - N // 2
        x = TT.ports(k, "fm")[0]
        for mode, gain in TT.MODES.items():
            for cut in ((9,), (4, 5)):
                p = G.Pipeline(N, 2, chans, max_blocks=TT.NB, flags=flags)
                p.set_demod(mode, gain)
                b0 = 0
                for n in cut:
                    run.done("%s, cut %r at %d" % (mode, cut, b0), p, p.work(x[b0 * H:(b0 + n) * H]))
                    b0 += n
                p.close()
        run.step("closed")
    return "demodulation: " + TT.PLANS[k][0], scenario


def squelched_audio(k, j):
    """the audio behind the carrier squelch, gated and packed, hang 0 and 3 (no tones)"""
    def scenario(run):
        name, N, chans, flags = TT.PLANS[k]
        run.guard(8 * N)
        H = N - N // 2
        T, S, W = TS.SETTINGS[1]
        x, _Z, _cm, thr_o, thr_c = TS.base(k, T, S, W)[:5]
        for hang in (0, 3):
            for packed in (False, True):
                p = TS.plain(k, T, S, W, tones=False, audio=audio_args(j))
                p.set_squelch(thr_o, thr_c, hang)
                if packed:
                    p.set_audio_packing(True)
                b0 = 0
                for n in (4, 5):
                    o = p.work(x[b0 * H:(b0 + n) * H])
                    run.step("hang %d, packed %r, call at %d" % (hang, packed, b0), p)
                    run.out("hang %d, packed %r, call at %d" % (hang, packed, b0), tail_outputs(p, n, o, packed, False, False))
                    b0 += n
                run.out("hang %d, packed %r: describe" % (hang, packed), p.describe())
                p.close()
        run.step("closed")
    return "audio D %d K %d %s behind the squelch: %s" % (AUDIO[j][:3] + (TT.PLANS[k][0],)), scenario


def tone_squelched(k, t):
    """toned() handles: everything on.  Cuts with calls shorter than a frame and calls that end inside one"""
    def scenario(run):
        name, N, chans, flags = TT.PLANS[k]
        run.guard(8 * N)
        H = N - N // 2
        T, S, W = TS.SETTINGS[t]
        x = TS.base(k, T, S, W)[0]
        j = 2 * (3 * k + t)
        for hang in (0, 3):
            for packed in (False, True):
                for cut in TAIL_CUTS:
                    p = TS.toned(k, T, S, W, hang, audio=audio_args(j), packed=packed)
                    b0 = 0
                    for n in cut:
                        o = p.work(x[b0 * H:(b0 + n) * H])
                        tag = "hang %d, packed %r, cut %r at %d" % (hang, packed, cut, b0)
                        run.step(tag, p)
                        run.out(tag, tail_outputs(p, n, o, packed, True, True))
                        b0 += n
                    run.out("hang %d, packed %r, cut %r: describe" % (hang, packed, cut), p.describe())
                    p.close()
                j += 1
        for kw in HANDLE_KW:
            p = TS.toned(k, T, S, W, 1, audio=audio_args(j), **kw)
            for b0, n in ((0, 4), (4, 5)):
                o = p.work(x[b0 * H:(b0 + n) * H])
                run.step("%r at %d" % (kw, b0), p)
                run.out("%r at %d" % (kw, b0), tail_outputs(p, n, o, False, True, True))
            p.close()
        run.step("closed")
    return "tone squelch T%d S%d W%d: %s" % (TS.SETTINGS[t] + (TT.PLANS[k][0],)), scenario


def tail_device(k):
    """the device entries as test_tone_squelch_gpu.test_device_entries makes them, with the audio on: the handle's device buffers read back"""
    def scenario(run):
        name, N, chans, flags = TT.PLANS[k]
        run.guard(8 * N)
        H, ovl = N - N // 2, N // 2
        T, S, W = TS.SETTINGS[1]
        x = TS.base(k, T, S, W)[0]
        for j in (0, 3):
            p = TS.toned(k, T, S, W, 1, audio=audio_args(j))
            A = sum(lo // AUDIO[j][0] for lo in p.lout)
            with FR.DeviceBuffers() as dev:
                for call, (first, n) in enumerate(((0, 3), (3, 4), (4, 3), (4, 3))):
                    ring = np.concatenate([np.zeros(ovl, np.complex64), x])
                    d_in = dev.put(np.ascontiguousarray(ring[first * H:first * H + ovl + n * H]))
                    d_o = dev.put(np.zeros(p.output_samples(n), np.float32))
                    p.process_device(d_in, first, n, d_o)
                    p.synchronize()
                    tag = "%s: process_device call %d" % (AUDIO[j][2], call)
                    run.step(tag, p)
                    got = tail_outputs(p, n, dev.get(d_o, p.output_samples(n), np.float32), False, True, True)
                    got.append(dev.get(C.c_void_p(p.squelch_device()), n * len(chans), np.uint8))
                    got.append(dev.get(C.c_void_p(p.audio_device()), n * A * (2 if AUDIO[j][2] == "s16" else 4), np.uint8))
                    nf = p.tones(n).shape[0]
                    if nf:
                        got.append(dev.get(C.c_void_p(p.tones_device()), nf * len(chans) * T, np.complex64))
                        got.append(dev.get(C.c_void_p(p.tone_squelch_device()), nf * len(chans), np.uint8))
                    run.out(tag, got)
            run.out("%s: describe" % AUDIO[j][2], p.describe())
            p.close()
        run.step("closed")
    return "device entries with the tail on: " + TT.PLANS[k][0], scenario


def regrow(k):
    """settings changed to larger sizes on a live handle: more taps, a smaller decimation (a longer audio row), more tones, a longer frame, then smaller
    again: the buffers sized by the setters are freed and made anew, the old blocks are checked at their free"""
    def scenario(run):
        name, N, chans, flags = TT.PLANS[k]
        run.guard(8 * N)
        H = N - N // 2
        x, _Z, _cm, thr_o, thr_c, tone, o_thr, c_thr, ratio = TS.base(k, *TS.SETTINGS[1])
        p = TS.plain(k, 7, 8, 2, audio=(64, np.array([0.75], np.float32)))
        p.set_squelch(thr_o, thr_c, 1)
        steps = [("as made", None),
                 ("more taps", lambda: p.set_audio(64, G.lowpass_taps(64, 32))),
                 ("a longer audio row", lambda: p.set_audio(8, G.lowpass_taps(8, 64), "s16", 9000.0)),
                 ("packed", lambda: p.set_audio_packing(True)),
                 ("more tones", lambda: p.set_tones(TT.increments(len(chans), 50, 16), 16, 2)),
                 ("the tone squelch", lambda: p.set_tone_squelch(np.minimum(tone, 6), o_thr, c_thr, ratio, 1, 1)),
                 ("the most tones, a frame of one block", lambda: (p.set_tone_squelch(None), p.set_tones(TT.increments(len(chans), 64, 64), 64, 1),
                                                                   p.set_tone_squelch(tone, o_thr, c_thr, ratio, 1, 3))),
                 ("the longest row", lambda: p.set_audio(1, G.lowpass_taps(1, 256))),
                 ("a longer frame", lambda: (p.set_tone_squelch(None), p.set_tones(TT.increments(len(chans), 64, 64), 64, 4),
                                             p.set_tone_squelch(tone, o_thr, c_thr, ratio, 0, 0))),
                 ("small again", lambda: (p.set_audio_packing(False), p.set_audio(64, np.array([0.75], np.float32)), p.set_tone_squelch(None),
                                          p.set_tones(TT.increments(len(chans), 7, 8), 8, 2)))]
        for what, change in steps:
            if change:
                change()
                run.step(what + ": the setters", p)
            p.reset()
            for b0, n in ((0, 4), (4, 5)):
                o = p.work(x[b0 * H:(b0 + n) * H])
                run.step("%s, call at %d" % (what, b0), p)
                run.out("%s, call at %d" % (what, b0), tail_outputs(p, n, o, p.audio_packing(), True, p.tone_squelch_setting() is not None))
            run.out(what + ": describe", p.describe())
        p.close()
        run.step("closed")
    return "settings that grow on a live handle: " + TT.PLANS[k][0], scenario


# ---- e. around the pipeline ------------------------------------------------------------------------------------------------------------------------------------

NO_ALLOC_PLAN = [(301, 64, 0.6, 0.85), (0, 256, 0.8, 1.0), (1024 + 7, 512, 0.8, 0.95)]                     # tests/test_no_alloc_gpu.py
SINKS_KW = dict(pac=[(0.3, 0.04, 0)], pac_thresh=6.0, pac_maxblocks=3, segments=[(0.55, 0.9)], det_thresh=10.0, det_maxblocks=3, minchandist=0.01)


def no_alloc_stream(nb, H):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(nb * H) + 1j * rng.standard_normal(nb * H)).astype(np.complex64)
    n = np.arange(nb * H)
    x += (np.exp(2j * np.pi * -0.2 * n) * (n > 2 * H) * (n < 6 * H)).astype(np.complex64)
    return x, (rng.standard_normal(nb * 4096) + 1j * rng.standard_normal(nb * 4096)).astype(np.complex64)


def pdus(b):
    """(meta, samples) of every PDU, the wall-clock stamp taken out of "id": the library names a PDU "<date and time of the bank's creation>.<block>.
    <source>.<number>", so two plain children started a second apart already disagree in it (seen on the MI355X: ids 2026-...-22.PowActChan.0.1 and
    ...-23.PowActChan.0.1 from two plain runs, every other field and every payload equal).  Everything behind the stamp stays in the comparison."""
    out = []
    for m, s in b:
        m = dict(m)
        stamp, _, rest = m["id"].partition(".")
        assert rest and len(stamp) == len("2000-01-01-00-00-00") and stamp.replace("-", "").isdigit(), m["id"]
        m["id"] = rest
        out.append((m, np.asarray(s)))
    return out


def sinks(run):
    N, R, nb = 4096, 2, 8
    run.guard(8 * N)
    x, spec_items = no_alloc_stream(nb, N - N // R)
    for lookahead in (False, True):
        p, b = G.Pipeline(N, R, NO_ALLOC_PLAN, max_blocks=nb, keep_spectrum=True), G.Sinks(N, R, lookahead=lookahead, max_blocks=nb, **SINKS_KW)
        tag = "pipelined" if lookahead else "serial"
        for call in range(3):
            o = p.work(x, sinks=b)
            run.step("%s, call %d" % (tag, call), p)
            run.out("%s, call %d" % (tag, call), [o, pdus(b.pdus())])
        flushed = []
        while p.flush_sinks(b) > 0:
            run.step(tag + ", flush", p)
            flushed.append(pdus(b.pdus()))
        run.out(tag + ", flushed", flushed)
        run.out(tag + ": describe", p.describe())
        p.close()
        b.close()
    # a bank and a group of two members on the mixed plan of tests/test_sinks_group_gpu.py, carriers keyed on and off
    from test_sinks_group_gpu import onoff_spectrum
    plan = [((c + 0.5) / 40 * 0.45 + 0.02, 0.006, c) for c in range(20)]
    segs = [(0.55, 0.70), (0.75, 0.95)]
    carriers = [(int(round((cf - bw / 2) * N)), int(round((cf + bw / 2) * N))) for (cf, bw, _i) in plan]
    carriers += [(int(0.58 * N), int(0.60 * N)), (int(0.64 * N), int(0.66 * N)), (int(0.8 * N), int(0.83 * N)), (int(0.9 * N), int(0.91 * N))]
    spec = np.ascontiguousarray(onoff_spectrum(N, 3 * nb, carriers, 77)).reshape(-1)
    kw = dict(pac=plan, pac_thresh=6.0, pac_maxblocks=4, segments=segs, det_thresh=10.0, det_maxblocks=3, minchandist=0.005, det_delay=1, puffer=0.2, max_blocks=nb)
    b = G.Sinks(N, R, **kw)
    g = G.SinksGroup(N, R, [0, 0], **kw)
    for call in range(3):
        for name, h in (("Sinks.work", b), ("SinksGroup.work", g)):
            got = pdus(h.work(spec[call * nb * N:(call + 1) * nb * N]))
            run.step("%s, call %d" % (name, call))
            run.out("%s, call %d" % (name, call), got)
    run.out("Sinks.work on spectrum items", pdus(b.work(spec_items * 1e-3)))
    run.step("Sinks.work on spectrum items")
    b.close()
    # the host engine (d_tasks, d_ext, h_ext) and sc16 payloads of the device engine (d_nland / h_nland)
    host = G.Sinks(N, R, host_decisions=True, **kw)
    narrow = G.Sinks(N, R, **kw)
    narrow.set_payload_format("sc16", 100.0)
    for call in range(3):
        for name, h in (("host engine", host), ("sc16 payloads", narrow)):
            got = pdus(h.work(spec[call * nb * N:(call + 1) * nb * N]))
            run.step("%s, call %d" % (name, call))
            run.out("%s, call %d" % (name, call), got)
    host.close()
    narrow.close()
    g.close()
    run.step("closed")


def sinks_wide(run):
    """an extraction wider than 4096 points (d_wide, between the two passes of its transform): one PowerActivationChannel of 0.4 of the band at N = 16384
    is cut out 8192 bins wide; both engines"""
    from test_sinks_engines_gpu import onoff_spectrum
    N, R, nb = 16384, 2, 6
    run.guard(8 * N)
    spec = np.ascontiguousarray(onoff_spectrum(N, 2 * nb, [(int(0.31 * N), int(0.69 * N))], 5)).reshape(-1)
    for name, host in (("device engine", False), ("host engine", True)):
        b = G.Sinks(N, R, pac=[(0.5, 0.4, 0)], pac_thresh=6.0, pac_maxblocks=2, max_blocks=nb, host_decisions=host)
        got = []
        for call in range(2):
            got.append(pdus(b.work(spec[call * nb * N:(call + 1) * nb * N])))
            run.step("%s, call %d" % (name, call))
        assert any(m["vectorend"] - m["vectorstart"] == 8192 and smp.size for c in got for m, smp in c), [m for c in got for m, _ in c]
        run.out(name, got)
        b.close()
    run.step("closed")


def pipeline_group(run):
    N, R, nb = 4096, 2, 8
    run.guard(8 * N)
    x, _ = no_alloc_stream(nb, N - N // R)
    g = G.PipelineGroup(N, R, FP.EXAMPLE, devices=[0, 0], max_blocks=nb, min_span_blocks=2)
    g.set_levels(True)
    g.set_lag1(True)
    for call in range(2):
        o = g.work(x)
        run.step("PipelineGroup.work, call %d" % call)
        run.out("PipelineGroup.work, call %d" % call, [o, g.levels(), g.lag1()])
    g.set_levels(False)
    g.set_lag1(False)
    g.set_output_format("sc16", 1000.0)
    g.reset()
    o = g.work(x)
    run.step("PipelineGroup.work, sc16 out")
    run.out("PipelineGroup.work, sc16 out", o)
    g.close()
    run.step("closed")


def waterfalls(run):
    from waterfall_model import power_stream
    nb = FP.WF_CALLS[0]
    for name, N, R, chans, _words in FP.WF_PLANS:
        run.guard(8 * N)
        p = G.Pipeline(N, R, chans, max_blocks=nb)
        w = G.Waterfall(N, 1e6, R, FP.WF_D, 0, *FP.LEVELS, 0, 0, max_items=nb)
        x = FP.signal(sum(FP.WF_CALLS) * p.H, 630)
        for call in range(len(FP.WF_CALLS)):
            o, rows = p.work_waterfall(np.ascontiguousarray(x[call * nb * p.H:(call + 1) * nb * p.H]), w)
            run.step("%s, call %d" % (name, call), p)
            run.out("%s, call %d" % (name, call), [o, list(rows)])
        run.out(name + ": describe", p.describe())
        p.close()
        w.close()
    for N in (512, 4096):
        run.guard(8 * N)
        pw = power_stream(sum(FP.WF_CALLS), N, seed=N)
        w = G.Waterfall(N, 1e6, 4, FP.WF_D, 0, *FP.LEVELS, 1, 0, max_items=3)
        for call in range(len(FP.WF_CALLS)):
            rows = w.work(pw[call * nb:(call + 1) * nb].reshape(-1))
            run.step("Waterfall.work N = %d, call %d" % (N, call))
            run.out("Waterfall.work N = %d, call %d" % (N, call), list(rows))
        w.close()
    run.step("closed")


def faces(run):
    run.guard(8 * 4096)
    fin = FP.signal(16 * 1024, 7)
    for call in range(2):
        got = G.fft_vcc(1024, True, True, fin)
        run.step("fdc_fft_vcc, call %d" % call)
        run.out("fdc_fft_vcc, call %d" % call, got)
    got = G.fft_vcc(4096, False, False, fin)
    run.step("fdc_fft_vcc, 4096 backward")
    run.out("fdc_fft_vcc, 4096 backward", got)
    made = {"overlap_save": (lambda: G.overlap_save(8, 4096, 2048), 2 * 2048, np.float32),
            "vector_cut": (lambda: G.vector_cut_vxx(8, 4096, 2413, 256), 2 * 4096, np.float32),
            "phase_window": (lambda: G.phase_shifting_windowing_vcc(256, 2, 1, 0.88, 1.0, 1), 256, np.complex64)}
    for name, (make, values, dtype) in made.items():
        b = make()
        at = 0
        for n in (2, 5, 3):                                     # grows once, then a call that fits (tests/test_handle_memory_gpu.py)
            a = np.arange(at, at + n * values).astype(dtype)
            if dtype is np.complex64:
                a = (a * (1 - 0.5j)).astype(np.complex64)
            got = b.work(a)
            run.step("%s, %d items" % (name, n))
            run.out("%s, %d items at %d" % (name, n, at), got)
            at += n * values
        b.close()
    run.step("closed")


def hier_block(run):
    """FrequencyDomainChannelizer with the tone-squelch keywords on, as tests/test_tone_squelch_gpu.py::test_hier_block makes it"""
    from test_demod_gpu import CYCLES, KW
    from test_fine_tuning_gpu import signal
    N, R, nb = 4096, 2, 6
    run.guard(8 * N)
    H = N - N // R
    x = signal(2 * nb * H, 11)
    S, W = 16, 2
    inc1 = G.tone_increments(G.ctcss_tones(), 25000.0, S)
    common = dict(inptype=8, demod="fm", demod_gain=CYCLES, levels=True, squelch_db=-60.0, squelch_hang=1, tones=inc1, tone_group=S, tone_frame=W)
    tone = np.array([3, -1, 40], np.int32)
    on = G.FrequencyDomainChannelizer(tone_squelch=tone, tone_open=1e-3, tone_close=5e-4, tone_ratio=0.0, tone_guard=2, tone_hang=1, **common, **KW)
    for call, xs in enumerate((x[:nb * H], x[nb * H:], x[:0])):
        o = on.work(xs)
        run.step("hier block, call %d" % call, on.pipeline)
        run.out("hier block, call %d" % call, [list(o), on.levels, on.squelch, on.tones, on.tone_squelch_dec])
    run.out("hier block: describe", on.pipeline.describe())
    on.pipeline.close()
    run.step("closed")


def groups():
    """{group: [(name, scenario)]}; needs suite()"""
    routes = [route_plan(k) for k in range(len(FP.PLANS))]
    routes += [chunked(j) for j in range(len(FP.CHUNKED))] + [work_real(j) for j in range(len(FP.HOST_PLANS))]
    routes += [with_spectrum(j) for j in range(2)] + [("spectrum items on a plan without a sink bank", spectrum_items)]
    global SHORT
    SHORT = [(c[0], c[1], c[3], False) for c in (FP.PLANS[0],)] + [(k + " bank", N, chans, False) for k, N, chans in FP.PERSISTENT]
    SHORT.append((FP.KEEP[2][0], FP.KEEP[2][1], FP.KEEP[2][3], True))
    routes += [short_groups(j) for j in range(len(SHORT))]
    routes += [registered(j) for j in range(len(FP.HOST_PLANS))] + [("three sub-batches of the handle's own rule", sub_batches)]
    tail = []
    for k in range(len(TT.PLANS)):
        tail.append(demod_alone(k))
        tail += [squelched_audio(k, j) for j in range(len(AUDIO))]
        tail += [tone_squelched(k, t) for t in range(len(TS.SETTINGS))]
        tail += [tail_device(k), regrow(k)]
    return {"routes": routes,
            "fused": [fused(k, R) for R in (2, 4) for k in range(len(FP.F4))],
            "tail": tail,
            "around": [("sinks", sinks), ("sinks, an extraction wider than 4096 points", sinks_wide), ("PipelineGroup", pipeline_group), ("waterfall", waterfalls), ("faces", faces), ("hier block", hier_block)]}


def binding_proof(shim, poison):
    """a buffer taken from the shim's hipMalloc and hit one byte behind its payload with the RUNTIME's own hipMemset: reported at offset n, so the memory
    the shim hands out is memory it watches.  The byte is put back and the buffer freed: nothing is left in the sticky count."""
    hip = C.CDLL("libamdhip64.so")
    n = 1000
    shim.set(64 * 1024, poison)
    p = shim.malloc(n)
    assert p % 256 == 0
    assert hip.hipMemset(C.c_void_p(p + n), C.c_int(poison ^ 0xFF), C.c_size_t(1)) == 0 and hip.hipDeviceSynchronize() == 0
    total, first, text = shim.check()
    assert hip.hipMemset(C.c_void_p(p + n), C.c_int(poison), C.c_size_t(1)) == 0 and hip.hipDeviceSynchronize() == 0
    clean = shim.check()[0]
    shim.free(p)
    return dict(total=total, payload=first[1], first=first[2], last=first[3], count=first[4], clean=clean, text=text)


def main(argv):
    """GROUP FIRST LAST [SHIM [keep]]; `keep` (measuring by hand): a scenario that raises is listed under "errors" and the next one runs, unless the text
    speaks of the device's health"""
    import time
    group, lo, hi = argv[1], int(argv[2]), int(argv[3])
    shim = None
    sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "oracle")]
    if len(argv) > 4 and argv[4]:
        import guard_alloc as GA
        shim = GA.Shim(argv[4], mode=C.RTLD_GLOBAL)             # BEFORE the library: its hipMalloc & co. bind to the shim
    keep = len(argv) > 5 and argv[5] == "keep"
    suite()
    table = groups()[group][lo:hi]
    result, errors = {}, []
    passes = [(None, "plain")] if shim is None else [(b, "0x%02X" % b) for b in GA.POISONS]
    for poison, label in passes:
        run = Run(shim, poison)
        for name, scenario in table:
            run.scenario = name
            t0 = time.perf_counter()
            try:
                scenario(run)
            except Exception as e:                              # noqa: BLE001
                text = "%s: %r" % (type(e).__name__, e)
                if not keep or "illegal" in text or "hipError" in text or "HIP" in text:
                    raise
                errors.append("%s, %s: %s" % (label, name, text[:1500]))
            print("TIME %s %7.3f s  %s" % (label, time.perf_counter() - t0, name), file=sys.stderr)
        result[label] = run.items
        if shim is not None:
            result.setdefault("banded after the first call", run.first_counts[0])
            result["binding " + label] = binding_proof(shim, poison)
            run.scenario = "binding proof"
            if not errors:
                run.step("after the binding proof")
    if shim is not None:
        result["counts"] = list(shim.counts())
    if errors:
        result["errors"] = errors
    print("RESULT " + json.dumps(result))


if __name__ == "__main__":
    main(sys.argv)
