"""Measurement only (needs the GPU): the device's end-to-end error over E (tests/fft_model.py: chain64, chain_model_error) for every plan of
tests/block_accuracy_cases.py — noise, impulse stream, tone calls; every (block, channel) row — with the plan asserted to run the kernel form named.
Prints one MEASURE line per plan and input: the largest rms / E_rms and per-sample / E_max over the rows more than one ulp off, and the rows.  No bound is
asserted: README.md in this directory says why there is none yet and holds the figures of the last run.  The case with a first block other than 0
(the device entry) is left out.

    python profiles/accuracy/chain_device.py [output file]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in ("tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, d))
import numpy as np                         # noqa: E402

import block_accuracy_cases as BC          # noqa: E402
import fft_model as M                      # noqa: E402
import gr_fdc_amd as G                     # noqa: E402
import oracle as O                         # noqa: E402
from gr_fdc_amd import _lib                # noqa: E402

O.build()
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


for case in BC.all_cases():
    if case.first_block:
        continue
    t0 = time.time()
    ref_ = BC.Reference(case, O)
    flags = None
    if case.flags:
        flags = 0
        for n in case.flags:
            flags |= getattr(_lib, "FDC_PIPE_" + n)
    nbmax = len(M.impulse_positions(case.N)) + 1
    p = G.Pipeline(case.N, case.R, case.chans, windowtype=case.wintype, max_blocks=nbmax, flags=flags, min_block_launch=1)
    d = p.describe()
    exp = case.expect if isinstance(case.expect, tuple) else (case.expect,)
    ok = p.path() == case.path and all(e in d for e in exp)
    if not ok:
        say("PLAN MISMATCH %s: path %d, %s" % (case.id, p.path(), d))
        p.close()
        continue
    worst = {}
    for run in ref_.runs():
        p.reset()
        outs = p.work_iq(run.ints, scale=run.scale) if case.fmt else p.work(run.stream)
        if case.fmt and ("input %s: fused" % case.fmt) not in p.describe():
            say("IQ ROUTE %s: %s" % (case.id, p.describe()))
        for idx, ref, e, ys in ref_.rows(run):
            y = np.stack([outs[c].reshape(run.nb, ref.shape[-1]) for c in idx], axis=1)
            r_l2, r_max = BC.k_ratios(y, ref, e)
            l2, mx = M.relative_errors(y, ref)
            w = worst.setdefault(run.kind, [0.0, "", 0.0, "", 0.0, 0.0])
            for i, r in ((0, r_l2), (2, r_max)):
                if r.max() > w[i]:
                    m, c = np.unravel_index(int(np.argmax(r)), r.shape)
                    rms, mxe, top = M.item_errors(y[m, c], ref[m, c])
                    w[i], w[i + 1] = float(r.max()), "%s block %d ch %d err %.2f ulp E %.2f ulp" % (
                        run.what, m, idx[c], (rms if i == 0 else mxe) / top / M.ULP, e[i // 2][m, c] / M.ULP)
            w[4], w[5] = max(w[4], float(l2.max())), max(w[5], float(mx.max()))
    p.close()
    for kind, w in worst.items():
        say("MEASURE kernel=%s case=%s %s rms/E=%.3f [%s] max/E=%.3f [%s] relL2=%.3g relmax=%.3g" % (case.kernel, case.id, kind, w[0], w[1], w[2], w[3], w[4], w[5]))
    say("  (%.1f s)" % (time.time() - t0))
say("DONE")
