"""GPU tests (-m gpu): the HIP sink engines against RECORDED runs of the reference's own sink blocks
(tests/golden/sink_ref_runs.npz, written by tests/golden/make_sink_ref_runs.py from lib/*_impl.cc compiled where they lie over
oracle/ref_standins/).  Neither the reference nor the oracle is involved here: the recordings do not depend on the oracle at all.

For every recorded case: the device engine and the host engine, payloads in host memory and left in HBM; inputs regenerated from
the seed and checked against the recorded CRC first.  The cases recorded from TIME SAMPLES (the reference ran on the numpy.fft
spectrum of those samples) go through fdc_pipeline_work_sinks instead — forward transform on the device, sinks fed from the
spectrum in HBM — in its serial form and in its pipelined look-ahead form with fdc_pipeline_flush_sinks at the end, in ragged calls.  Metadata (source and channel number of the ID, finalized, part and its
absence, blockstart, blockend, vectorstart, vectorend, sample count, order) exact, rel_bw / rel_cfreq to 1e-12, payloads to
TOL = 1e-5 against the recorded reference values (every sample of a small payload; L2 norm and a strided excerpt of a large one).
Noisy-class cases were recorded only where the reference's decisions survive noise 100 dB under the burst, which is what makes an
exact comparison fair for kernels that sum the power cells in another order.  Nothing is left out."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gr_fdc_amd as G
import sink_ref_cases as K

pytestmark = pytest.mark.gpu
TOL = 1e-5

with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sink_ref_runs.npz")) as _f:
    REC = {k: _f[k] for k in _f.files}
CASES = json.loads(str(REC["cases"]))
SEEN = dict(cases=set(), device=set(), pdus=0, l2=0.0, mx=0.0)


def test_the_recordings_cover_what_they_should():
    per = {b: sum(c["block"] == b and c["index"] >= 0 for c in CASES) for b in K.BLOCKS}
    assert all(n >= 40 for n in per.values()), per
    assert all(sum(c["block"] == b and c["from_samples"] for c in CASES) >= 1 for b in K.BLOCKS)
    for b in K.BLOCKS:                                        # most recorded cases publish something (sink_ref_cases.py aims its bursts)
        assert 3 * sum(REC[c["name"] + "_meta"].shape[0] > 0 for c in CASES if c["block"] == b) >= 2 * sum(c["block"] == b for c in CASES), b
    assert {"pac_baseline", "vcm_baseline"} <= {c["name"] for c in CASES}
    exact = {(c["block"], c["index"]) for c in CASES if c["klass"] == "exact"}
    assert exact == {(b, i) for b in K.BLOCKS for i in range(K.RECORDED) if K.klass_of(i) == "exact"}      # no exact case left out
    assert all(c["gen_version"] == K.GEN_VERSION for c in CASES)


def _bank(c, host, devpay, max_blocks, lookahead=False):
    a = c["args"]
    kw = dict(max_blocks=max_blocks, host_decisions=host, device_payload=devpay, lookahead=lookahead)
    if c["block"] == "pac":
        bank = G.Sinks(a["N"], a["R"], pac=[tuple(ch) for ch in a["chans"]], pac_thresh=a["thresh"], pac_maxblocks=a["maxblocks"],
                       pac_delay=a["delay"], **kw)
    else:
        sd = c["block"] == "sd"
        bank = G.Sinks(a["N"], a["R"], segments=[tuple(s) for s in a["segs"]], det_thresh=a["thresh"], det_maxblocks=a["maxblocks"],
                       minchandist=a["minchandist"], det_delay=a["delay"], puffer=a["puffer"], det_variant=1 if sd else 0,
                       det_id=a["ident"] if sd else -1, **kw)
    # the engine that is meant: a quiet fall-back to host threads would make the "device" leg the host engine a second time
    want = 0 if host else int(K.device_engine_expected(a, [bank.segment_params(i) for i in range(bank.nseg)]))
    assert bank.engine() == want, (c["name"], bank.engine(), want)
    if want:
        SEEN["device"].add(c["name"])
    return bank


def _fetch(pdus, devpay):
    if not devpay:
        return pdus
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = []
    for m, d in pdus:
        if isinstance(d, tuple):                              # (device address, sample count): the payload stayed in HBM
            ptr, n = d
            arr = np.zeros(n, np.complex64)
            if n:
                assert hip.hipMemcpy(arr.ctypes.data, ptr, 8 * n, 2) == 0
            d = arr
        out.append((m, d))
    return out


def _check(c, got, what):
    """got: (meta, samples) of one bank in its order of publication.  A PowerActivationChannel bank publishes item by item across
    its channels, the reference blocks were run channel after channel: both are brought into (source, order within the source)."""
    name, pac = c["name"], c["block"] == "pac"
    if pac:
        order = {ch[2]: k for k, ch in enumerate(c["args"]["chans"])}
        got = sorted(got, key=lambda g: order[g[0]["source"]])                  # stable: the order within a channel stays
    keys = K.META[:-2] if pac else K.META                     # (a PowerActivationChannel dictionary has no vectorstart / vectorend)
    rows = [tuple(int(m[k]) if not (k == "part" and not m["has_part"]) else -1 for k in keys) + (int(d.size),) for m, d in got]
    ref = [tuple(int(v) for v in (r[:len(keys)] if pac else r[:-1])) + (int(r[-1]),) for r in REC[name + "_meta"]]
    assert rows == ref, (what, [(k, a, b) for k, (a, b) in enumerate(zip(rows, ref)) if a != b][:3], len(rows), len(ref))
    small, off, big = REC[name + "_small"], 0, 0
    for k, ((m, d), rel) in enumerate(zip(got, REC[name + "_rel"])):
        assert abs(m["rel_bw"] - rel[0]) < 1e-12 and abs(m["rel_cfreq"] - rel[1]) < 1e-12, (what, k)
        if d.size == 0:
            continue
        if d.size <= K.SMALL:
            r = small[off:off + d.size].astype(np.complex128)
            off += d.size
            e = d.astype(np.complex128) - r
            nr = np.linalg.norm(r)
            assert np.linalg.norm(e) <= TOL * nr, (what, k, np.linalg.norm(e), nr)
        else:
            r = REC[name + "_excerpt"][big].astype(np.complex128)
            nr = REC[name + "_norm"][big]
            big += 1
            assert abs(np.linalg.norm(d.astype(np.complex128)) - nr) <= TOL * nr, (what, k)
            e = d[K.excerpt_index(d.size)].astype(np.complex128) - r
            nr = np.linalg.norm(r)
            assert np.linalg.norm(e) <= TOL * nr, (what, k, np.linalg.norm(e), nr)
        mr = np.abs(r).max()
        assert np.abs(e).max() <= TOL * mr, (what, k, np.abs(e).max(), mr)
        if nr > 0:
            SEEN["l2"], SEEN["mx"] = max(SEEN["l2"], np.linalg.norm(e) / nr), max(SEEN["mx"], np.abs(e).max() / mr)
    assert off == small.size and big == REC[name + "_norm"].size
    SEEN["cases"].add(name)
    SEEN["pdus"] += len(got)


@pytest.mark.parametrize("c", [c for c in CASES if not c["from_samples"]], ids=[c["name"] for c in CASES if not c["from_samples"]])
def test_engines_against_the_recorded_reference_run(c):
    case = K.regenerate(c)
    spec = case["spec"]
    assert K.crc(spec) == c["crc"] and case["seed"] == c["seed"], "the input regenerated here is not the one that was recorded"
    for host, devpay, max_blocks in ((False, False, 7), (True, False, 7), (False, True, spec.shape[0]), (True, False, spec.shape[0])):
        bank = _bank(c, host, devpay, max_blocks)
        got = _fetch(bank.work(spec.reshape(-1)), devpay)                       # batches of 7 items: state crosses the calls
        _check(c, got, "%s, %s engine, payload %s, batches of %d" % (c["name"], "host" if host else "device", "in HBM" if devpay else "on the host", max_blocks))
        bank.close()


@pytest.mark.parametrize("lookahead", [False, True], ids=["serial", "pipelined"])
@pytest.mark.parametrize("host", [False, True], ids=["device-engine", "host-engine"])
@pytest.mark.parametrize("c", [c for c in CASES if c["from_samples"]], ids=[c["name"] for c in CASES if c["from_samples"]])
def test_pipeline_entry_from_samples_against_the_recorded_reference_run(c, host, lookahead):
    """fdc_pipeline_work_sinks on time samples, in ragged calls; the pipelined form hands a call's PDUs out one or two calls later and
    the rest at fdc_pipeline_flush_sinks.  The recorded run is the reference on the numpy.fft spectrum of the same samples."""
    case = K.regenerate(c)
    x, a = case["samples"], c["args"]
    assert K.crc(x) == c["crc"] and case["seed"] == c["seed"], "the input regenerated here is not the one that was recorded"
    H = a["N"] - a["N"] // a["R"]
    assert sum(case["cuts"]) * H == x.size
    for devpay in (False, True):
        bank = _bank(c, host, devpay, max(case["cuts"]), lookahead)
        p = G.Pipeline(a["N"], a["R"], [], max_blocks=max(case["cuts"]), keep_spectrum=True)
        assert p.sinks_latency(bank) == ((1 if host else 2) if lookahead else 0)
        got, at = [], 0
        for n in case["cuts"]:
            p.work(x[at * H:(at + n) * H], sinks=bank)
            got += _fetch(bank.pdus(), devpay)
            at += n
        while p.flush_sinks(bank) > 0:
            got += _fetch(bank.pdus(), devpay)
        _check(c, got, "%s from samples, %s engine, %s, payload %s" % (c["name"], "host" if host else "device",
                                                                      "pipelined" if lookahead else "serial", "in HBM" if devpay else "on the host"))
        bank.close()


@pytest.fixture(scope="module", autouse=True)
def _report():
    """for the record, next to TOL: what this module compared, printed once when its last test is done"""
    yield
    print("\nrecorded reference runs: %d cases (%d of them with the decisions on the device), %d PDUs compared; largest payload error against the reference run: L2 %.2e, max %.2e (TOL %.0e)"
          % (len(SEEN["cases"]), len(SEEN["device"]), SEEN["pdus"], SEEN["l2"], SEEN["mx"], TOL))
