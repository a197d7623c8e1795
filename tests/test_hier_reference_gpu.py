"""GPU tests (-m gpu): the device against RECORDED runs of the reference's own hier block and chain blocks
(tests/golden/hier_ref_*.npz, written by tests/golden/make_hier_ref_runs.py from python/FrequencyDomainChannelizer.py executed to
its last line over lib/*_impl.cc compiled where they lie).  Neither the reference nor the oracle is involved here: the recordings
do not depend on the oracle at all, and this file does not need the oracle to agree with anything.

Every recorded case goes through G.FrequencyDomainChannelizer(*args) — the recorded argument list of the reference's constructor —
in ragged work() calls (1 item, several, 0, the rest); every recorded port is held against the recording at TOL = 1e-5 in both norms
of test_parity_gpu.py (relative L2 and relative max), port by port, every recorded sample.  The sink case runs serial and pipelined
with flush(); PDUs are compared per sink block in that block's own order (the order AMONG blocks is the scheduler's), metadata
exact, rel_bw / rel_cfreq to 1e-12, payloads to TOL.  Bank cases run again from the same integers through iq_input="sc16" and
through PipelineGroup([0, 0]), and must report the kernel path they were written for.  The single-block faces are held against the
block-level recordings: overlap_save and vector_cut_vxx bit for bit, the phase window to the 1e-6 of test_phase_window_block."""
import glob
import json
import os

import numpy as np
import pytest

import gr_fdc_amd as G
import hier_ref_cases as HC
import sink_ref_cases as K

pytestmark = pytest.mark.gpu
TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

REC, CASES, INPUTS = {}, [], {}
for _p in sorted(glob.glob(os.path.join(GOLDEN, "hier_ref_runs_*.npz"))):
    with np.load(_p) as _f:
        REC.update({k: _f[k] for k in _f.files if k != "cases"})
        CASES += json.loads(str(_f["cases"]))
for _p in sorted(glob.glob(os.path.join(GOLDEN, "hier_ref_input*.npz"))):
    with np.load(_p) as _f:
        INPUTS.update({k: _f[k] for k in _f.files})
BLOCKS = {}
for _p in sorted(glob.glob(os.path.join(GOLDEN, "hier_ref_blocks_*.npz"))):
    with np.load(_p) as _f:
        for _c in json.loads(str(_f["cases"])):
            BLOCKS[_c["key"]] = dict(_c, input=_f[_c["key"] + ".in"], output=_f[_c["key"] + ".out"])
BANKS = [c for c in CASES if c["family"] in "cd"]
SEEN = dict(ports=0, samples=0, l2=0.0, mx=0.0, pdus=0, pl2=0.0, pmx=0.0)
ids = lambda lst: [c["name"] for c in lst]


def forced():
    return any(G.defaults.get(k) for k in ("FDC_FORCE_GENERIC", "FDC_NO_POLY", "FDC_NO_BLOCK", "FDC_NO_FUSED"))


def rel(a, r):
    d = a.astype(np.complex128) - r.astype(np.complex128)
    return float(np.linalg.norm(d) / np.linalg.norm(r)), float(np.abs(d).max() / np.abs(r).max())


def hold(c, ports, what):
    assert len(ports) == c["nports"], (what, len(ports), c["nports"])
    for p in c["ports"]:
        r = REC["%s.port%d" % (c["name"], p)]
        assert ports[p].shape == r.shape, (what, p, ports[p].shape, r.shape)
        l2, mx = rel(ports[p], r)
        assert l2 <= TOL and mx <= TOL, (what, "port %d" % p, l2, mx)
        SEEN["l2"], SEEN["mx"] = max(SEEN["l2"], l2), max(SEEN["mx"], mx)
        SEEN["ports"] += 1
        SEEN["samples"] += r.size


def test_the_recordings_cover_what_they_should():
    assert {c["family"] for c in CASES} == set("abcdefg") and all(c["gen_version"] == HC.GEN_VERSION for c in CASES)
    assert [c["name"] for c in CASES] == [c["name"] for c in HC.cases()]                    # nothing dropped between the list and the files
    for c in CASES:
        assert c["nblocks"] >= 2 * c["relinvovl"] + 1 and c["input"] in INPUTS, c["name"]
        assert all("%s.port%d" % (c["name"], p) in REC for p in c["ports"]) and 0 in c["ports"] and c["nports"] - 1 in c["ports"], c["name"]
        assert len(c["ports"]) == c["nports"] or len(c["ports"]) >= 18, c["name"]
    assert {c["channel_params"][1][1] for c in CASES if c["family"] == "c"} == {64, 128, 256, 512, 1024}
    assert len(BLOCKS) >= 100


def run_ragged(fdc, c, x, per_item, collect=None):
    """work() in calls of 1, several, 0 and the rest of the items; returns the ports, call outputs joined"""
    parts, at = [], 0
    for n in HC.ragged(c["nblocks"]):
        parts.append(fdc.work(x[at * per_item:(at + n) * per_item]))
        if collect is not None:
            collect += fdc.messages
        at += n
    assert at == c["nblocks"]
    return [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]


def check_path(c, pipeline):
    if c["path"] is not None and not forced():
        assert pipeline.path() == c["path"] and all(w in pipeline.describe() for w in c["words"]), (c["name"], pipeline.path(), pipeline.describe())


def pdu_meta(d, data):
    """a published (dictionary, samples) pair in the columns of sink_ref_cases.META (+ sample count); source and channel number are in the ID"""
    tail = d["ID"][20:].split(".")                      # the stamp is "YYYY-mm-dd-HH-MM-SS." (19 characters and a dot)
    pac = tail[0] == "PowActChan"
    row = [0 if pac else 1, int(tail[1]), int(tail[2]), int(d["finalized"]), int("part" in d), int(d["part"]) if "part" in d else -1,
           int(d["blockstart"]), int(d["blockend"])]
    if not pac:
        row += [int(d["vectorstart"]), int(d["vectorend"])]
    return pac, tuple(row) + (int(data.size),)


def hold_pdus(c, messages, what):
    for label, name, a in c["sinks"]:
        pac = name == "PowerActivationChannel"
        ident = a[11] if pac else a[0]
        got = [(m, d) for (m, d) in messages if pdu_meta(m, d)[0] == pac and pdu_meta(m, d)[1][1] == ident]
        meta, relv, pay = REC["%s.%s.meta" % (c["name"], label)], REC["%s.%s.rel" % (c["name"], label)], REC["%s.%s.payload" % (c["name"], label)]
        want = [tuple(int(v) for v in (list(r[:8]) + [r[-1]] if pac else r)) for r in meta]            # (no vectorstart / vectorend in a PowerActivationChannel dictionary)
        rows = [pdu_meta(m, d)[1] for (m, d) in got]
        assert rows == want, (what, label, [(k, x, y) for k, (x, y) in enumerate(zip(rows, want)) if x != y][:3], len(rows), len(want))
        off = 0
        for k, ((m, d), rv) in enumerate(zip(got, relv)):
            assert abs(m["rel_bw"] - rv[0]) < 1e-12 and abs(m["rel_cfreq"] - rv[1]) < 1e-12, (what, label, k)
            r = pay[off:off + d.size]
            off += d.size
            if d.size:
                l2, mx = rel(d, r)
                assert l2 <= TOL and mx <= TOL, (what, label, k, l2, mx)
                SEEN["pl2"], SEEN["pmx"] = max(SEEN["pl2"], l2), max(SEEN["pmx"], mx)
        assert off == pay.size
        SEEN["pdus"] += len(got)
    assert sum(len(REC["%s.%s.meta" % (c["name"], s[0])]) for s in c["sinks"]) == len(messages), what


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_hier_block_against_the_recorded_reference_run(c):
    x = HC.as_complex(INPUTS[c["input"]])
    per_item = c["inpblocklen"] if c["args"][1] == 1 else c["blocksize"]
    for pipelined in ((False, True) if c["sinks"] else (False,)):
        fdc = G.FrequencyDomainChannelizer(*c["args"], max_blocks=c["max_blocks"], pipelined=pipelined)
        assert [tuple(p) for p in fdc.channel_params] == [tuple(p) for p in c["channel_params"]] and fdc.inpblocklen == c["inpblocklen"]
        check_path(c, fdc.pipeline)
        msgs = []
        ports = run_ragged(fdc, c, x, per_item, msgs)
        msgs += fdc.flush()
        what = "%s%s" % (c["name"], ", pipelined" if pipelined else "")
        hold(c, ports, what)
        if c["sinks"]:
            hold_pdus(c, msgs, what)
        else:
            assert not msgs
        fdc.pipeline.close()


@pytest.mark.parametrize("c", BANKS, ids=ids(BANKS))
def test_bank_cases_from_the_same_integers_through_sc16(c):
    iq = INPUTS[c["input"]]
    fdc = G.FrequencyDomainChannelizer(*c["args"], max_blocks=c["max_blocks"], iq_input="sc16", iq_scale=HC.SCALE)
    check_path(c, fdc.pipeline)
    hold(c, run_ragged(fdc, c, iq, c["inpblocklen"]), c["name"] + ", sc16")
    fdc.pipeline.close()


@pytest.mark.parametrize("c", BANKS, ids=ids(BANKS))
def test_bank_cases_through_a_group_of_two_members_on_one_device(c):
    plan = [(f, l, pb, sb) for (f, l, _lo, pb, sb) in c["channel_params"]]
    g = G.PipelineGroup(c["blocksize"], c["relinvovl"], plan, [0, 0], windowtype=c["args"][10], max_blocks=c["max_blocks"])
    assert forced() or g.path() == c["path"], (c["name"], g.path())
    hold(c, g.work(HC.as_complex(INPUTS[c["input"]])), c["name"] + ", PipelineGroup([0, 0])")
    g.close()


def _ragged_block(blk, c, per):
    out, at = [], 0
    for n in c["calls"]:
        out.append(blk.work(c["input"][at * per:(at + n) * per]))
        at += n
    return np.concatenate(out)


@pytest.mark.parametrize("key", sorted(BLOCKS), ids=lambda k: "%s-%s" % (k, BLOCKS[k]["block"]))
def test_single_block_faces_against_the_recorded_reference_blocks(key):
    c = BLOCKS[key]
    a = c["ctor"]
    if c["block"] == "overlap_save":
        got = _ragged_block(G.overlap_save(*a), c, a[0] * (a[1] - a[2]) // c["input"].dtype.itemsize)
        assert got.tobytes() == c["output"].tobytes(), (key, a, c["calls"])
    elif c["block"] == "vector_cut_vxx":
        got = _ragged_block(G.vector_cut_vxx(*a), c, a[0] * a[1] // c["input"].dtype.itemsize)
        assert got.tobytes() == c["output"].tobytes(), (key, a, c["calls"])
    else:
        got = _ragged_block(G.phase_shifting_windowing_vcc(*a), c, a[0])
        l2, mx = rel(got, c["output"])
        assert l2 <= 1e-6 and mx <= 1e-6, (key, a, c["calls"], l2, mx)


@pytest.mark.parametrize("a", HC.PHASE_WINDOW_REFUSALS)
def test_phase_window_face_refuses_what_the_reference_refuses(a):
    with pytest.raises(ValueError):
        G.phase_shifting_windowing_vcc(*a)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """for the record, next to TOL: what this module compared, printed once when its last test is done"""
    yield
    print("\nrecorded runs of the reference's hier block: %d ports, %d samples compared, largest error L2 %.2e, max %.2e; %d PDUs, largest payload error "
          "L2 %.2e, max %.2e (TOL %.0e)" % (SEEN["ports"], SEEN["samples"], SEEN["l2"], SEEN["mx"], SEEN["pdus"], SEEN["pl2"], SEEN["pmx"], TOL))
