"""CPU tests (-m "not gpu"): the reference's OWN sink blocks — lib/PowerActivationChannel_impl.cc,
lib/activity_detection_channelizer_vcm_impl.cc and lib/SegmentDetection_impl.cc compiled where they lie into
oracle/_ref/libref_sinks.so over the stand-ins of oracle/ref_standins/ — as a second, independent judge of the oracle's
restatement (oracle/fdc_oracle_detect.c) and of the hand-derived scenarios.

Metadata (ID suffix, finalized, part and its absence, blockstart, blockend, vectorstart, vectorend, sample count, order) is
compared exactly, rel_cfreq / rel_bw to 1e-12, payloads to TOL = 1e-5 (relative L2 and max) with the reference run as the
denominator.  Skipped only where neither the reference's sources nor a built libref_sinks.so exist."""
import json
import os
import subprocess

import numpy as np
import pytest

import sink_ref_cases as K
import sink_scenarios as S

TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.have_ref_sinks():
        pytest.skip("neither /root/reference nor oracle/_ref/libref_sinks.so is present: the reference's sink blocks cannot be run")
    return oracle


def _pairs(pdus, expect=None):
    """(meta, samples) pairs for sink_scenarios.check.  A PowerActivationChannel dictionary has no vectorstart / vectorend
    (the scenario tables carry the extraction range for the product's C structure): they are taken from the expectation, and
    check() still pins them through rel_cfreq = (start + stop) / 2 / N and rel_bw, which the dictionary does carry."""
    out = []
    for k, d in enumerate(pdus):
        d = dict(d)
        if d["vectorstart"] < 0 and expect is not None and k < len(expect):
            d["vectorstart"], d["vectorend"] = expect[k]["vectorstart"], expect[k]["vectorend"]
        out.append((d, d["samples"]))
    return out


# ---- every hand-derived scenario through the compiled reference: was the paper right?
@pytest.mark.parametrize("per_call", [0, 1])
@pytest.mark.parametrize("sc", S.VCM, ids=[s["name"] for s in S.VCM])
def test_reference_vcm_scenarios(ref, sc, per_call):
    blk = ref.RefActivityDetectionVcm(S.N, [sc.get("segment", S.SEG)], 10.0, S.R, sc["maxblocks"], 0.0625, sc["delay"], sc["puffer"])
    S.check(sc["name"], _pairs(blk.work(sc["spec"], per_call)), sc["expect"])


@pytest.mark.parametrize("per_call", [0, 1])
@pytest.mark.parametrize("sc", S.PAC, ids=[s["name"] for s in S.PAC])
def test_reference_pac_scenarios(ref, sc, per_call):
    got = ref.RefPowerActivationChannel(S.N, 0.5, 16.0 / S.N, S.R, 6.0, sc["maxblocks"], 0, 9).work(sc["spec"], per_call)
    S.check(sc["name"], _pairs(got, sc["expect"]), sc["expect"])
    assert all(d["source"] == 9 and d["ident"].endswith(".fin" if d["finalized"] else ".part") for d in got)


@pytest.mark.parametrize("per_call", [0, 1])
@pytest.mark.parametrize("sc", S.PAC_GEOM, ids=[s["name"] for s in S.PAC_GEOM])
def test_reference_pac_geometry_and_payload_scenarios(ref, sc, per_call):
    cf, bw = sc["pac"]
    got = ref.RefPowerActivationChannel(S.N, cf, bw, S.R, 6.0, sc["maxblocks"], 0, 9).work(sc["spec"], per_call)
    S.check(sc["name"], _pairs(got, sc["expect"]), sc["expect"])


@pytest.mark.parametrize("per_call", [0, 1])
@pytest.mark.parametrize("sc", S.SD, ids=[s["name"] for s in S.SD])
def test_reference_segment_detection_scenarios(ref, sc, per_call):
    ident, a, b = sc["sd"]
    got = ref.RefSegmentDetection(ident, S.N, S.R, a, b, 10.0, 0.0625, sc["puffer"], sc["maxblocks"], sc["delay"]).work(sc["spec"], per_call)
    S.check(sc["name"], _pairs(got), sc["expect"])
    assert all(d["source"] == ident for d in got)


# ---- the three known answers, re-run through the compiled reference
def test_known_answers_are_the_compiled_references(ref, golden_dir):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(golden_dir, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ka = json.load(open(os.path.join(golden_dir, "sink_known_answers.json")))
    now = mod.sink_known_answers()
    assert {k: v for k, v in ka.items() if k != "source"} == {k: v for k, v in now.items() if k != "source"}


# ---- differential fuzz: compiled reference against the oracle
def compare(ref_pdus, got_pdus, what, vec=True):
    """exact metadata, rel_* to 1e-12, payload to TOL with the reference run as the denominator; returns the largest errors seen"""
    assert K.meta_of(got_pdus, vec) == K.meta_of(ref_pdus, vec), (what, K.meta_of(got_pdus, vec), K.meta_of(ref_pdus, vec))
    worst = (0.0, 0.0)
    for k, (r, g) in enumerate(zip(ref_pdus, got_pdus)):
        assert abs(g["rel_bw"] - r["rel_bw"]) < 1e-12 and abs(g["rel_cfreq"] - r["rel_cfreq"]) < 1e-12, (what, k)
        if r["samples"].size:
            d = g["samples"].astype(np.complex128) - r["samples"].astype(np.complex128)
            nr, mr = np.linalg.norm(r["samples"].astype(np.complex128)), np.abs(r["samples"]).max()
            assert np.linalg.norm(d) <= TOL * nr and np.abs(d).max() <= TOL * mr, (what, k, np.linalg.norm(d), nr, np.abs(d).max(), mr)
            if nr > 0:                               # (an all-zero reference payload must be met exactly)
                worst = (max(worst[0], np.linalg.norm(d) / nr), max(worst[1], np.abs(d).max() / mr))
    return worst


def _reference(ref, case, **kw):
    return K.run_blocks(case, ref.RefPowerActivationChannel, ref.RefActivityDetectionVcm, ref.RefSegmentDetection, **kw)


def _oracle(ref, case):
    return K.run_blocks(case, ref.PowerActivationChannel, ref.ActivityDetectionVcm, ref.SegmentDetection)


def stable(ref, case):
    """decision-stable by the reference alone: the same metadata for the input and for the input plus noise 100 dB under the burst"""
    return K.meta_of(_reference(ref, case)) == K.meta_of(_reference(ref, dict(case, input=K.perturbed(case))))


@pytest.mark.parametrize("block", K.BLOCKS)
def test_fuzz_reference_against_oracle(ref, block, capfd):
    n_exact = n_noisy = n_stable = n_pdus = n_nonempty = 0
    worst, least_margin = (0.0, 0.0), np.inf
    for index in range(K.N_FUZZ):
        case = K.make_case(block, index)
        what = "%s case %d (%s, seed %d)" % (block, index, case["klass"], case["seed"])
        if case["klass"] == "exact":
            n_exact += 1
            m = K.margin(case)
            assert m > 1e-4, (what, "a decision quotient sits at the threshold", m)
            least_margin = min(least_margin, m)
        else:
            n_noisy += 1
            if not stable(ref, case):
                continue
            n_stable += 1
        r = _reference(ref, case, per_call=case["per_call"])           # ragged work() calls: 1, 2, 7 items or all in one
        w = compare(r, _oracle(ref, case), what, vec=block != "pac")
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        n_pdus += len(r)
        n_nonempty += bool(r)
        if case["per_call"]:                                           # ... and the reference against itself in one call
            assert K.meta_of(_reference(ref, case)) == K.meta_of(r), what
    with capfd.disabled():
        print("\n%s: %d exact cases (none left out, least margin to a threshold %.2e), %d noisy cases drawn, %d stable and kept, %d dropped; "
              "%d PDUs compared, %d cases publish something; largest payload error of the oracle against the reference run: L2 %.2e, max %.2e (TOL %.0e)"
              % (block, n_exact, least_margin, n_noisy, n_stable, n_noisy - n_stable, n_pdus, n_nonempty, worst[0], worst[1], TOL))
    assert n_exact + n_noisy == K.N_FUZZ >= 300 and n_exact == sum(K.klass_of(i) == "exact" for i in range(K.N_FUZZ))
    assert n_stable >= 0.9 * n_noisy, (n_stable, n_noisy)
    assert n_pdus >= 3 * K.N_FUZZ // 2
    # a case that publishes nothing checks "no false detection" and none of the state machines: the generator aims its bursts so
    # that most cases activate something (sink_ref_cases.py); at least two of three must
    assert 3 * n_nonempty >= 2 * K.N_FUZZ, (n_nonempty, K.N_FUZZ)


def _by_item(pdus):
    return sorted(K.meta_of(pdus))


@pytest.mark.parametrize("block", ["vcm", "sd"])
def test_reference_threaded_equals_single_threaded(ref, block):
    """`threads` true against false on the reference.  The threaded paths publish from concurrent threads and send the partial
    PDUs of an item behind all of its final ones, so WITHIN one item the order of publication is theirs to choose; the items are
    fed one per work() call and each item's PDUs are compared as a set, payloads bit for bit."""
    for index in range(0, 60, 3):                                      # exact class
        case = K.make_case(block, index)
        a = case["args"]
        if block == "vcm":
            mk = lambda t: ref.RefActivityDetectionVcm(a["N"], [list(s) for s in a["segs"]], a["thresh"], a["R"], a["maxblocks"],
                                                       a["minchandist"], a["delay"], a["puffer"], threads=t)
        else:
            mk = lambda t: ref.RefSegmentDetection(a["ident"], a["N"], a["R"], a["segs"][0][0], a["segs"][0][1], a["thresh"],
                                                   a["minchandist"], a["puffer"], a["maxblocks"], a["delay"], threads=t)
        one, many = mk(False), mk(True)
        for item in case["spec"]:
            p, q = one.work(item), many.work(item)
            key = lambda d: K.meta_of([d])[0]
            p, q = sorted(p, key=key), sorted(q, key=key)
            assert K.meta_of(p) == K.meta_of(q), (block, index)
            assert all(np.array_equal(x["samples"], y["samples"]) for x, y in zip(p, q)), (block, index)


# ---- the recordings the GPU machine judges the device by are what the compiled reference gives today
def test_recorded_reference_runs_are_current(ref, golden_dir):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_sink_ref_runs", os.path.join(golden_dir, "make_sink_ref_runs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    now = mod.record(ref)
    with np.load(os.path.join(golden_dir, "sink_ref_runs.npz")) as have:
        assert sorted(have.files) == sorted(now)
        for k in now:
            assert have[k].dtype == now[k].dtype and np.array_equal(have[k], now[k]), k


# ---- the sanitized build of the same sources reads and writes inside its buffers
def test_sanitized_reference_build_is_clean(ref, tmp_path):
    if not os.path.isdir("/root/reference"):
        pytest.skip("the reference's sources are not present: oracle/_san/ref_sinks_check cannot be built")
    exe = os.path.join(ROOT, "oracle", "_san", "ref_sinks_check")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "_san/ref_sinks_check"])
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:log_path=stderr"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=str(tmp_path), timeout=600)
    err = p.stderr.decode(errors="replace")
    report = [ln for ln in err.splitlines() if "Sanitizer" in ln or "runtime error" in ln]
    assert p.returncode == 0 and not report, (p.returncode, p.stdout.decode()[-2000:], err[-4000:])
    assert b"cases, all as expected" in p.stdout
