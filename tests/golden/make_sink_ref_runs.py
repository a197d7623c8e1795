"""Records what the reference's OWN sink blocks (oracle/_ref/libref_sinks.so: lib/*_impl.cc compiled where they lie over
oracle/ref_standins/, recipe `make -C oracle ref`) publish for the seeded cases of tests/sink_ref_cases.py, so that a machine
without the reference can hold the device kernels against them (tests/test_sinks_reference_gpu.py).

    python tests/golden/make_sink_ref_runs.py        writes tests/golden/sink_ref_runs.npz (data only)

Per case: constructor arguments, seed, generator version and input CRC (JSON in "cases"); per PDU the metadata row
(sink_ref_cases.META + sample count), rel_bw / rel_cfreq, and of the payload either every sample (up to SMALL) or its float64 L2
norm and EXCERPT strided samples.  A noisy-class case is recorded only where the reference gives the same metadata for the input
plus noise 100 dB under the burst (sink_ref_cases.perturbed); the ones left out are listed in "dropped"."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import sink_ref_cases as K  # noqa: E402


def record(O):
    """O: the oracle module (its Ref* classes).  Returns the dict of arrays of sink_ref_runs.npz."""
    def run(case):
        return K.run_blocks(case, O.RefPowerActivationChannel, O.RefActivityDetectionVcm, O.RefSegmentDetection)
    out, cases, dropped = {}, [], []
    for name, case in K.recorded_cases():
        pdus = run(case)
        if case["klass"] == "noisy" and K.meta_of(run(dict(case, input=K.perturbed(case)))) != K.meta_of(pdus):
            assert "samples" not in case, name + ": a case from samples must be decision-stable (choose another one in sink_ref_cases.py)"
            dropped.append(name)
            continue
        cases.append(dict(name=name, block=case["block"], index=case["index"], klass=case["klass"], seed=case["seed"],
                          gen_version=K.GEN_VERSION, crc=K.crc(case["samples"] if "samples" in case else case["spec"]), from_samples="samples" in case, nb=int(case["spec"].shape[0]), args=case["args"]))
        out[name + "_meta"] = np.array(K.meta_of(pdus), dtype=np.int64).reshape(len(pdus), len(K.META) + 1)
        out[name + "_rel"] = np.array([[d["rel_bw"], d["rel_cfreq"]] for d in pdus], dtype=np.float64).reshape(len(pdus), 2)
        small = [d["samples"] for d in pdus if d["samples"].size <= K.SMALL]
        large = [d["samples"] for d in pdus if d["samples"].size > K.SMALL]
        out[name + "_small"] = np.concatenate(small + [np.zeros(0, np.complex64)]).astype(np.complex64)
        out[name + "_norm"] = np.array([np.linalg.norm(s.astype(np.complex128)) for s in large], dtype=np.float64)
        out[name + "_excerpt"] = np.array([s[K.excerpt_index(s.size)] for s in large], dtype=np.complex64).reshape(len(large), K.EXCERPT)
    out["cases"] = np.array(json.dumps(cases))
    out["dropped"] = np.array(json.dumps(dropped))
    return out


if __name__ == "__main__":
    import oracle as O
    O.build()
    arrays = record(O)
    path = os.path.join(HERE, "sink_ref_runs.npz")
    np.savez_compressed(path, **arrays)
    n = json.loads(str(arrays["cases"]))
    print("%d cases recorded (%s dropped as unstable), %d PDUs, %d bytes" % (
        len(n), json.loads(str(arrays["dropped"])), sum(arrays[c["name"] + "_meta"].shape[0] for c in n), os.path.getsize(path)))
