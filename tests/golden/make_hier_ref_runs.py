#!/usr/bin/env python3
"""Writes tests/golden/hier_ref_*.npz: RECORDED runs of the reference's hier block, python/FrequencyDomainChannelizer.py executed
to its last line over the reference's own compiled blocks (oracle/ref_hier.py), and of its three chain blocks on their own.  Data
only: argument lists, inputs (int16 I/Q with a power-of-two scale) and what the reference run gave.  The oracle is not involved.

Runs where the reference is present; the GPU machine reads the files.  tests/test_hier_reference_cpu.py regenerates everything in
memory and compares it with the committed files.

  hier_ref_input_<key>.npz / hier_ref_inputs_small.npz   the inputs, one array per input key of tests/hier_ref_cases.py
  hier_ref_runs_<family><k>.npz     "cases": JSON (name, args, input key, ports kept, the channel parameters and inpblocklen the run derived,
                                    the sink constructor calls, kernel path and describe() words); "<name>.port<p>": that output port, every
                                    sample; sink cases: "<name>.<block label>.meta" / ".rel" / ".payload": the PDUs of that block in its order
  hier_ref_blocks_<block>.npz       block-level cases: inputs and outputs of overlap_save / vector_cut_vxx / phase_shifting_windowing_vcc
  hier_ref_refused.json             what the reference refuses (exception type and message) and the listed divergences

Usage:  python3 tests/golden/make_hier_ref_runs.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import hier_ref_cases as HC           # noqa: E402
import sink_ref_cases as K            # noqa: E402

BUDGET = 800 * 1024                    # bytes of arrays per runs file (random-like float32 does not compress)
_inputs = {}


def input_of(key):
    if key not in _inputs:
        _inputs[key] = HC.make_input(key)
    return _inputs[key]


def run_case(RH, case, x=None):
    """(Built, output ports, {sink label: PDUs}) of the executed reference"""
    b = RH.build(*case["args"])
    outs, pdus = b.run(HC.as_complex(input_of(case["input"])) if x is None else x, per_call=1)
    return b, outs, pdus


def pdu_arrays(pdus):
    meta = np.array(K.meta_of(pdus), dtype=np.int64).reshape(len(pdus), len(K.META) + 1)
    rel = np.array([[d["rel_bw"], d["rel_cfreq"]] for d in pdus], dtype=np.float64).reshape(len(pdus), 2)
    pay = np.concatenate([d["samples"] for d in pdus]).astype(np.complex64) if pdus else np.zeros(0, np.complex64)
    return meta, rel, pay


def stable(RH, case, pdus):
    """sink_ref_cases' criterion: the same metadata, block by block, for the input plus noise 100 dB under the carriers"""
    x = HC.perturbed(HC.as_complex(input_of(case["input"])), HC.hash_name(case["name"]))
    _, _, again = run_case(RH, case, x)
    return all(K.meta_of(again[k]) == K.meta_of(pdus[k]) for k in pdus)


def describe(case, b, keep):
    return dict(name=case["name"], family=case["family"], args=case["args"], input=case["input"], N=case["N"], R=case["R"], nblocks=case["nblocks"],
                max_blocks=case["max_blocks"], path=case["path"], words=case["words"], gen_version=HC.GEN_VERSION, nports=b.nports(), ports=keep,
                channel_params=[list(p) for p in b.channel_params()], inpblocklen=int(b.obj.inpblocklen), blocksize=int(b.obj.blocksize),
                relinvovl=int(b.obj.relinvovl),
                sinks=[[blk.label(), blk.name, list(blk.args)] for blk in b.graph.blocks if blk.sink is not None],
                msg_ports=list(b.graph.msg_ports))


def record_blocks(O):
    make = {"overlap_save": O.RefOverlapSave, "vector_cut_vxx": O.RefVectorCut, "phase_shifting_windowing_vcc": O.RefPhaseWindow}
    files = {}
    for i, c in enumerate(HC.block_cases()):
        arrays, listing = files.setdefault("hier_ref_blocks_%s.npz" % c["block"], ({}, []))
        blk = make[c["block"]](*c["ctor"])
        per = blk.in_bytes // c["input"].dtype.itemsize
        out, at = [], 0
        for n in c["calls"]:
            out.append(blk.work(c["input"][at * per:(at + n) * per]))
            at += n
        assert at * per == c["input"].size
        arrays["b%03d.in" % i], arrays["b%03d.out" % i] = c["input"], np.concatenate(out)
        listing.append(dict(key="b%03d" % i, block=c["block"], ctor=list(c["ctor"]), calls=c["calls"]))
    return {name: dict(arrays, cases=np.array(json.dumps(listing))) for name, (arrays, listing) in files.items()}


def record_refused(RH):
    out = dict(refused=[], divergences=[])
    for name, a in HC.refused():
        try:
            RH.build(*a)
        except Exception as e:                             # noqa: BLE001 (the type IS the record)
            out["refused"].append(dict(name=name, args=a, raises=type(e).__name__, msg=str(e)))
        else:
            raise AssertionError("%s: the reference accepts this construction" % name)
    for name, a, ref_does, product_does, line in HC.divergences():
        try:
            RH.build(*a)
            got = "accepts"
        except Exception as e:                             # noqa: BLE001
            got = "raises " + type(e).__name__
        assert ref_does.startswith(got), (name, got, ref_does)
        out["divergences"].append(dict(name=name, args=a, reference=got, product=product_does, line=line))
    return out


def record(O, RH, runs=None):
    """{file name: {key: array}} of every .npz, and the refusals' dictionary.  runs: optional dict filled with name -> (Built, outs, pdus)."""
    files = {}
    pack, size, fam, k = {}, 0, None, 0
    listing = []

    def close():
        nonlocal pack, size, listing, k
        if listing:
            pack["cases"] = np.array(json.dumps(listing))
            files["hier_ref_runs_%s%d.npz" % (fam, k)] = pack
            k += 1
        pack, size, listing = {}, 0, []
    for case in HC.cases():
        b, outs, pdus = run_case(RH, case)
        if runs is not None:
            runs[case["name"]] = (b, outs, pdus)
        assert len(outs) == b.nports()
        keep = HC.stored_ports(case, len(outs))
        mine = {"%s.port%d" % (case["name"], p): outs[p] for p in keep}
        if pdus:
            assert stable(RH, case, pdus), "%s: a decision of the reference sits within noise of its threshold" % case["name"]
            assert sum(len(v) for v in pdus.values()) >= 4, "%s publishes next to nothing" % case["name"]
            for label, lst in pdus.items():
                mine[case["name"] + "." + label + ".meta"], mine[case["name"] + "." + label + ".rel"], mine[case["name"] + "." + label + ".payload"] = pdu_arrays(lst)
        nbytes = sum(v.nbytes for v in mine.values())
        if case["family"] != fam:
            close()
            fam, k = case["family"], 0
        elif size + nbytes > BUDGET:
            close()
        pack.update(mine)
        size += nbytes
        listing.append(describe(case, b, keep))
    close()
    small = {}
    for key, arr in sorted(_inputs.items()):
        if arr.nbytes >= 150 * 1024:
            files["hier_ref_input_%s.npz" % key] = {key: arr}
        else:
            small[key] = arr
    files["hier_ref_inputs_small.npz"] = small
    files.update(record_blocks(O))
    return files, record_refused(RH)


def main():
    import oracle as O
    import ref_hier as RH
    O.build()
    files, refused = record(O, RH)
    for old in os.listdir(HERE):
        if old.startswith("hier_ref_") and (old.endswith(".npz") or old.endswith(".json")):
            os.remove(os.path.join(HERE, old))
    for name, arrays in sorted(files.items()):
        np.savez_compressed(os.path.join(HERE, name), **arrays)
        print("%-44s %8d bytes" % (name, os.path.getsize(os.path.join(HERE, name))))
        assert os.path.getsize(os.path.join(HERE, name)) < 1000000, name
    with open(os.path.join(HERE, "hier_ref_refused.json"), "w") as fh:
        json.dump(refused, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
