#!/usr/bin/env python3
"""Do the kernels of two commits compile to the same code?

    tools/compare_block_isa.py [--files A,B,...] [--new-files C,D,...] [BASE [NEW]]
        BASE: a commit (default HEAD); NEW: a commit, or the working tree when left out
        --files: the .hip files of gr-fdc_amd/csrc to compile, without the suffix (default: the four one-block-per-CU kernel files and fdc_fused4096);
        --new-files: those of the NEW side where they differ — a kernel that moved between files is matched by its symbol

Compiles the files of both sides for the device only (the Makefile's flags plus --cuda-device-only -S) and compares every kernel by symbol:
the instructions of its body, and its resource usage (the .amdhsa_* block, the .set lines of its register counts, its entry in the
amdhsa.kernels metadata).  The order of the kernels in a file and the numbers in local labels follow the order of instantiation, which is
not code: both are normalised away.  Needs hipcc, no GPU.  Exit status 1 on a difference."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "gr-fdc_amd/csrc"
FILES = ["fdc_block256", "fdc_block512", "fdc_block1024", "fdc_blocknarrow", "fdc_fused4096"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-Wall", "-Wno-unused-result",
         "--cuda-device-only", "-S"]


def compile_side(rev, files, tmp):
    """{file: assembly text} of one side, compiled in tmp (a directory of this side's own: BASE and NEW may be the same commit); rev None = the working tree"""
    src = os.path.join(ROOT, CSRC)
    os.makedirs(tmp)
    if rev is not None:
        top = os.path.join(tmp, "src")
        os.makedirs(top)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", top], stdin=tar.stdout)
        if tar.wait():
            raise SystemExit("git archive %s failed" % rev)
        src = os.path.join(top, CSRC)
    out = {}
    procs = []
    for f in files:
        s = os.path.join(tmp, f + ".s")
        procs.append((f, s, subprocess.Popen([HIPCC] + FLAGS + [f + ".hip", "-o", s], cwd=src, stderr=subprocess.PIPE, text=True)))
    for f, s, p in procs:
        err = p.communicate()[1]
        if p.returncode:
            raise SystemExit("%s.hip of %s does not compile:\n%s" % (f, rev or "the working tree", err))
        out[f] = open(s).read()
    return out


LABEL = re.compile(r"(\.L)?(BB|func_begin|func_end|tmp)\d+")
COMMENT_GAP = re.compile(r"\s*;")                                  # comments are aligned behind labels whose length follows the numbers


def kernels(text):
    """{symbol: (instructions, resource usage)} of one assembly file"""
    lines = [ln for ln in text.split("\n") if "__hip_cuid_" not in ln]
    body, res = {}, {}
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"(_Z\w+):", ln)
        if m:
            j = i + 1
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            body[m.group(1)] = [COMMENT_GAP.sub(" ;", LABEL.sub(lambda k: k.group(2), x)) for x in lines[i + 1:j]]
            i = j
        m = re.match(r"\t\.amdhsa_kernel (\S+)", ln)
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            res.setdefault(m.group(1), []).extend(lines[i:j])
            i = j
        m = re.match(r"\t\.set (_Z\w+)\.\w+, ", ln)
        if m:
            res.setdefault(m.group(1), []).append(LABEL.sub(lambda k: k.group(2), ln))
        i += 1
    # amdhsa.kernels: a YAML list, one item per kernel, each with its .name
    if "amdhsa.kernels:" in lines:
        a = lines.index("amdhsa.kernels:")
        b = a + 1
        while lines[b].startswith("  "):
            b += 1
        item = []
        for ln in lines[a + 1:b] + ["  - end"]:
            if ln.startswith("  - ") and item:
                name = [x.split()[-1] for x in item if x.strip().startswith(".name:")][0]
                res.setdefault(name, []).extend(item)
                item = []
            item.append(ln)
    return {k: (body[k], res.get(k)) for k in body}


def pooled(side):
    """{symbol: (instructions, resource usage, file)} over all files of one side"""
    return {k: v + (f,) for f, text in side.items() for k, v in kernels(text).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", default=",".join(FILES))
    ap.add_argument("--new-files")
    ap.add_argument("base", nargs="?", default="HEAD")
    ap.add_argument("new", nargs="?")
    a = ap.parse_args()
    fa = a.files.split(",")
    fb = (a.new_files or a.files).split(",")
    with tempfile.TemporaryDirectory() as tmp:
        ka, kb = pooled(compile_side(a.base, fa, os.path.join(tmp, "base"))), pooled(compile_side(a.new, fb, os.path.join(tmp, "new")))
    print("%s %s --cuda-device-only -S; %s (%s) vs %s (%s)" % (os.path.basename(HIPCC), " ".join(FLAGS[:-2]), a.base, " ".join(fa),
                                                             a.new or "the working tree", " ".join(fb)))
    bad = False
    for f in fa:
        mine = sorted(k for k in ka if ka[k][2] == f)
        both = [k for k in mine if k in kb]
        nres = sum(ka[k][1] == kb[k][1] for k in both)
        nins = sum(ka[k][0] == kb[k][0] for k in both)
        print("%s: %d instantiations; %d with identical resource usage, %d with identical instructions" % (f, len(mine), nres, nins))
        for k in mine:
            if k not in kb:
                print("  no longer instantiated: " + k)
            elif ka[k][:2] != kb[k][:2]:
                print("  differs: " + k)
            elif kb[k][2] != f:
                print("  identical, now in %s: %s" % (kb[k][2], k))
        bad = bad or nres != len(mine) or nins != len(mine)
    for k in sorted(set(kb) - set(ka)):
        print("  new instantiation (%s): %s" % (kb[k][2], k))
        bad = True
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
