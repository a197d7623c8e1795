#!/bin/bash
# usage: ab.sh <other library> [bench args...]; alternates this tree's library with another build of it (FDC_AMD_LIB, e.g. a libfdc_amd.so built
# from another commit) three times on this box (same process count, same box)
OTHER=$1; shift
for i in 1 2 3; do
  for lib in "" "$OTHER"; do
    FDC_AMD_LIB=${lib:+$(realpath "$lib")} python bench.py --steps 100 --warmup 5 --no-cpu-baseline --no-end-to-end --timing-stride 1 "$@" 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); r=d['roofline']; print('${lib:-this tree}', d['ms_per_step'], r['pipeline_frac'], r['kernel_ms_per_step'], d['verified']['max_rel_err'])"
  done
done
