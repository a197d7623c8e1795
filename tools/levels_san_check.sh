#!/bin/bash
# The argument paths of the five channel-level entries under AddressSanitizer + UBSan: tests/cpp/levels_args_check.cpp (a program with its own main)
# linked against the library's objects with their HOST code instrumented.  For a machine WITHOUT a device (CPU build host): never run it on a GPU machine.
# Output: gr-fdc_amd/_san/levels_args_check (not committed).
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT/gr-fdc_amd/csrc"
OUT="$ROOT/gr-fdc_amd/_san/levels_obj"
mkdir -p "$OUT"
SRCS="fdc_api fdc_plan fdc_enqueue fdc_work fdc_faces fdc_kernels fdc_postpass fdc_fast256 fdc_block256 fdc_block512 fdc_block1024 fdc_blocknarrow fdc_chanwide fdc_fused4096 fdc_sinks fdc_sinks_host fdc_sinks_dev fdc_group fdc_waterfall"
printf '%s\n' $SRCS | xargs -P "${JOBS:-8}" -I{} /opt/rocm/bin/hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
    -Xarch_host -fno-omit-frame-pointer -Wno-unused-result -c {}.hip -o "$OUT/{}.o"
/opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
    -x hip ../../tests/cpp/levels_args_check.cpp -c -o "$OUT/levels_args_check.o"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o ../_san/levels_args_check "$OUT"/*.o -Wl,-rpath,/opt/rocm/lib -lpthread
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 ../_san/levels_args_check
