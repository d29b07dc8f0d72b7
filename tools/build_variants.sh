#!/bin/bash
# Experimental: the control of an in-process A/B.  Compiles the UNCHANGED csrc/attn_bwd.hip a second time under the symbol suffix _same into
# libvt355_exp.so, so that tools/kbench_variants.py can time two copies of the same code against each other (what the run-to-run spread of the
# method is).  Variants with other flags: tools/build_exp.sh.  The variants this script used to build are listed in csrc/exp/README.md,
# "Variants removed from attn_bwd.hip / attn_fwd.hip".  Not part of build().
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")/../videotuna-dev_amd/csrc" && pwd)"
OUT="$HERE/../libvt355_exp.so"
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics"
mkdir -p "$HERE/obj_exp"; rm -f "$HERE"/obj_exp/*.o
hipcc $F -DVT_SUFFIX=_same -c "$HERE/attn_bwd.hip" -o "$HERE/obj_exp/bwd_same.o"
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" "$HERE"/obj_exp/*.o
echo "built $OUT"
