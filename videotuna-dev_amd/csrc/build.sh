#!/bin/bash
# Build libvt355.so for gfx950 (cross-compiles without a GPU).  Usage: build.sh [outdir]
# VT_OBJ_DIR / VT_LIB_NAME / VT_SCHED_<file>=<strategy> let tools/ build flag experiments next to the shipped library.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${1:-$HERE/..}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wno-unused-result ${VT_EXTRA_FLAGS:-}"
OBJ="${VT_OBJ_DIR:-$HERE/obj}"
LIB="${VT_LIB_NAME:-libvt355.so}"
mkdir -p "$OBJ"
# per-file LLVM scheduling strategy (VT_SCHED_<file>=max-ilp ...).  Measured, r01: max-ilp helps the four-wave attention
# backward (15.70 -> 15.33 ms) but not the shipped eight-wave one (14.3 -> 15.2) nor the GEMMs (-2..4 %): default everywhere.
sched_of() { local v="VT_SCHED_$1"; if [ -n "${!v:-}" ]; then echo "${!v}"; fi; }
pids=()
for f in api gemm_bf16 gemm_big_bf16 gemm_pc_bf16 gemm_nt_bf16 attn_fwd attn_bwd norm elementwise lora lora_wide dora reduce t5 groupnorm conv3d convnd unet_ops attn_small attn_dual attn_relpos attn_gen gemm_fp8 gemm_mxfp8 qknorm128 attn128 sampler; do
  if [ ! -f "$OBJ/$f.o" ] || [ "$HERE/$f.hip" -nt "$OBJ/$f.o" ] || [ "$HERE/common.h" -nt "$OBJ/$f.o" ] || [ "$HERE/gemm_epilogue.h" -nt "$OBJ/$f.o" ] || [ "$HERE/attn_small.h" -nt "$OBJ/$f.o" ] || [ "$HERE/build.sh" -nt "$OBJ/$f.o" ]; then
    st="$(sched_of $f)"; extra=""; [ -n "$st" ] && [ "$st" != default ] && extra="-mllvm -amdgpu-sched-strategy=$st"
    $HIPCC $FLAGS $extra -c "$HERE/$f.hip" -o "$OBJ/$f.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/$LIB" "$OBJ"/*.o
echo "built $OUT/$LIB"
# libvt355_test.so: the attention backward with CH_SPIN_LIMIT=0 (every dQ hand-off wait that is not satisfied at once times out)
# under the symbol suffix _tmo -- only tests/ load it (the forced time-out test of the sticky error word / optimizer guard)
if [ -z "${VT_LIB_NAME:-}" ]; then
  T="$OBJ/../obj_test"; mkdir -p "$T"
  if [ ! -f "$T/attn_bwd_tmo.o" ] || [ "$HERE/attn_bwd.hip" -nt "$T/attn_bwd_tmo.o" ] || [ "$HERE/common.h" -nt "$T/attn_bwd_tmo.o" ]; then
    $HIPCC $FLAGS -DVT_SUFFIX=_tmo -DCH_SPIN_LIMIT=0 -c "$HERE/attn_bwd.hip" -o "$T/attn_bwd_tmo.o"
  fi
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/libvt355_test.so" "$T"/*.o
  echo "built $OUT/libvt355_test.so"
fi
