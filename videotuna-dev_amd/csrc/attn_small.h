// Pieces shared by the short-key attention kernels (attn_small.hip, attn_dual.hip): LDS image geometry and the 32x32 MFMA
// accumulator <-> operand index maps.
#pragma once
#include "common.h"

#define AS_KROW 144          // bytes per row of the row-major K / V images (64 bf16 + 16 B pad)
#define AS_MAXK 128
#define AS_TROW(skp) (((skp) + 8) * 2)     // bytes per row of a transposed image [64][skp + 8]

__device__ __forceinline__ int as_crow(int r, int hh) { return ((r >> 2) << 3) + (hh << 2) + (r & 3); }     // row of C register r (32x32 MFMA)

__device__ __forceinline__ bf16x8 as_pack8(const f32x16& a, int s2) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (bf16_t)a[8 * s2 + e];
    return o;
}
// B / A operand whose contraction index follows the C-register order: slots e <-> index (2 s2 + e/4) * 8 + 4 hh + e%4 of a row of a
// transposed image: two 8-byte reads
__device__ __forceinline__ bf16x8 as_tfrag(const char* row, int s2, int hh) {
    const u32x2 lo = *(const u32x2*)(row + ((2 * s2) * 8 + 4 * hh) * 2);
    const u32x2 hi = *(const u32x2*)(row + ((2 * s2 + 1) * 8 + 4 * hh) * 2);
    u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
    return __builtin_bit_cast(bf16x8, v);
}
