// DoRA (weight-decomposed adapters, peft 0.12 DoraLinearLayer with use_dora=True, no dropout) on the K-extension layout:
//     norm_j = || W_j + s (B A)_j ||_2   (detached),   c_j = m_j / norm_j,   y = b + c (x) (W x + s B A x)
// The fused products already compute W x + s B A x in one GEMM over [W | s B]; DoRA is that sum times one factor per output
// feature, so the engine folds c into the packed operands once per optimizer step and no GEMM or rank-side kernel changes.
// The kernels here: the row norms (vt_dora_norm), the scaled operand refresh (vt_dora_scale, vt_dora_transpose_scale), and the two
// finishes of the backward pass that need the row factor (vt_dora_db_add: dB = diag(c) s g^T T; vt_dora_dm: the magnitude gradient).
#include "common.h"

// ---------------- out[j] = || W_j + scale * B_j A ||_2  (mag == null)  or  mag[j] / that norm ----------------
// W [n d_out, K] bf16, adapter a owns rows [a d_out, (a+1) d_out); A [n r, K] bf16 (adapter a = rows [a r, (a+1) r)); B [n d_out, r]
// bf16, contiguous.  A and B are the bf16 compute copies of the masters, the values the products see; everything else is fp32.
// The rank-r update of a row is formed in registers, never in memory: a wave owns DN_ROWS rows and walks K in 16-byte chunks per lane;
// for each chunk it reads the r chunks of A once (one 1 KB line set per rank row, shared by the four waves of the block through the
// cache) and applies them to its DN_ROWS rows with the rows' scale * B held in LDS (two broadcast 16-byte reads per rank row).
// Every lane sums its squares in chunk order and the lanes are added by a butterfly: the order depends on (K, r) only, so the same
// operands give the same bits -- m initialised from this kernel makes c == 1.0f exactly while B = 0.
#define DN_ROWS 8
#define DN_WAVES 4
#define DN_MAXR 128
__global__ __launch_bounds__(64 * DN_WAVES) void dora_norm_kernel(const bf16_t* __restrict__ W, int ldw, const bf16_t* __restrict__ A, int lda,
                                                                  const bf16_t* __restrict__ B, int N, int d_out, int r, int K, float scale,
                                                                  const float* __restrict__ mag, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float bs[DN_WAVES][DN_MAXR][DN_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j0 = (blockIdx.x * DN_WAVES + wave) * DN_ROWS;          // d_out % DN_ROWS == 0: the rows of a wave share one adapter
    const bool live = j0 < N;
    if (live)
        for (int idx = lane; idx < r * DN_ROWS; idx += 64) {
            const int i = idx / DN_ROWS, q = idx - i * DN_ROWS;
            bs[wave][i][q] = scale * bf2f(B[(size_t)(j0 + q) * r + i]);
        }
    __syncthreads();
    if (!live) return;
    const bf16_t* Aa = A + (size_t)(j0 / d_out) * r * lda;
    float acc[DN_ROWS];
#pragma unroll
    for (int q = 0; q < DN_ROWS; ++q) acc[q] = 0.f;
    for (int c = lane; c < (K >> 3); c += 64) {
        float v[DN_ROWS][8];
#pragma unroll
        for (int q = 0; q < DN_ROWS; ++q) unpack8(*(const u32x4*)(W + (size_t)(j0 + q) * ldw + c * 8), v[q]);
        for (int i = 0; i < r; ++i) {
            float a[8];
            unpack8(*(const u32x4*)(Aa + (size_t)i * lda + c * 8), a);
            const f32x4 b0 = *(const f32x4*)&bs[wave][i][0], b1 = *(const f32x4*)&bs[wave][i][4];
#pragma unroll
            for (int q = 0; q < DN_ROWS; ++q) {
                const float b = q < 4 ? b0[q & 3] : b1[q & 3];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[q][e] = __builtin_fmaf(b, a[e], v[q][e]);
            }
        }
#pragma unroll
        for (int q = 0; q < DN_ROWS; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[q] = __builtin_fmaf(v[q][e], v[q][e], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < DN_ROWS; ++q) acc[q] = wave_sum(acc[q]);
    if (lane < DN_ROWS) {
        float s = acc[0];
#pragma unroll
        for (int q = 1; q < DN_ROWS; ++q) s = lane == q ? acc[q] : s;
        const float nrm = sqrtf(s);
        out[j0 + lane] = mag != nullptr ? mag[j0 + lane] / nrm : nrm;
    }
}
extern "C" int vt_dora_norm(const void* W, int ldw, const void* A, int lda, const void* B, int n_adapters, int d_out, int r, int K,
                            float scale, const float* mag, float* out, void* stream) {
    if (n_adapters <= 0 || n_adapters > 3 || d_out <= 0 || (d_out % DN_ROWS) || r <= 0 || r > DN_MAXR || K <= 0 || (K % 8) || (ldw % 8) ||
        ldw < K || (lda % 8) || lda < K)
        return VT_ERR_BAD_SHAPE;
    if (W == nullptr || A == nullptr || B == nullptr || out == nullptr) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)W) | ((uintptr_t)A)) & 15) return VT_ERR_BAD_ALIGN;
    if ((((uintptr_t)B) & 1) || ((((uintptr_t)mag) | ((uintptr_t)out)) & 3)) return VT_ERR_BAD_ALIGN;
    const int N = n_adapters * d_out;
    const int blocks = (N + DN_WAVES * DN_ROWS - 1) / (DN_WAVES * DN_ROWS);
    hipLaunchKernelGGL(dora_norm_kernel, dim3(blocks), dim3(64 * DN_WAVES), 0, (hipStream_t)stream, (const bf16_t*)W, ldw, (const bf16_t*)A, lda,
                       (const bf16_t*)B, N, d_out, r, K, scale, mag, out);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---------------- dst[j, k] = bf16(c[BYCOL ? k : j] * src[j, k]),  one round-to-nearest-even of the fp32 product ----------------
// The scaled refresh of an operand whose orientation the source already has: the base columns of the forward operand [c W | c s B] from
// the pristine weight (factor per row), and, in place (src == dst), the extension columns behind them (per row), the s B^T extension rows
// of a transposed operand and w2_bt (per column).  16-byte loads and stores, a grid-stride loop over the chunks.
template <bool BYCOL>
__global__ __launch_bounds__(256) void dora_scale_kernel(const bf16_t* src, long long lds_, bf16_t* dst, long long ldd, const float* __restrict__ c,
                                                        int rows, int cols) {
    const int nch = cols >> 3;
    const long long total = (long long)rows * nch;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long j = i / nch;
        const int ch = (int)(i - j * nch);
        float v[8];
        unpack8(*(const u32x4*)(src + j * lds_ + ch * 8), v);
        if constexpr (BYCOL) {
            const f32x4 c0 = *(const f32x4*)(c + ch * 8), c1 = *(const f32x4*)(c + ch * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] *= c0[e]; v[e + 4] *= c1[e]; }
        } else {
            const float cj = c[j];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= cj;
        }
        *(u32x4*)(dst + j * ldd + ch * 8) = pack8(v);
    }
}
extern "C" int vt_dora_scale(const void* src, long long lds_, void* dst, long long ldd, const float* c, int rows, int cols, int by_col,
                             void* stream) {
    if (rows <= 0 || cols <= 0 || (cols % 8) || (lds_ % 8) || (ldd % 8) || lds_ < cols || ldd < cols || c == nullptr) return VT_ERR_BAD_SHAPE;
    if (((((uintptr_t)src) | ((uintptr_t)dst)) & 15) || (((uintptr_t)c) & (by_col ? 15 : 3))) return VT_ERR_BAD_ALIGN;
    const long long total = (long long)rows * (cols >> 3), b = (total + 255) / 256;
    const dim3 grid((unsigned)(b > 8192 ? 8192 : b));
    if (by_col)
        hipLaunchKernelGGL(dora_scale_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, lds_, (bf16_t*)dst, ldd, c, rows, cols);
    else
        hipLaunchKernelGGL(dora_scale_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, lds_, (bf16_t*)dst, ldd, c, rows, cols);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---------------- dst[k, j] = bf16(c[j] * src[j, k]): the base part of a transposed operand from the pristine weight ----------------
// vt_transpose_bf16's 64 x 64 tile through LDS (16-byte global loads and stores on both sides, the 66-element row pitch that keeps the
// column reads off one bank), with the factor of the source row applied, and rounded once, on the way in.
__global__ __launch_bounds__(256) void dora_transpose_scale_kernel(const bf16_t* __restrict__ src, long long src_ld, bf16_t* __restrict__ dst,
                                                                   long long dst_ld, const float* __restrict__ c, int rows, int cols) {
    __shared__ unsigned short tile[64][66];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (t >> 3) + 32 * i, ch = t & 7;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r0 + r < rows && c0 + ch * 8 < cols) {
            float f[8];
            unpack8(*(const u32x4*)(src + (long long)(r0 + r) * src_ld + c0 + ch * 8), f);
            const float cj = c[r0 + r];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] *= cj;
            v = pack8(f);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) *(unsigned int*)&tile[r][ch * 8 + 2 * e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cc = (t >> 3) + 32 * i, ch = t & 7;            // output row cc (a source column), output columns 8 ch .. (source rows)
        if (c0 + cc < cols && r0 + ch * 8 < rows) {
            u32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (unsigned)tile[ch * 8 + 2 * e][cc] | ((unsigned)tile[ch * 8 + 2 * e + 1][cc] << 16);
            *(u32x4*)(dst + (long long)(c0 + cc) * dst_ld + r0 + ch * 8) = v;
        }
    }
}
extern "C" int vt_dora_transpose_scale(const void* src, long long src_ld, void* dst, long long dst_ld, const float* c, int rows, int cols,
                                       void* stream) {
    if (rows <= 0 || cols <= 0 || (rows % 8) || (cols % 8) || (src_ld % 8) || (dst_ld % 8) || src_ld < cols || dst_ld < rows || c == nullptr)
        return VT_ERR_BAD_SHAPE;
    if (((((uintptr_t)src) | ((uintptr_t)dst)) & 15) || (((uintptr_t)c) & 3)) return VT_ERR_BAD_ALIGN;
    const dim3 grid((cols + 63) / 64, (rows + 63) / 64);
    if (grid.y > 65535) return VT_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(dora_transpose_scale_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, src_ld, (bf16_t*)dst, dst_ld, c,
                       rows, cols);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---------------- G[j, i] += c[j] * S[j, i]: dB = diag(c) s g^T T from the product s g^T T that a tn kernel left in a zeroed scratch ----------------
__global__ __launch_bounds__(256) void dora_db_add_kernel(float* __restrict__ G, const float* __restrict__ S, const float* __restrict__ c,
                                                          long long total, int r) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) G[i] += c[i / r] * S[i];
}
extern "C" int vt_dora_db_add(float* G, const float* S, const float* c, int N, int r, void* stream) {
    if (N <= 0 || r <= 0 || r > DN_MAXR || G == nullptr || S == nullptr || c == nullptr) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)G) | ((uintptr_t)S) | ((uintptr_t)c)) & 3) return VT_ERR_BAD_ALIGN;
    const long long total = (long long)N * r;
    hipLaunchKernelGGL(dora_db_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, S, c, total, r);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---------------- dm[j] += (sum_gy[j] - bias[j] * sum_g[j]) / mag[j] ----------------
// The magnitude gradient dm_j = sum_m g[m, j] (y[m, j] - b_j) / m_j (the norm is detached, W x + s B A x = (y - b) / c) from the two
// column sums that vt_group_colsum(X = g, Y = y) produces.  bias: bf16 or null.
__global__ __launch_bounds__(256) void dora_dm_kernel(const float* __restrict__ sg, const float* __restrict__ sgy, const bf16_t* __restrict__ bias,
                                                      const float* __restrict__ mag, float* __restrict__ dm, int N) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < N) dm[j] += (sgy[j] - (bias != nullptr ? bf2f(bias[j]) : 0.f) * sg[j]) / mag[j];
}
extern "C" int vt_dora_dm(const float* sum_g, const float* sum_gy, const void* bias, const float* mag, float* dm, int N, void* stream) {
    if (N <= 0 || sum_g == nullptr || sum_gy == nullptr || mag == nullptr || dm == nullptr) return VT_ERR_BAD_SHAPE;
    if (((((uintptr_t)sum_g) | ((uintptr_t)sum_gy) | ((uintptr_t)mag) | ((uintptr_t)dm)) & 3) || (((uintptr_t)bias) & 1)) return VT_ERR_BAD_ALIGN;
    hipLaunchKernelGGL(dora_dm_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, sum_g, sum_gy, (const bf16_t*)bias, mag, dm, N);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
