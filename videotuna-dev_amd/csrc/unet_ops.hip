// Memory-bound kernels of the VideoCrafter2 UNet path (BASELINE configs[3]) on ONE channels-last layout
// [N, P, C] / [B, T, H, W, C] (bf16 activations, fp32 statistics and parameter gradients):
//   GroupNorm backward (+ the SiLU that follows it) .. GroupNormSpecific -> SiLU of ResBlock / TemporalConvBlock / out, the plain
//                                                      GroupNorm of Spatial/TemporalTransformer.norm
//                                                      (lvdm/modules/networks/openaimodel3d.py:229-255, 278-296, 643-648;
//                                                       lvdm/modules/attention.py:337-339, 421-423; utils.py:192-203)
//   GEGLU forward / backward ......................... attention.py:522-529  (x * gelu(gate), exact erf GELU)
//   frame <-> pixel row transposes ................... the `b c t h w -> (b h w) t c` rearranges of TemporalTransformer.forward
//                                                      (attention.py:476-481, 509-516) as ONE row permutation each way
//   nearest x2 upsample forward / backward ........... Upsample.forward (openaimodel3d.py:112-120)
//   zero insertion ................................... input gradient of Downsample.op (stride-2 conv, :71-79): dX = conv(stride 1) of
//                                                      the zero-upsampled dY with the flipped weight
//   row add .......................................... gradient accumulation where a tensor feeds two consumers (residuals, skips)
//   eps-prediction MSE loss forward / backward ....... LVDMFlow.p_losses (lvdm/ddpm3d.py:787-847), q_sample (schedulers/ddpm.py:216-222)
// All HBM-bound, one read + one write of each operand unless noted.
#include "common.h"

#define UO_THREADS 256

__device__ __forceinline__ float silu_sig(float g) { return 1.0f - __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(g * 1.4426950408889634f) + 1.0f); }

// ----------------------------------------------------------------------------------------------------------------- GroupNorm backward
// forward (groupnorm.hip): g = x * a[n,c] + b[n,c], y = SILU ? g * sigmoid(g) : g; ws_fwd = [N][4][C]: mean_c | rstd_c | a | b.
// backward: dg = dy * (SILU ? s (1 + g (1 - s)) : 1);  xh = (x - mean) rstd
//   S1[n,c] = sum_p dg, S2[n,c] = sum_p dg * xh              (pass 1, per-channel, fp32 atomics into ws_bwd [N][4][C])
//   dgamma[c] += sum_n S2, dbeta[c] += sum_n S1;  per group: A = sum_c gamma S2, Bs = sum_c gamma S1, cnt = P * C/G
//   dx = dg * a + x * k2 + k3,   k2 = -rstd^2 A / cnt,  k3 = -rstd Bs / cnt - mean k2       (pass 2: finalize, pass 3: apply)
template <bool SILU>
__global__ __launch_bounds__(UO_THREADS) void gn_bwd_stats_kernel(const bf16_t* dy, long long lddy, const bf16_t* x, long long ldx, long long P,
                                                                 int C, const float* wsf, float* wsb, int slabs) {
    extern __shared__ float red[];                 // [2][C]
    const int n = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
    const int nch = C >> 3;
    for (int i = tid; i < 2 * C; i += UO_THREADS) red[i] = 0.f;
    __syncthreads();
    const float* wf = wsf + (size_t)n * 4 * C;
    const long long p0 = P * slab / slabs, p1 = P * (slab + 1) / slabs;
    for (int c0 = 0; c0 < nch; c0 += UO_THREADS) {
        const int ncl = min(nch - c0, UO_THREADS);
        const int lanes = UO_THREADS / ncl * ncl;
        if (tid < lanes) {
            const int c = c0 + tid % ncl, row = tid / ncl, rows = lanes / ncl;
            float mean[8], rstd[8], a[8], b[8], s1[8], s2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                mean[j] = wf[c * 8 + j]; rstd[j] = wf[C + c * 8 + j]; a[j] = wf[2 * C + c * 8 + j]; b[j] = wf[3 * C + c * 8 + j];
                s1[j] = 0.f; s2[j] = 0.f;
            }
            for (long long p = p0 + row; p < p1; p += 2 * rows) {          // two positions (four loads) in flight per thread
                u32x4 rx[2], rd[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const long long pp = p + (long long)u * rows;
                    rx[u] = (u32x4){0u, 0u, 0u, 0u}; rd[u] = rx[u];
                    if (pp < p1) {
                        rx[u] = *(const u32x4*)(x + ((long long)n * P + pp) * ldx + c * 8);
                        rd[u] = *(const u32x4*)(dy + ((long long)n * P + pp) * lddy + c * 8);
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float xv[8], dv[8];
                    unpack8(rx[u], xv); unpack8(rd[u], dv);          // a position past the slab has dy = 0: contributes nothing
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float dg = dv[j];
                        if (SILU) {
                            const float g = xv[j] * a[j] + b[j];
                            const float sg = silu_sig(g);
                            dg *= sg * (1.0f + g * (1.0f - sg));
                        }
                        s1[j] += dg;
                        s2[j] += dg * (xv[j] - mean[j]) * rstd[j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { atomicAdd(red + c * 8 + j, s1[j]); atomicAdd(red + C + c * 8 + j, s2[j]); }
        }
    }
    __syncthreads();
    float* w = wsb + (size_t)n * 4 * C;
    for (int i = tid; i < 2 * C; i += UO_THREADS) atomicAdd(w + i, red[i]);
}

// one block per sample, a thread per channel, group sums through LDS (see gn_finalize_kernel)
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(const float* wsf, float* wsb, const bf16_t* gamma, float* dgamma, float* dbeta, long long P, int C, int G) {
    extern __shared__ float gsh[];                  // [4][G]: A | Bs | k2 | k3
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* wf = wsf + (size_t)n * 4 * C;
    float* w = wsb + (size_t)n * 4 * C;
    const int cpg = C / G;
    for (int g = tid; g < 2 * G; g += 256) gsh[g] = 0.f;
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float ga = gamma ? bf2f(gamma[c]) : 1.f;
        const float s1 = w[c], s2 = w[C + c];
        atomicAdd(gsh + c / cpg, ga * s2); atomicAdd(gsh + G + c / cpg, ga * s1);
        if (dgamma) atomicAdd(dgamma + c, s2);
        if (dbeta) atomicAdd(dbeta + c, s1);
    }
    __syncthreads();
    const float cnt = (float)cpg * (float)P;
    for (int g = tid; g < G; g += 256) {
        const float mean = wf[g * cpg], rstd = wf[C + g * cpg];
        const float k2 = -rstd * rstd * gsh[g] / cnt;
        gsh[2 * G + g] = k2;
        gsh[3 * G + g] = -rstd * gsh[G + g] / cnt - mean * k2;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) { w[2 * C + c] = gsh[2 * G + c / cpg]; w[3 * C + c] = gsh[3 * G + c / cpg]; }
}

template <bool SILU, bool ACC>
__global__ __launch_bounds__(UO_THREADS) void gn_bwd_apply_kernel(const bf16_t* dy, long long lddy, const bf16_t* x, long long ldx, bf16_t* dx,
                                                                 long long lddx, long long P, int C, const float* wsf, const float* wsb) {
    const int n = blockIdx.y;
    const int nch = C >> 3;
    const float* a = wsf + (size_t)n * 4 * C + 2 * C;
    const float* b = a + C;
    const float* k2 = wsb + (size_t)n * 4 * C + 2 * C;
    const float* k3 = k2 + C;
    const long long total = P * nch;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const long long p = i / nch;
        const int c = (int)(i - p * nch) * 8;
        float xv[8], dv[8], o[8];
        unpack8(*(const u32x4*)(x + ((long long)n * P + p) * ldx + c), xv);
        unpack8(*(const u32x4*)(dy + ((long long)n * P + p) * lddy + c), dv);
        if (ACC) unpack8(*(const u32x4*)(dx + ((long long)n * P + p) * lddx + c), o);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float dg = dv[j];
            const float aj = a[c + j];
            if (SILU) {
                const float g = xv[j] * aj + b[c + j];
                const float s = silu_sig(g);
                dg *= s * (1.0f + g * (1.0f - s));
            }
            const float r = dg * aj + xv[j] * k2[c + j] + k3[c + j];
            o[j] = ACC ? o[j] + r : r;
        }
        *(u32x4*)(dx + ((long long)n * P + p) * lddx + c) = pack8(o);
    }
}

// dy, x: bf16 [N, P, C]; ws_fwd: the forward call's workspace (vt_groupnorm_silu_cl leaves mean | rstd | a | b per (n, c) in it);
// ws_bwd: fp32 scratch of vt_groupnorm_ws_bytes(N, C) bytes; dgamma / dbeta: fp32 [C], ACCUMULATED (or null); dx: bf16 [N, P, C],
// overwritten, or added to when accumulate != 0 (the tensor also feeds another consumer).
extern "C" int vt_groupnorm_silu_bwd_cl(const void* dy, long long lddy, const void* x, long long ldx, const void* gamma,
                                        const float* ws_fwd, float* ws_bwd, long long ws_bytes, void* dx, long long lddx,
                                        float* dgamma, float* dbeta, int N, long long P, int C, int G, int silu, int accumulate, void* stream) {
    if (N <= 0 || P <= 0 || C <= 0 || G <= 0 || (C % G) || (C % 8) || (ldx % 8) || (lddy % 8) || (lddx % 8) || ldx < C || lddy < C || lddx < C)
        return VT_ERR_BAD_SHAPE;
    if (N > 65535 || ws_fwd == nullptr || ws_bwd == nullptr || ws_bytes < (long long)N * 4 * C * 4) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)x) | ((uintptr_t)dy) | ((uintptr_t)dx) | ((uintptr_t)ws_fwd) | ((uintptr_t)ws_bwd)) & 15) return VT_ERR_BAD_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws_bwd, 0, (size_t)N * 4 * C * 4, st) != hipSuccess) return VT_ERR_LAUNCH;
    int slabs;
    {   // as gn_slabs (groupnorm.hip): ~1.5 blocks per CU over all samples, at least 4 positions per thread row
        const int nch = C >> 3;
        const int rows = nch >= 256 ? 1 : 256 / nch;
        long long want = (384 + N - 1) / N;
        const long long cap = P / (4LL * rows);
        if (want > cap) want = cap;
        slabs = (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    }
    if (silu) hipLaunchKernelGGL(gn_bwd_stats_kernel<true>, dim3(slabs, N), dim3(UO_THREADS), 2 * C * sizeof(float), st, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, P, C, ws_fwd, ws_bwd, slabs);
    else hipLaunchKernelGGL(gn_bwd_stats_kernel<false>, dim3(slabs, N), dim3(UO_THREADS), 2 * C * sizeof(float), st, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, P, C, ws_fwd, ws_bwd, slabs);
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(N), dim3(256), 4 * G * sizeof(float), st, ws_fwd, ws_bwd, (const bf16_t*)gamma, dgamma, dbeta, P, C, G);
    const long long total = P * (C >> 3);
    long long blocks = (total + UO_THREADS - 1) / UO_THREADS;
    if (blocks > 8192) blocks = 8192;
    dim3 grid((unsigned)blocks, N);
#define GNB(S, A) hipLaunchKernelGGL((gn_bwd_apply_kernel<S, A>), grid, dim3(UO_THREADS), 0, st, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, (bf16_t*)dx, lddx, P, C, ws_fwd, ws_bwd)
    if (silu) { if (accumulate) GNB(true, true); else GNB(true, false); }
    else { if (accumulate) GNB(false, true); else GNB(false, false); }
#undef GNB
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ----------------------------------------------------------------------------------------------------------------- GEGLU
__device__ __forceinline__ float gelu_erf_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad_f(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}
// h: [M, 2F] = (a | gate) from GEGLU.proj; y[m, f] = a * gelu(gate)
__global__ __launch_bounds__(UO_THREADS) void geglu_fwd_kernel(const bf16_t* h, long long ldh, bf16_t* y, long long ldy, long long M, int F) {
    const int nch = F >> 3;
    const long long total = M * nch;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const long long m = i / nch;
        const int c = (int)(i - m * nch) * 8;
        float a[8], g[8];
        unpack8(*(const u32x4*)(h + m * ldh + c), a);
        unpack8(*(const u32x4*)(h + m * ldh + F + c), g);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] *= gelu_erf_f(g[j]);
        *(u32x4*)(y + m * ldy + c) = pack8(a);
    }
}
__global__ __launch_bounds__(UO_THREADS) void geglu_bwd_kernel(const bf16_t* dy, long long lddy, const bf16_t* h, long long ldh, bf16_t* dh, long long lddh,
                                                              long long M, int F) {
    const int nch = F >> 3;
    const long long total = M * nch;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const long long m = i / nch;
        const int c = (int)(i - m * nch) * 8;
        float a[8], g[8], d[8], da[8], dg[8];
        unpack8(*(const u32x4*)(h + m * ldh + c), a);
        unpack8(*(const u32x4*)(h + m * ldh + F + c), g);
        unpack8(*(const u32x4*)(dy + m * lddy + c), d);
#pragma unroll
        for (int j = 0; j < 8; ++j) { da[j] = d[j] * gelu_erf_f(g[j]); dg[j] = d[j] * a[j] * gelu_erf_grad_f(g[j]); }
        *(u32x4*)(dh + m * lddh + c) = pack8(da);
        *(u32x4*)(dh + m * lddh + F + c) = pack8(dg);
    }
}
static unsigned uo_blocks(long long total) { long long b = (total + UO_THREADS - 1) / UO_THREADS; return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b)); }
extern "C" int vt_geglu_fwd(const void* h, long long ldh, void* y, long long ldy, long long M, int F, void* stream) {
    if (M <= 0 || F <= 0 || (F % 8) || (ldh % 8) || (ldy % 8) || ldh < 2 * F || ldy < F) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)h) | ((uintptr_t)y)) & 15) return VT_ERR_BAD_ALIGN;
    hipLaunchKernelGGL(geglu_fwd_kernel, dim3(uo_blocks(M * (F >> 3))), dim3(UO_THREADS), 0, (hipStream_t)stream, (const bf16_t*)h, ldh, (bf16_t*)y, ldy, M, F);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
extern "C" int vt_geglu_bwd(const void* dy, long long lddy, const void* h, long long ldh, void* dh, long long lddh, long long M, int F, void* stream) {
    if (M <= 0 || F <= 0 || (F % 8) || (ldh % 8) || (lddy % 8) || (lddh % 8) || ldh < 2 * F || lddh < 2 * F || lddy < F) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)h) | ((uintptr_t)dy) | ((uintptr_t)dh)) & 15) return VT_ERR_BAD_ALIGN;
    hipLaunchKernelGGL(geglu_bwd_kernel, dim3(uo_blocks(M * (F >> 3))), dim3(UO_THREADS), 0, (hipStream_t)stream, (const bf16_t*)dy, lddy, (const bf16_t*)h, ldh,
                       (bf16_t*)dh, lddh, M, F);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ----------------------------------------------------------------------------------------------------------------- row-wise helpers
// out[m, :] = a[m, :] + b[m, :]   (b may alias out)
__global__ __launch_bounds__(UO_THREADS) void add_rows_kernel(const bf16_t* a, long long lda, const bf16_t* b, long long ldb, bf16_t* o, long long ldo,
                                                             long long M, int C) {
    const int nch = C >> 3;
    const long long total = M * nch;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const long long m = i / nch;
        const int c = (int)(i - m * nch) * 8;
        float x[8], y[8];
        unpack8(*(const u32x4*)(a + m * lda + c), x);
        unpack8(*(const u32x4*)(b + m * ldb + c), y);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] += y[j];
        *(u32x4*)(o + m * ldo + c) = pack8(x);
    }
}
extern "C" int vt_add_rows_bf16(const void* a, long long lda, const void* b, long long ldb, void* out, long long ldo, long long M, int C, void* stream) {
    if (M <= 0 || C <= 0 || (C % 8) || (lda % 8) || (ldb % 8) || (ldo % 8) || lda < C || ldb < C || ldo < C) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)out)) & 15) return VT_ERR_BAD_ALIGN;
    hipLaunchKernelGGL(add_rows_kernel, dim3(uo_blocks(M * (C >> 3))), dim3(UO_THREADS), 0, (hipStream_t)stream, (const bf16_t*)a, lda, (const bf16_t*)b, ldb,
                       (bf16_t*)out, ldo, M, C);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ----------------------------------------------------------------------------------------------------------------- dropout
// y[m, c] = keep(m, c) ? x[m, c] / (1 - p) : 0 with keep = Philox4x32-10(key = seed, counter = (offset + e / 4, 0, 0, 0))[e % 4] >= p * 2^32,
// e = m * C + c: the mask is a pure function of (seed, offset, element index), so the backward pass calls the same kernel on the
// gradient with the same (seed, offset) and no mask is stored.  nn.Dropout of TemporalConvBlock (openaimodel3d.py:278-296, p = 0.1)
// in training mode.  mask_out (uint8 [M, C], optional): the keep bits, for parity tests (the oracle applies the exported mask).
__global__ __launch_bounds__(UO_THREADS) void dropout_kernel(const bf16_t* x, long long ldx, bf16_t* y, long long ldy, long long M, int C, unsigned thresh,
                                                            float inv_keep, unsigned long long seed, unsigned long long offset, unsigned char* mask) {
    const int nch = C >> 3;
    const long long total = M * nch;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const long long m = i / nch;
        const int c = (int)(i - m * nch) * 8;
        const unsigned long long ctr = offset + (unsigned long long)(m * C + c) / 4;      // two consecutive counters cover this 8-element chunk
        unsigned rnd[8];
        philox4x32_10((unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), rnd);
        philox4x32_10((unsigned)(ctr + 1), (unsigned)((ctr + 1) >> 32), 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), rnd + 4);
        float v[8];
        unpack8(*(const u32x4*)(x + m * ldx + c), v);
        unsigned long long mbits = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool keep = rnd[j] >= thresh;
            v[j] = keep ? v[j] * inv_keep : 0.f;
            mbits |= (unsigned long long)(keep ? 1 : 0) << (8 * j);
        }
        *(u32x4*)(y + m * ldy + c) = pack8(v);
        if (mask != nullptr) *(unsigned long long*)(mask + m * C + c) = mbits;
    }
}
extern "C" int vt_dropout_bf16(const void* x, long long ldx, void* y, long long ldy, long long M, int C, float p, unsigned long long seed,
                               unsigned long long offset, void* mask_out, void* stream) {
    if (M <= 0 || C <= 0 || (C % 8) || (ldx % 8) || (ldy % 8) || ldx < C || ldy < C || !(p >= 0.f) || !(p < 1.f)) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)x) | ((uintptr_t)y)) & 15 || (((uintptr_t)mask_out) & 7)) return VT_ERR_BAD_ALIGN;
    const double t = (double)p * 4294967296.0;
    const unsigned thresh = t >= 4294967295.0 ? 0xffffffffu : (unsigned)t;
    hipLaunchKernelGGL(dropout_kernel, dim3(uo_blocks(M * (C >> 3))), dim3(UO_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (bf16_t*)y, ldy, M, C,
                       thresh, 1.0f / (1.0f - p), seed, offset, (unsigned char*)mask_out);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// Row gather with an optional add: out[m, :] (+)= src[map(m), :].  MODE 0: [B, A1, A2, C] -> [B, A2, A1, C] (the frame <-> pixel transpose
// of TemporalTransformer, its own inverse with A1 / A2 swapped); MODE 1: nearest x2 upsample [N, H, W] -> [N, 2H, 2W]; MODE 2: zero
// insertion [N, H, W] -> [N, 2H, 2W] (value at even positions, zeros elsewhere); MODE 3: sum of the 2x2 block [N, 2H, 2W] -> [N, H, W]
// (backward of MODE 1).
template <int MODE>
__global__ __launch_bounds__(UO_THREADS) void row_map_kernel(const bf16_t* src, long long lds_, bf16_t* out, long long ldo, long long Mo, int C,
                                                            int d1, int d2, int accumulate) {
    const int nch = C >> 3;
    const long long total = Mo * nch;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const long long m = i / nch;
        const int c = (int)(i - m * nch) * 8;
        float v[8];
        if (MODE == 0) {            // out row (b, a2, a1) <- src row (b, a1, a2); d1 = A1, d2 = A2
            const long long b = m / ((long long)d1 * d2);
            const long long r = m - b * d1 * d2;
            const long long a2 = r / d1, a1 = r - a2 * d1;
            unpack8(*(const u32x4*)(src + ((b * d1 + a1) * d2 + a2) * lds_ + c), v);
        } else if (MODE == 1 || MODE == 2) {       // out [N, 2H, 2W]; d1 = H, d2 = W of the source
            const long long n = m / (4LL * d1 * d2);
            const long long r = m - n * 4LL * d1 * d2;
            const int ho = (int)(r / (2 * d2)), wo = (int)(r - (long long)ho * 2 * d2);
            if (MODE == 1 || ((ho & 1) == 0 && (wo & 1) == 0)) unpack8(*(const u32x4*)(src + ((n * d1 + (ho >> 1)) * d2 + (wo >> 1)) * lds_ + c), v);
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = 0.f;
            }
        } else {                    // MODE 3: out [N, H, W] <- sum of src [N, 2H, 2W] blocks; d1 = H, d2 = W of the OUTPUT
            const long long n = m / ((long long)d1 * d2);
            const long long r = m - n * (long long)d1 * d2;
            const int h = (int)(r / d2), w = (int)(r - (long long)h * d2);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float t[8];
                unpack8(*(const u32x4*)(src + ((n * 2 * d1 + 2 * h + (q >> 1)) * 2 * d2 + 2 * w + (q & 1)) * lds_ + c), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] += t[j];
            }
        }
        if (accumulate) {
            float o[8];
            unpack8(*(const u32x4*)(out + m * ldo + c), o);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += o[j];
        }
        *(u32x4*)(out + m * ldo + c) = pack8(v);
    }
}
// mode 0: src [B, d1, d2, C] -> out [B, d2, d1, C] (Mo = B*d1*d2); 1: nearest x2, src [N, d1, d2, C] -> out [N, 2 d1, 2 d2, C];
// 2: zero insertion, same shapes as 1; 3: 2x2 block sum, src [N, 2 d1, 2 d2, C] -> out [N, d1, d2, C].  nb = B or N.
extern "C" int vt_row_map_bf16(const void* src, long long lds_, void* out, long long ldo, int mode, long long nb, int d1, int d2, int C,
                               int accumulate, void* stream) {
    if (nb <= 0 || d1 <= 0 || d2 <= 0 || C <= 0 || (C % 8) || (lds_ % 8) || (ldo % 8) || lds_ < C || ldo < C || mode < 0 || mode > 3) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)src) | ((uintptr_t)out)) & 15) return VT_ERR_BAD_ALIGN;
    const long long Mo = (mode == 1 || mode == 2) ? nb * 4LL * d1 * d2 : nb * (long long)d1 * d2;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(uo_blocks(Mo * (C >> 3)));
#define RM(MD) hipLaunchKernelGGL(row_map_kernel<MD>, grid, dim3(UO_THREADS), 0, st, (const bf16_t*)src, lds_, (bf16_t*)out, ldo, Mo, C, d1, d2, accumulate)
    if (mode == 0) RM(0); else if (mode == 1) RM(1); else if (mode == 2) RM(2); else RM(3);
#undef RM
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ----------------------------------------------------------------------------------------------------------------- eps-MSE loss
// q_sample: x_t = sqrt_ab[b] * scale[b] * x0 + sqrt_1mab[b] * noise  (fp32 in, bf16 out; scale = scale_arr[t], ddpm3d.py:740-741, or null)
__global__ __launch_bounds__(UO_THREADS) void q_sample_kernel(const float* x0, const float* noise, const float* sa, const float* sb, const float* scale,
                                                             bf16_t* xt, long long per, int B) {
    const long long total = per * B;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const int b = (int)(i / per);
        const float s = scale ? scale[b] : 1.0f;
        xt[i] = f2bf(sa[b] * s * x0[i] + sb[b] * noise[i]);
    }
}
extern "C" int vt_q_sample(const float* x0, const float* noise, const float* sqrt_ab, const float* sqrt_1mab, const float* scale, void* xt,
                           long long per_sample, int B, void* stream) {
    if (per_sample <= 0 || B <= 0) return VT_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(q_sample_kernel, dim3(uo_blocks(per_sample * B)), dim3(UO_THREADS), 0, (hipStream_t)stream, x0, noise, sqrt_ab, sqrt_1mab, scale,
                       (bf16_t*)xt, per_sample, B);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
// loss = mean_b mean_i (pred - target)^2 ; dpred = 2 (pred - target) / (per * B) * gscale   (pred bf16, target fp32)
__global__ __launch_bounds__(UO_THREADS) void mse_loss_kernel(const bf16_t* pred, const float* target, float* loss, bf16_t* dpred, long long total,
                                                             float inv, float gscale) {
    __shared__ float red[UO_THREADS / 64];
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const float d = bf2f(pred[i]) - target[i];
        acc += d * d;
        if (dpred) dpred[i] = f2bf(2.0f * d * inv * gscale);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < UO_THREADS / 64; ++i) s += red[i];
        atomicAdd(loss, s * inv);
    }
}
// loss: fp32 [1], zeroed by the call; dpred (bf16, optional) = d loss / d pred * grad_scale
extern "C" int vt_mse_loss(const void* pred, const float* target, float* loss, void* dpred, long long total, float grad_scale, void* stream) {
    if (total <= 0) return VT_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(loss, 0, 4, st) != hipSuccess) return VT_ERR_LAUNCH;
    long long b = (total + UO_THREADS - 1) / UO_THREADS;
    hipLaunchKernelGGL(mse_loss_kernel, dim3((unsigned)(b > 2048 ? 2048 : b)), dim3(UO_THREADS), 0, st, (const bf16_t*)pred, target, loss, (bf16_t*)dpred, total,
                       1.0f / (float)total, grad_scale);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ----------------------------------------------------------------------------------------------------------------- OpenSora IDDPM loss
// LatentDiffusion.p_losses of OpenSora v1.0 (videotuna/models/opensora/models/iddpm3d.py:1332-1413; EPSILON mean, LEARNED_RANGE variance,
// MSE loss): model output [B, 2C, ...] = (eps_hat | v);  loss = mean_b( mean (eps - eps_hat)^2 + vb_b ),
//   vb_b = KL( q(x_{t-1} | x_t, x0) || N(mean_p, exp(lv)) ) / ln 2   (t > 0)   |   -log-likelihood of the discretised Gaussian / ln 2 (t == 0)
//   lv = frac * max_log + (1 - frac) * min_log, frac = (v + 1) / 2;  mean_p = coef1 * eps_hat + coef2 * x_t  -- the reference feeds the RAW
//   eps_hat where x0 is expected (OpenSoraScheduler.p_mean_variance :497-500, a quirk reproduced on purpose); the mean prediction is
//   detached inside vb (:1366), so d vb flows to v only.
// coef: fp64 [B, 8] = sqrt_ac, sqrt_1mac, coef1, coef2, min_log, max_log, (t == 0), unused -- the reference's posterior tables are
// float64 (np.append(1.0, ...)), so the VB arithmetic runs in fp64 here as it (implicitly) does there.
// out: fp32 in (model output cast to fp32, stdit.py:309); x0, noise fp32; loss3: fp64 [3] = loss, mse, vb (zeroed by the call);
// dout fp32 [B, 2C, ...] = d loss / d out * gscale.
__device__ __forceinline__ double os_cdf(double x) { return 0.5 * (1.0 + tanh(0.7978845608028654 * (x + 0.044715 * x * x * x))); }
__device__ __forceinline__ double os_dcdf(double x) {
    const double u = 0.7978845608028654 * (x + 0.044715 * x * x * x);
    const double th = tanh(u);
    return 0.5 * (1.0 - th * th) * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * x * x);
}
__global__ __launch_bounds__(UO_THREADS) void opensora_loss_kernel(const float* out, const float* x0, const float* noise, const double* coef,
                                                                  double* loss3, float* dout, long long per_c, int C, int B, float gscale) {
    // per_c = elements per channel group (T*H*W); sample b: eps_hat at [b, 0:C], v at [b, C:2C]
    const long long per = per_c * C, total = per * B;
    double a_mse = 0.0, a_vb = 0.0;
    const double inv = 1.0 / ((double)per * (double)B);
    const double LN2 = 0.6931471805599453;
    for (long long i = (long long)blockIdx.x * UO_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * UO_THREADS) {
        const int b = (int)(i / per);
        const long long r = i - (long long)b * per;
        const double* cf = coef + b * 8;
        const long long ie = (long long)b * 2 * per + r, iv = ie + per;
        const double e = out[ie], v = out[iv], xs = x0[i], nz = noise[i];
        const double xt = cf[0] * xs + cf[1] * nz;
        const double d = nz - e;
        a_mse += d * d;
        const double frac = 0.5 * (v + 1.0);
        const double lv = frac * cf[5] + (1.0 - frac) * cf[4];
        const double mp = cf[2] * e + cf[3] * xt;                // REFERENCE QUIRK: raw eps_hat in the place of x0
        double term, dlv;
        if (cf[6] == 0.0) {
            const double mt = cf[2] * xs + cf[3] * xt, lt = cf[4];
            const double dm2 = (mt - mp) * (mt - mp), ex = exp(lt - lv), ev = exp(-lv);
            term = 0.5 * (-1.0 + lv - lt + ex + dm2 * ev);
            dlv = 0.5 * (1.0 - ex - dm2 * ev);
        } else {
            const double ls = 0.5 * lv, is = exp(-ls), c = xs - mp;
            const double zp = is * (c + 1.0 / 255.0), zm = is * (c - 1.0 / 255.0);
            const double cp = os_cdf(zp), cm = os_cdf(zm);
            double ll, dls;           // d z / d ls = -z
            if (xs < -0.999) { const double q = cp > 1e-12 ? cp : 1e-12; ll = log(q); dls = cp > 1e-12 ? os_dcdf(zp) * (-zp) / q : 0.0; }
            else if (xs > 0.999) { const double q = (1.0 - cm) > 1e-12 ? (1.0 - cm) : 1e-12; ll = log(q); dls = (1.0 - cm) > 1e-12 ? -os_dcdf(zm) * (-zm) / q : 0.0; }
            else { const double dl = cp - cm; const double q = dl > 1e-12 ? dl : 1e-12; ll = log(q); dls = dl > 1e-12 ? (os_dcdf(zp) * (-zp) - os_dcdf(zm) * (-zm)) / q : 0.0; }
            term = -ll;
            dlv = -0.5 * dls;
        }
        a_vb += term;
        if (dout != nullptr) {
            dout[ie] = (float)(-2.0 * d * inv * gscale);
            dout[iv] = (float)(dlv * 0.5 * (cf[5] - cf[4]) / LN2 * inv * gscale);
        }
    }
    __shared__ double red[2][UO_THREADS / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a_mse += __shfl_xor(a_mse, o, 64); a_vb += __shfl_xor(a_vb, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a_mse; red[1][threadIdx.x >> 6] = a_vb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = 0.0, v = 0.0;
        for (int i = 0; i < UO_THREADS / 64; ++i) { m += red[0][i]; v += red[1][i]; }
        m *= inv; v *= inv / LN2;
        atomicAdd(loss3 + 1, m); atomicAdd(loss3 + 2, v); atomicAdd(loss3, m + v);
    }
}
extern "C" int vt_opensora_loss(const float* out, const float* x0, const float* noise, const double* coef, double* loss3, float* dout,
                                long long per_channel, int C, int B, float grad_scale, void* stream) {
    if (per_channel <= 0 || C <= 0 || B <= 0) return VT_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(loss3, 0, 24, st) != hipSuccess) return VT_ERR_LAUNCH;
    long long b = (per_channel * C * B + UO_THREADS - 1) / UO_THREADS;
    hipLaunchKernelGGL(opensora_loss_kernel, dim3((unsigned)(b > 1024 ? 1024 : b)), dim3(UO_THREADS), 0, st, out, x0, noise, coef, loss3, dout,
                       per_channel, C, B, grad_scale);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ----------------------------------------------------------------------------------------------------------------- batched transpose
// dst[b][c][r] = src[b][r][c] for nb matrices of rows x cols bf16 (both multiples of 8); matrix b starts at src + b * src_boff and
// dst + b * dst_boff (elements; either may be negative).  The per-step operand packing of full fine-tuning: W^T of every Linear for
// its input gradient (nb = 1), and the input-gradient weight of a convolution -- taps flipped, channels swapped:
// D[ci][T-1-t][co] = S[co][t][ci] is, per tap, the transpose of a [Cout x Cin] matrix with row stride taps * Cin into one with row
// stride taps * Cout (torch did this as flip + permute + reshape + contiguous: three strided copies per weight, 11.6 ms of the UNet's step).
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16_t* __restrict__ src, long long src_ld, long long src_boff, bf16_t* __restrict__ dst,
                                                             long long dst_ld, long long dst_boff, int rows, int cols) {
    __shared__ unsigned short tile[64][66];
    const int b = blockIdx.z;
    const bf16_t* s = src + (long long)b * src_boff;
    bf16_t* d = dst + (long long)b * dst_boff;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (t >> 3) + 32 * i, ch = t & 7;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r0 + r < rows && c0 + ch * 8 < cols) v = *(const u32x4*)(s + (long long)(r0 + r) * src_ld + c0 + ch * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) *(unsigned int*)&tile[r][ch * 8 + 2 * e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = (t >> 3) + 32 * i, ch = t & 7;            // output row c (a source column), output columns 8 ch .. (source rows)
        if (c0 + c < cols && r0 + ch * 8 < rows) {
            u32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (unsigned)tile[ch * 8 + 2 * e][c] | ((unsigned)tile[ch * 8 + 2 * e + 1][c] << 16);
            *(u32x4*)(d + (long long)(c0 + c) * dst_ld + r0 + ch * 8) = v;
        }
    }
}

extern "C" int vt_transpose_bf16(const void* src, long long src_ld, long long src_boff, void* dst, long long dst_ld, long long dst_boff, int rows, int cols,
                                 int nb, void* stream) {
    if (rows <= 0 || cols <= 0 || nb <= 0 || nb > 65535 || (rows % 8) || (cols % 8) || (src_ld % 8) || (dst_ld % 8) || (src_boff % 8) || (dst_boff % 8) ||
        src_ld < cols || dst_ld < rows)
        return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) return VT_ERR_BAD_ALIGN;
    const dim3 grid((cols + 63) / 64, (rows + 63) / 64, nb);
    hipLaunchKernelGGL(transpose_bf16_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, src_ld, src_boff, (bf16_t*)dst, dst_ld, dst_boff,
                       rows, cols);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}


// ------------------------------------------------------------------------------------------------
// Many transposes in ONE launch (the per-step operand packing of full fine-tuning: ~640 weights in the VideoCrafter2 UNet, ~280 in STDiT --
// one launch each was 3.5 ms of kernels plus as many launch gaps, most of them far too small to fill the chip alone).
// table: njobs rows of 8 int64 on the device: {src, dst, src_ld, dst_ld, rows, cols, first_block, tiles_x}; job j owns blocks
// [first_block_j, first_block_{j+1}), 64 x 64 tiles, row-major over (tile row, tile column).  Same tile body as transpose_bf16_kernel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_multi_bf16_kernel(const long long* __restrict__ table, int njobs) {
    __shared__ unsigned short tile[64][66];
    const long long blk = blockIdx.x;
    int lo = 0, hi = njobs - 1;                                   // last job whose first_block <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * 8 + 6] <= blk) lo = mid; else hi = mid - 1;
    }
    const long long* J = table + (size_t)lo * 8;
    const bf16_t* s = (const bf16_t*)J[0];
    bf16_t* d = (bf16_t*)J[1];
    const long long src_ld = J[2], dst_ld = J[3];
    const int rows = (int)J[4], cols = (int)J[5];
    const int local = (int)(blk - J[6]), tiles_x = (int)J[7];
    const int r0 = (local / tiles_x) * 64, c0 = (local % tiles_x) * 64;
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (t >> 3) + 32 * i, ch = t & 7;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r0 + r < rows && c0 + ch * 8 < cols) v = *(const u32x4*)(s + (long long)(r0 + r) * src_ld + c0 + ch * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) *(unsigned int*)&tile[r][ch * 8 + 2 * e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = (t >> 3) + 32 * i, ch = t & 7;
        if (c0 + c < cols && r0 + ch * 8 < rows) {
            u32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (unsigned)tile[ch * 8 + 2 * e][c] | ((unsigned)tile[ch * 8 + 2 * e + 1][c] << 16);
            *(u32x4*)(d + (long long)(c0 + c) * dst_ld + r0 + ch * 8) = v;
        }
    }
}

// table (device, int64 [njobs][8]) and total_blocks come from the caller's one-time plan (vt355.ops.TransposePlan validates every job:
// rows, cols, leading dimensions multiples of 8, 16-byte aligned pointers, first_block = running sum of tiles).
extern "C" int vt_transpose_multi_bf16(const void* table, int njobs, long long total_blocks, void* stream) {
    if (table == nullptr || njobs <= 0 || total_blocks <= 0 || total_blocks > 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    if (((uintptr_t)table) & 7) return VT_ERR_BAD_ALIGN;
    hipLaunchKernelGGL(transpose_multi_bf16_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, (const long long*)table, njobs);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
