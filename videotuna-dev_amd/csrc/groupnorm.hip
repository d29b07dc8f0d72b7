// GroupNorm (+ SiLU) over channels-last activations [N, P, C] (P = T*H*W positions), bf16 in / out, fp32 statistics.
// First kernel of the next scope rows: the block `GroupNorm(32) -> SiLU -> conv` opens every ResNet block
// of the CogVideoX 3D causal VAE encoder (the step before the DiT, cogvideo_pl.py:792-813 -> AutoencoderKLCogVideoX; SAT twin
// videotuna/models/cogvideo_sat/vae_modules/cp_enc_dec.py:436-459, 681-777) and of the VideoCrafter2 UNet
// (videotuna/models/lvdm/modules/networks/openaimodel3d.py:229-255, `normalization` = GroupNorm32 in lvdm/basics.py).
// The reference keeps NCHW / NCTHW and permutes between 2-D and 3-D views; here the layout is channels-last once and for all,
// which is also what an implicit-GEMM convolution wants for its K dimension.
//
// HBM-bound: x is read twice (statistics, apply) and y written once = 6 bytes per element.  Three launches:
//   1. per-CHANNEL sums and sums of squares of x - k_c about the pivot k_c = x[n, 0, c] (every block reads it for itself): a thread owns 8
//      consecutive channels and strides over the positions, block reduction through LDS, one fp32 atomic per channel and block into ws
//      (any channels-per-group works, e.g. 320 / 32 = 10);
//   2. fold channels into groups -> per-channel affine  y = x * a[n,c] + b[n,c]  (a = rstd*gamma, b = beta - mean*rstd*gamma);
//   3. apply (+ SiLU).
// Why the pivot: sums of x and x^2 give var = E[x^2] - mean^2, which is rounding noise in fp32 once |mean| >> std (a plateau at 100 with a
// spread of 0.05 came back with rstd off by 14 % .. 50 x).  About a sample of the channel itself the sums are of the size of the spread, and
// the pass over x stays a single one.  The group's variance is the parallel-variance fold of its channels (gn_finalize_kernel).
#include "common.h"

#define GN_THREADS 256

__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(const bf16_t* x, long long ldx, long long P, int C, float* ws,
                                                              int slabs) {
    extern __shared__ float red[];                 // [2][C]
    const int n = blockIdx.y, slab = blockIdx.x;
    const int nch = C >> 3;                        // 16-byte chunks per position
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * C; i += GN_THREADS) red[i] = 0.f;
    __syncthreads();
    const long long p0 = P * slab / slabs, p1 = P * (slab + 1) / slabs;
    for (int c0 = 0; c0 < nch; c0 += GN_THREADS) {       // more than 2048 channels (the UNet's 2560-wide skip concatenations): channel passes
        const int ncl = min(nch - c0, GN_THREADS);
        const int lanes = GN_THREADS / ncl * ncl;         // threads that take part (a whole number of positions per pass)
        if (tid < lanes) {
            const int c = c0 + tid % ncl, row = tid / ncl, rows = lanes / ncl;
            float s[8], q[8], k[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
            const bf16_t* xb = x + ((long long)n * P) * ldx + c * 8;
            const u32x4 kraw = *(const u32x4*)xb;                           // the pivots: position 0 of the sample
            unpack8(kraw, k);
            for (long long p = p0 + row; p < p1; p += 4 * rows) {          // four positions in flight per thread
                u32x4 r[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long pp = p + (long long)u * rows;
                    r[u] = kraw;                                            // past the slab: x - k = 0 adds nothing
                    if (pp < p1) r[u] = *(const u32x4*)(xb + pp * ldx);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float v[8];
                    unpack8(r[u], v);
#pragma unroll
                    for (int j = 0; j < 8; ++j) { const float d = v[j] - k[j]; s[j] += d; q[j] += d * d; }
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { atomicAdd(red + c * 8 + j, s[j]); atomicAdd(red + C + c * 8 + j, q[j]); }
        }
    }
    __syncthreads();
    float* w = ws + (size_t)n * 4 * C;
    for (int i = tid; i < 2 * C; i += GN_THREADS) atomicAdd(w + i, red[i]);
}

// one block per sample, a thread per channel: the channel sums are folded into their groups through LDS (r03: the first version gave a
// group to a thread, 2 x C/G dependent global reads each -- 13 .. 39 us per call at C = 1280, 27 ms of the UNet's step with its backward twin).
// Channel c holds s = sum (x - k_c), q = sum (x - k_c)^2 over its P positions:  mean_c = k_c + s / P,  M2_c = q - s^2 / P.  Groups by the
// parallel-variance formula, the channel means taken relative to the pivot of the group's first channel (differences of bf16 values: exact):
//   d_c = mean_c - k_g,  mean_g = k_g + avg_c d_c,  M2_g = sum_c M2_c + P sum_c (d_c - avg d)^2,  var_g = M2_g / (P C/G)
__global__ __launch_bounds__(256) void gn_finalize_kernel(float* ws, const bf16_t* x, long long ldx, const bf16_t* gamma, const bf16_t* beta,
                                                          long long P, int C, int G, float eps) {
    extern __shared__ float gsh[];                  // [4][G]: sum of d_c, then of (d_c - avg d)^2 | sum of M2_c | mean | rstd
    const int n = blockIdx.x, tid = threadIdx.x;
    float* w = ws + (size_t)n * 4 * C;
    const bf16_t* x0 = x + ((long long)n * P) * ldx;
    const int cpg = C / G;
    const float invp = 1.0f / (float)P;
    for (int g = tid; g < 2 * G; g += 256) gsh[g] = 0.f;
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float s = w[c], q = w[C + c];
        const float d = (bf2f(x0[c]) - bf2f(x0[c / cpg * cpg])) + s * invp;
        w[2 * C + c] = d;                           // the a | b planes are free until the last loop
        atomicAdd(gsh + c / cpg, d);
        atomicAdd(gsh + G + c / cpg, fmaxf(q - s * s * invp, 0.f));
    }
    __syncthreads();
    for (int g = tid; g < G; g += 256) { gsh[2 * G + g] = gsh[g] / (float)cpg; gsh[g] = 0.f; }      // avg d; the slot now sums (d_c - avg d)^2
    __syncthreads();
    for (int c = tid; c < C; c += 256) { const float e = w[2 * C + c] - gsh[2 * G + c / cpg]; atomicAdd(gsh + c / cpg, e * e); }
    __syncthreads();
    const float cnt = (float)cpg * (float)P;
    for (int g = tid; g < G; g += 256) {
        const float var = (gsh[G + g] + (float)P * gsh[g]) / cnt;
        gsh[2 * G + g] += bf2f(x0[g * cpg]);
        gsh[3 * G + g] = rsqrtf(var + eps);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float mean = gsh[2 * G + c / cpg], rstd = gsh[3 * G + c / cpg];
        const float ga = gamma ? bf2f(gamma[c]) : 1.f, be = beta ? bf2f(beta[c]) : 0.f;
        w[2 * C + c] = rstd * ga;
        w[3 * C + c] = be - mean * rstd * ga;
        w[c] = mean;              // the sums are spent: the first two planes keep the statistics for vt_groupnorm_silu_bwd_cl
        w[C + c] = rstd;
    }
}

template <bool SILU>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(const bf16_t* x, long long ldx, bf16_t* y, long long ldy, long long P, int C,
                                                              const float* ws) {
    const int n = blockIdx.y;
    const int nch = C >> 3;
    const float* a = ws + (size_t)n * 4 * C + 2 * C;
    const float* b = a + C;
    const long long total = P * nch;
    for (long long i = (long long)blockIdx.x * GN_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * GN_THREADS) {
        const long long p = i / nch;
        const int c = (int)(i - p * nch) * 8;
        float v[8];
        unpack8(*(const u32x4*)(x + ((long long)n * P + p) * ldx + c), v);
        const f32x4 a0 = *(const f32x4*)(a + c), a1 = *(const f32x4*)(a + c + 4), b0 = *(const f32x4*)(b + c), b1 = *(const f32x4*)(b + c + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = v[j] * a0[j] + b0[j]; v[j + 4] = v[j + 4] * a1[j] + b1[j]; }
        if (SILU) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * (1.0f - __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v[j] * 1.4426950408889634f) + 1.0f));
        }
        *(u32x4*)(y + ((long long)n * P + p) * ldy + c) = pack8(v);
    }
}

// position slabs per sample of the statistics passes: about 1.5 blocks per CU over all samples (every block ends in 2 C fp32 atomics on the
// sample's sums -- more blocks pile up on the same addresses, fewer leave CUs idle: the first version's P / 256 slabs were 8 blocks at the
// UNet's innermost level, 100 .. 200 us for 6.5 MB), at least 4 positions per thread row
static int gn_slabs(int N, long long P, int C) {
    const int nch = C >> 3;
    const int rows = nch >= 256 ? 1 : 256 / nch;
    long long want = (384 + N - 1) / N;
    const long long cap = P / (4LL * rows);
    if (want > cap) want = cap;
    return (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
}

extern "C" long long vt_groupnorm_ws_bytes(int N, int C) { return (long long)N * 4 * C * 4; }

// x, y: [N, P, C] bf16 with position stride ldx / ldy (>= C, multiples of 8); gamma / beta: bf16 [C] or null; ws: fp32 scratch of
// vt_groupnorm_ws_bytes(N, C) bytes (contents don't matter).  silu != 0 applies x*sigmoid(x) to the normalised value.
extern "C" int vt_groupnorm_silu_cl(const void* x, long long ldx, const void* gamma, const void* beta, void* y, long long ldy,
                                    int N, long long P, int C, int G, float eps, int silu, float* ws, long long ws_bytes, void* stream) {
    if (N <= 0 || P <= 0 || C <= 0 || G <= 0 || (C % G) || (C % 8) || C > 8192 || (ldx % 8) || (ldy % 8) || ldx < C || ldy < C)
        return VT_ERR_BAD_SHAPE;
    if (N > 65535 || ws == nullptr || ws_bytes < vt_groupnorm_ws_bytes(N, C)) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)ws)) & 15) return VT_ERR_BAD_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)N * 4 * C * 4, st) != hipSuccess) return VT_ERR_LAUNCH;
    const int slabs = gn_slabs(N, P, C);
    hipLaunchKernelGGL(gn_stats_kernel, dim3(slabs, N), dim3(GN_THREADS), 2 * C * sizeof(float), st, (const bf16_t*)x, ldx, P, C, ws, slabs);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(N), dim3(256), 4 * G * sizeof(float), st, ws, (const bf16_t*)x, ldx, (const bf16_t*)gamma, (const bf16_t*)beta, P, C, G, eps);
    const long long total = P * (C >> 3);
    long long blocks = (total + GN_THREADS - 1) / GN_THREADS;
    if (blocks > 8192) blocks = 8192;
    if (silu) hipLaunchKernelGGL(gn_apply_kernel<true>, dim3((unsigned)blocks, N), dim3(GN_THREADS), 0, st, (const bf16_t*)x, ldx, (bf16_t*)y, ldy, P, C, ws);
    else hipLaunchKernelGGL(gn_apply_kernel<false>, dim3((unsigned)blocks, N), dim3(GN_THREADS), 0, st, (const bf16_t*)x, ldx, (bf16_t*)y, ldy, P, C, ws);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------------
// SpatialNorm3D (+ SiLU) of the CogVideoX VAE decoder (cp_enc_dec.py:462-539):  y = silu?( GroupNorm(x) * conv_y(zq^) + conv_b(zq^) ),
// zq^ = the latent nearest-interpolated to x's size with the first frame handled apart.  conv_y / conv_b are 1x1x1, so they commute with
// the interpolation: the host computes them ONCE at latent resolution (one GEMM) into mod [N, Tz, Hz, Wz, 2C] = (Y | B) and this apply
// pass gathers from that table (L2-resident: 13x60x90 positions x 2C) -- no upsampled zq is ever stored.  Index rule (ratios are powers of
// two, the host checks): hz = h >> sh, wz = w >> sw;  T > 1: tz = 0 for t = 0, else 1 + ((t-1) >> st);  T == 1: tz = 0.
// Statistics: the two passes above, unchanged.  Positions of one sample are indexed in 32 bits (the host bounds P * C/8 < 2^31), every
// element offset is 64-bit: x / y may lie past 2 / 4 GiB.
template <bool SILU>
__global__ __launch_bounds__(GN_THREADS) void spn_apply_kernel(const bf16_t* x, long long ldx, bf16_t* y, long long ldy, const bf16_t* mod,
                                                               int T, int H, int W, int C, int Tz, int Hz, int Wz, int st, int sh, int sw,
                                                               const float* ws) {
    const int n = blockIdx.y;
    const unsigned nch = C >> 3, HW = (unsigned)H * W;
    const float* a = ws + (size_t)n * 4 * C + 2 * C;
    const float* b = a + C;
    const unsigned total = (unsigned)T * HW * nch;
    const long long xbase = (long long)n * T * HW;
    const long long zbase = (long long)n * Tz * Hz * Wz;
    for (unsigned i = blockIdx.x * GN_THREADS + threadIdx.x; i < total; i += gridDim.x * GN_THREADS) {
        const unsigned p = i / nch;
        const int c = (int)(i - p * nch) * 8;
        const unsigned t = p / HW, r = p - t * HW;
        const unsigned h = r / (unsigned)W, w = r - h * (unsigned)W;
        const int tz = (T > 1 && t > 0) ? 1 + (int)((t - 1) >> st) : 0;
        const long long zrow = zbase + ((long long)tz * Hz + (h >> sh)) * Wz + (w >> sw);
        float v[8], my[8], mb[8];
        unpack8(*(const u32x4*)(x + (xbase + p) * ldx + c), v);
        unpack8(*(const u32x4*)(mod + zrow * (2LL * C) + c), my);
        unpack8(*(const u32x4*)(mod + zrow * (2LL * C) + C + c), mb);
        const f32x4 a0 = *(const f32x4*)(a + c), a1 = *(const f32x4*)(a + c + 4), b0 = *(const f32x4*)(b + c), b1 = *(const f32x4*)(b + c + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = (v[j] * a0[j] + b0[j]) * my[j] + mb[j];
            v[j + 4] = (v[j + 4] * a1[j] + b1[j]) * my[j + 4] + mb[j + 4];
        }
        if (SILU) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * (1.0f - __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v[j] * 1.4426950408889634f) + 1.0f));
        }
        *(u32x4*)(y + (xbase + p) * ldy + c) = pack8(v);
    }
}

static int pow2_shift(int big, int small) {          // log2(big / small) when that ratio is a power of two, else -1
    if (small <= 0 || big % small) return -1;
    const int r = big / small;
    if (r & (r - 1)) return -1;
    int s = 0;
    while ((1 << s) < r) ++s;
    return s;
}

// x, y: bf16 [N, T, H, W, C] channels-last with position stride ldx / ldy; gamma / beta: bf16 [C] or null; mod: bf16 [N, Tz, Hz, Wz, 2C]
// contiguous (conv_y(zq) | conv_b(zq) at latent resolution); ws as for vt_groupnorm_silu_cl.  H / Hz, W / Wz and (T-1) / (Tz-1) must be
// powers of two (T > 1 needs Tz > 1; T == 1 reads latent frame 0).
extern "C" int vt_spatialnorm_silu_cl(const void* x, long long ldx, const void* gamma, const void* beta, const void* mod, void* y,
                                      long long ldy, int N, int T, int H, int W, int C, int Tz, int Hz, int Wz, int G, float eps, int silu,
                                      float* ws, long long ws_bytes, void* stream) {
    if (N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || G <= 0 || (C % G) || (C % 8) || C > 8192 || (ldx % 8) || (ldy % 8) || ldx < C || ldy < C)
        return VT_ERR_BAD_SHAPE;
    if (N > 65535 || mod == nullptr || ws == nullptr || ws_bytes < vt_groupnorm_ws_bytes(N, C)) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)ws) | ((uintptr_t)mod)) & 15) return VT_ERR_BAD_ALIGN;
    const int sh = pow2_shift(H, Hz), sw = pow2_shift(W, Wz);
    int st = 0;
    if (T > 1) {
        if (Tz < 2) return VT_ERR_BAD_SHAPE;
        st = pow2_shift(T - 1, Tz - 1);
    } else if (Tz < 1) return VT_ERR_BAD_SHAPE;
    if (sh < 0 || sw < 0 || st < 0) return VT_ERR_BAD_SHAPE;
    const long long P = (long long)T * H * W;
    if (P * (C >> 3) >= 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)N * 4 * C * 4, s) != hipSuccess) return VT_ERR_LAUNCH;
    const int slabs = gn_slabs(N, P, C);
    hipLaunchKernelGGL(gn_stats_kernel, dim3(slabs, N), dim3(GN_THREADS), 2 * C * sizeof(float), s, (const bf16_t*)x, ldx, P, C, ws, slabs);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(N), dim3(256), 4 * G * sizeof(float), s, ws, (const bf16_t*)x, ldx, (const bf16_t*)gamma, (const bf16_t*)beta, P, C, G, eps);
    long long blocks = (P * (C >> 3) + GN_THREADS - 1) / GN_THREADS;
    if (blocks > 8192) blocks = 8192;
    if (silu) hipLaunchKernelGGL(spn_apply_kernel<true>, dim3((unsigned)blocks, N), dim3(GN_THREADS), 0, s, (const bf16_t*)x, ldx, (bf16_t*)y, ldy,
                                 (const bf16_t*)mod, T, H, W, C, Tz, Hz, Wz, st, sh, sw, ws);
    else hipLaunchKernelGGL(spn_apply_kernel<false>, dim3((unsigned)blocks, N), dim3(GN_THREADS), 0, s, (const bf16_t*)x, ldx, (bf16_t*)y, ldy,
                            (const bf16_t*)mod, T, H, W, C, Tz, Hz, Wz, st, sh, sw, ws);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Temporal compression of the VAE's DownSample3D (compress_time, cp_enc_dec.py:640-657): the first frame is kept, the remaining
// T - 1 frames are averaged in consecutive pairs (avg_pool1d(kernel 2, stride 2): a trailing odd frame is dropped).
//   y[n, 0] = x[n, 0];   y[n, 1 + i] = (x[n, 1 + 2i] + x[n, 2 + 2i]) / 2,   To = 1 + (T - 1) / 2      (T == 1: copy)
// keep_first == 0: plain avg_pool1d(2, 2) over ALL frames, y[n, i] = (x[n, 2i] + x[n, 2i+1]) / 2, To = T / 2 -- the branch the same module
// takes on context-parallel ranks > 0 / fake_cp=False (cp_enc_dec.py:659-667) and diffusers' CogVideoXDownsample3D takes for an EVEN
// frame count (the 8-frame chunks after the first 9 of its chunked encode).
// x: bf16 [N, T, HW, C], y: bf16 [N, To, HW, C] channels-last.
__global__ __launch_bounds__(256) void temporal_pool_kernel(const bf16_t* x, long long ldx, bf16_t* y, long long ldy, int T, int To,
                                                            long long HW, int C, long long total, int keep_first) {
    const int nch = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % nch) * 8;
        const long long pos = i / nch;               // (n, to, hw)
        const long long hw = pos % HW;
        const long long nto = pos / HW;
        const int to = (int)(nto % To);
        const long long n = nto / To;
        const bf16_t* xs = x + ((n * T) * HW + hw) * ldx + c;
        float a[8];
        if (to == 0 && keep_first) {
            unpack8(*(const u32x4*)xs, a);
        } else {
            float b[8];
            unpack8(*(const u32x4*)(xs + (long long)(2 * to - keep_first) * HW * ldx), a);
            unpack8(*(const u32x4*)(xs + (long long)(2 * to + 1 - keep_first) * HW * ldx), b);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = 0.5f * (a[j] + b[j]);
        }
        *(u32x4*)(y + pos * ldy + c) = pack8(a);
    }
}

extern "C" int vt_temporal_pool_cl(const void* x, long long ldx, void* y, long long ldy, int N, int T, long long HW, int C, int keep_first,
                                   void* stream) {
    keep_first = keep_first ? 1 : 0;
    if (!keep_first && T < 2) return VT_ERR_BAD_SHAPE;
    if (N <= 0 || T <= 0 || HW <= 0 || C <= 0 || (C % 8) || (ldx % 8) || (ldy % 8) || ldx < C || ldy < C) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)x) | ((uintptr_t)y)) & 15) return VT_ERR_BAD_ALIGN;
    const int To = keep_first ? 1 + (T - 1) / 2 : T / 2;
    const long long total = (long long)N * To * HW * (C >> 3);
    long long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(temporal_pool_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (bf16_t*)y, ldy,
                       T, To, HW, C, total, keep_first);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
