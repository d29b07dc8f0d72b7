// MX-scaled FP8 (OCP E4M3) GEMM on the gfx950 matrix cores, and the kernels that feed it with delayed per-tensor scaling:
//   C[M,N] = epilogue( (Aq[M,K] Wq[N,K]^T) * scale_a * scale_w  [+ At[M,Kt] Wt[N,Kt]^T in bf16]  + bias )
// The product runs on v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands and every E8M0 block scale fixed at 127 (= 2^0), i.e. a plain
// per-tensor fp8 product at twice the bf16 MFMA rate (the non-scaled v_mfma_f32_16x16x32_fp8_fp8 of gemm_fp8.hip runs at the bf16 rate).
// scale_a / scale_w are device scalars (no host sync).  The optional bf16 tail is the K-extension of an adapted (LoRA) Linear: its
// [x A3^T | scaling B] columns stay bf16 and go through v_mfma_f32_16x16x32_bf16 into the same accumulators after the scaled fp8 part
// (the C/D layout of both instructions is the same on gfx950).  The optional fp8 copy of the output, Cq = e4m3(C_bf16 / scale_out) with
// max |C_bf16| into an amax slot, hands the next Linear its quantised input without another pass.
// vt_gemm_mxfp8_dx is the same kernel for the input-gradient products dX = g W of the backward: the quantised gradient (second MFMA
// operand slot, format code in blgp) is E5M2 or E4M3, the weight (first slot, cbsz) the byte-transposed E4M3 copy; epilogues plain,
// EPI_DGELU (saved pre-activation u) and "+ residual" (EPI_GATED_RES without gates); the fp8 copy of the output in either format.
//
// Kernel: the 128x128 tile / LDS-DMA staging / XOR-swizzled 128-byte rows of gemm_fp8.hip.  A K-tile is 128 bytes per row = ONE 128-deep
// MFMA k-step; lane group q = lane >> 4 takes the 32 bytes [32 q, 32 q + 32) of its row (chunks 2 q, 2 q + 1) for both operands, so
// whichever k order the instruction assigns to those bytes, A and B agree on it.  K % 128 == 0, N % 4 == 0.
#include "gemm_epilogue.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;

struct GemmMxParams {
    GemmParams g;                                   // C, bias, epilogue operands, M, N, K, ldc (A / W / lda / ldw unused)
    const unsigned char* A; const unsigned char* W; int lda, ldw;
    const float* scale_a; const float* scale_w;
    const bf16_t* At; const bf16_t* Wt; int ldat, ldwt, Kt;     // bf16 tail (Kt = 0: none)
    unsigned char* Cq; int ldcq; const float* scale_out; unsigned int* amax;   // fp8 copy of the output (Cq = null: none)
};

enum { MX_MAX_KT = 384 };                          // widest bf16 tail: three rank-128 adapters (vt355.lora.extension_layout)
enum { FMT_E4M3 = 0, FMT_E5M2 = 1 };               // the f8f6f4 format codes of v_mfma_scale (cbsz / blgp), OCP formats on gfx950

__device__ __forceinline__ unsigned int e4m3x4(const float* v, float sc) {
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = fminf(fmaxf(__fdiv_rn(v[j], sc), -448.0f), 448.0f);     // satfinite(RNE(x / scale))
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], r, true);
    return (unsigned int)r;
}

__device__ __forceinline__ unsigned int e5m2x4(const float* v, float sc) {
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = fminf(fmaxf(__fdiv_rn(v[j], sc), -57344.0f), 57344.0f);  // satfinite(RNE(x / scale))
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_bf8_f32(t[0], t[1], r, false);
    r = __builtin_amdgcn_cvt_pk_bf8_f32(t[2], t[3], r, true);
    return (unsigned int)r;
}

// one publisher per workgroup of 256 threads: wave maxima through LDS
__device__ __forceinline__ void amax_publish_block(unsigned int* slot, float mx) {
    __shared__ float red[4];
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) amax_publish(slot, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

template <int FMT>
__device__ __forceinline__ unsigned int fp8x4(const float* v, float sc) {
    return FMT == FMT_E5M2 ? e5m2x4(v, sc) : e4m3x4(v, sc);
}

// FA: format of the A operand (activation: E4M3; output gradient: either), FO: format of the fp8 copy of the output.  W is always E4M3.
// WT: the wide bf16 tail (64 < Kt <= 384).  A 64-column step of the tail is 128 bytes per row, the geometry of an fp8 K-tile, so the
// tail's [128, 64] A and W slabs go through the same two LDS stages with the same DMA pattern and swizzle: they are K-tiles nk, nk + 1, ...
// of the one pipeline (the first one is requested during the last fp8 tile), each read back as two 32-deep bf16 k-steps.
template <int EPI, int FA = FMT_E4M3, int FO = FMT_E4M3, bool WT = false>
__global__ __launch_bounds__(256, 2) void gemm_mxfp8_kernel(GemmMxParams p) {
    __shared__ __attribute__((aligned(16))) char smem[65536];
    const GemmParams& g = p.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int nbm = (g.M + 127) / 128, nbn = (g.N + 127) / 128;
    const int id = xcd_remap(blockIdx.x, nbm * nbn);
    const int GM = 8;
    const int in_group = GM * nbn;
    const int group = id / in_group;
    const int first_m = group * GM;
    const int gsz = min(nbm - first_m, GM);
    const int tile_m = first_m + (id % in_group) % gsz;
    const int tile_n = (id % in_group) / gsz;
    const int row0 = tile_m * 128, col0 = tile_n * 128;
    const long long a_rem = (long long)(g.M - row0) * p.lda, w_rem = (long long)(g.N - col0) * p.ldw;
    __amdgpu_buffer_rsrc_t ra = make_rsrc(p.A + (size_t)row0 * p.lda, (unsigned)(a_rem > 0x7fffffffLL ? 0x7fffffffLL : a_rem));
    __amdgpu_buffer_rsrc_t rw = make_rsrc(p.W + (size_t)col0 * p.ldw, (unsigned)(w_rem > 0x7fffffffLL ? 0x7fffffffLL : w_rem));
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int drl = lane >> 3, dcp = lane & 7;
    int a_voff[4], w_voff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 8 * (wv + 4 * j) + drl;
        a_voff[j] = row * p.lda + ((dcp ^ drl) << 4);
        w_voff[j] = row * p.ldw + ((dcp ^ drl) << 4);
    }
    auto dma = [&](int kt, int buf) {
        const int soff = kt * 128;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            char* dst = smem + buf * 32768 + (wv + 4 * j) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)dst, 16, a_voff[j], soff, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(dst + 16384), 16, w_voff[j], soff, 0, 0);
        }
    };
    // WT: the tail slabs.  The resource ends with the Kt columns of the last valid row: rows past M / N and the columns past Kt of that
    // row come back as zeros, the columns past Kt of every other row are bytes of the wider buffer that no MFMA reads (Kt % 64 == 32).
    const int nts = WT ? (p.Kt + 63) / 64 : 0;
    auto dma_tail = [&](int s, int buf) {
        const long long at_rem = ((long long)(g.M - row0 - 1) * p.ldat + p.Kt) * 2, wt_rem = ((long long)(g.N - col0 - 1) * p.ldwt + p.Kt) * 2;
        __amdgpu_buffer_rsrc_t rat = make_rsrc(p.At + (size_t)row0 * p.ldat, (unsigned)(at_rem > 0x7fffffffLL ? 0x7fffffffLL : at_rem));
        __amdgpu_buffer_rsrc_t rwt = make_rsrc(p.Wt + (size_t)col0 * p.ldwt, (unsigned)(wt_rem > 0x7fffffffLL ? 0x7fffffffLL : wt_rem));
        const int soff = s * 128;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 8 * (wv + 4 * j) + drl;
            char* dst = smem + buf * 32768 + (wv + 4 * j) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rat, (__attribute__((address_space(3))) void*)dst, 16,
                                                     row * p.ldat * 2 + ((dcp ^ drl) << 4), soff, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rwt, (__attribute__((address_space(3))) void*)(dst + 16384), 16,
                                                     row * p.ldwt * 2 + ((dcp ^ drl) << 4), soff, 0, 0);
        }
    };
    f32x4 acc[4][4];   // [tn][tm]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nk = g.K / 128;
    dma(0, 0);
    __syncthreads();
    const int frow = lane & 15, fq = lane >> 4, fx = lane & 7;
    const int c0 = ((2 * fq) ^ fx) << 4, c1 = ((2 * fq + 1) ^ fx) << 4;        // swizzled offsets of this lane group's two 16-byte chunks
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) dma(kt + 1, buf ^ 1);
        else if (WT) dma_tail(0, buf ^ 1);
        const char* As = smem + buf * 32768;
        const char* Ws = As + 16384;
        i32x8 af[4], wf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const char* pa = As + (wm * 64 + t * 16 + frow) * 128;
            const char* pw = Ws + (wn * 64 + t * 16 + frow) * 128;
            const i32x4 a0 = *(const i32x4*)(pa + c0), a1 = *(const i32x4*)(pa + c1);
            const i32x4 w0 = *(const i32x4*)(pw + c0), w1 = *(const i32x4*)(pw + c1);
            af[t] = (i32x8){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            wf[t] = (i32x8){w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
        }
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)      // first slot (cbsz): the e4m3 weight; second slot (blgp): A in format FA; unit block scales (E8M0 127)
                acc[tn][tm] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[tn], af[tm], acc[tn][tm], FMT_E4M3, FA, 0, 127, 0, 127);
        __syncthreads();
    }
    const float sc = p.scale_a[0] * p.scale_w[0];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn)
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) acc[tn][tm] *= sc;
    if (WT) {
        // wide bf16 tail from LDS: step s (64 columns) sits in stage (nk + s) & 1; lane l holds row l & 15, k = 8 (l >> 4) .. + 7 of each of
        // its two 32-deep k-steps, i.e. the 16-byte chunks (l >> 4) and 4 + (l >> 4) of its 128-byte row.  The next step's slabs are in
        // flight while this step's MFMAs run.
        const int t0 = ((fq ^ fx) << 4), t1 = (((4 + fq) ^ fx) << 4);
        for (int s = 0; s < nts; ++s) {
            const int buf = (nk + s) & 1;
            if (s + 1 < nts) dma_tail(s + 1, buf ^ 1);
            const char* As = smem + buf * 32768;
            const char* Ws = As + 16384;
            const bool two = 64 * s + 32 < p.Kt;
            bf16x8 a8[4], w8[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a8[t] = *(const bf16x8*)(As + (wm * 64 + t * 16 + frow) * 128 + t0);
                w8[t] = *(const bf16x8*)(Ws + (wn * 64 + t * 16 + frow) * 128 + t0);
            }
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w8[tn], a8[tm], acc[tn][tm], 0, 0, 0);
            if (two) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    a8[t] = *(const bf16x8*)(As + (wm * 64 + t * 16 + frow) * 128 + t1);
                    w8[t] = *(const bf16x8*)(Ws + (wn * 64 + t * 16 + frow) * 128 + t1);
                }
#pragma unroll
                for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                    for (int tm = 0; tm < 4; ++tm) acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w8[tn], a8[tm], acc[tn][tm], 0, 0, 0);
            }
            __syncthreads();
        }
    } else if (p.Kt > 0) {
        // bf16 tail, straight from global memory (Kt <= 64 columns): lane l holds row l & 15, k = 8 (l >> 4) .. + 7 of a 32-deep k-step.
        // Rows past M / N read the last row (their results are never stored).
        const bf16_t* at[4]; const bf16_t* wt[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            at[t] = p.At + (size_t)min(row0 + wm * 64 + t * 16 + frow, g.M - 1) * p.ldat + fq * 8;
            wt[t] = p.Wt + (size_t)min(col0 + wn * 64 + t * 16 + frow, g.N - 1) * p.ldwt + fq * 8;
        }
        for (int k = 0; k < p.Kt; k += 32) {
            bf16x8 a8[4], w8[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { a8[t] = *(const bf16x8*)(at[t] + k); w8[t] = *(const bf16x8*)(wt[t] + k); }
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w8[tn], a8[tm], acc[tn][tm], 0, 0, 0);
        }
    }
    float* Cs = (float*)smem;
    const int er = tid >> 5, ec = (tid & 31) * 4;
    const int n = col0 + ec;
    // EPI_DGELU: this thread's 16 x 4 saved pre-activations are fetched now, ahead of the LDS transposes, instead of one dependent 8-byte
    // load per row pass (the epilogue of the N 12288 product was latency-bound on them)
    constexpr bool PRE = EPI == EPI_DGELU;
    constexpr int UNR = PRE ? 8 : 2;
    u32x2 auxp[2][8];
    if (PRE) {
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int pass = 0; pass < 8; ++pass) {
                const int m = row0 + half * 64 + pass * 8 + er;
                auxp[half][pass] = (m < g.M && n < g.N) ? gemm_epilogue_aux_load<EPI>(g, m, n) : (u32x2){0u, 0u};
            }
    }
    float bias4[4] = {0.f, 0.f, 0.f, 0.f};
    if (g.bias != nullptr && n < g.N) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bias4[j] = bf2f(g.bias[n + j]);
    }
    const GateCtx gc = gate_ctx_load(g, row0, 128, n);
    const float qsc = p.Cq != nullptr ? p.scale_out[0] : 1.0f;
    float amax = 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (wm == half) {
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm)
                    *(f32x4*)(Cs + (tm * 16 + frow) * 132 + wn * 64 + tn * 16 + fq * 4) = acc[tn][tm];
        }
        __syncthreads();
#pragma unroll UNR
        for (int pass = 0; pass < 8; ++pass) {
            const int ml = pass * 8 + er;
            const int m = row0 + half * 64 + ml;
            if (m < g.M && n < g.N) {
                const f32x4 v = *(const f32x4*)(Cs + ml * 132 + ec);
                const f32x4 o = gemm_epilogue_apply<EPI>(g, m, n, v, bias4, PRE ? auxp[half][pass] : gemm_epilogue_aux_load<EPI>(g, m, n), &gc);
                u32x2 c2;
                c2[0] = pack2(o[0], o[1]);
                c2[1] = pack2(o[2], o[3]);
                *(u32x2*)((bf16_t*)g.C + (size_t)m * g.ldc + n) = c2;
                if (p.Cq != nullptr) {
                    const float b[4] = {__uint_as_float(c2[0] << 16), __uint_as_float(c2[0] & 0xffff0000u),
                                        __uint_as_float(c2[1] << 16), __uint_as_float(c2[1] & 0xffff0000u)};     // the bf16 values as written
#pragma unroll
                    for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fabsf(b[j]));
                    *(unsigned int*)(p.Cq + (size_t)m * p.ldcq + n) = fp8x4<FO>(b, qsc);
                }
            }
        }
        __syncthreads();
    }
    if (p.Cq != nullptr) {                       // amax: wave maximum, then one atomic per workgroup (non-negative floats order as their bits)
        amax = wave_max(amax);
        float* red = (float*)smem;
        if (lane == 0) red[wave] = amax;
        __syncthreads();
        if (tid == 0) amax_publish(p.amax, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
    }
}

// Kt <= 64: the instantiation every call ran before the wide tail existed; above: the LDS-staged tail
template <int EPI, int FA, int FO>
static void launch_mxfp8(const GemmMxParams& p, int tiles, hipStream_t st) {
    if (p.Kt > 64) hipLaunchKernelGGL((gemm_mxfp8_kernel<EPI, FA, FO, true>), dim3(tiles), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_mxfp8_kernel<EPI, FA, FO>), dim3(tiles), dim3(256), 0, st, p);
}

// A, W: float8_e4m3fn [M, lda] / [N, ldw] (bytes; multiples of 16); scale_a, scale_w: device fp32 scalars; epilogue / bias / residual /
// gates / pre_act_out as vt_gemm_bf16 (EPI_BIAS, EPI_BIAS_GELU, EPI_GATED_RES); C bf16 [M, ldc].  At / Wt: bf16 tail [M, ldat] / [N, ldwt]
// of Kt columns (Kt = 0: none; else a multiple of 32, <= 384; ldat / ldwt may exceed Kt: column slices of wider buffers; up to 64 the
// kernel reads them straight from global memory, above that it stages them through LDS).  Cq: e4m3 copy of C [M, ldcq] (null: none) with scale_out (device fp32)
// and max |C| into amax (device uint32 holding float bits; accumulated, not cleared).  K % 128 == 0, N % 4 == 0.
extern "C" int vt_gemm_mxfp8(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* bias,
                             const float* scale_a, const float* scale_w, int epilogue, const void* residual, int ldr,
                             const float* gate_txt, const float* gate_vid, int gate_bstride, int S, int St, void* pre_act_out, int ldc2,
                             const void* At, int ldat, const void* Wt, int ldwt, int Kt, void* Cq, int ldcq, const float* scale_out,
                             unsigned int* amax, void* stream) {
    if (M <= 0 || N <= 0 || K <= 0 || (K % 128) || (N % 4) || (lda % 16) || (ldw % 16) || (ldc % 4) || lda < K || ldw < K || ldc < N) return VT_ERR_BAD_SHAPE;
    if (scale_a == nullptr || scale_w == nullptr) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)A) | ((uintptr_t)W)) & 15 || (((uintptr_t)C) & 7)) return VT_ERR_BAD_ALIGN;
    if (epilogue != EPI_BIAS && epilogue != EPI_BIAS_GELU && epilogue != EPI_GATED_RES) return VT_ERR_UNSUPPORTED;
    if (epilogue == EPI_BIAS_GELU && (pre_act_out == nullptr || ldc2 < N || (ldc2 % 4))) return VT_ERR_BAD_SHAPE;
    if (epilogue == EPI_GATED_RES && (residual == nullptr || ldr < N || (ldr % 4))) return VT_ERR_BAD_SHAPE;
    if (epilogue == EPI_GATED_RES && pre_act_out != nullptr && (ldc2 < N || (ldc2 % 4))) return VT_ERR_BAD_SHAPE;
    if (gate_vid != nullptr && (gate_txt == nullptr || S <= 0 || (gate_bstride % 4) || (((uintptr_t)gate_txt | (uintptr_t)gate_vid) & 15)))
        return VT_ERR_BAD_SHAPE;
    if (Kt < 0 || Kt > MX_MAX_KT || (Kt % 32)) return VT_ERR_BAD_SHAPE;
    if (Kt > 0 && (At == nullptr || Wt == nullptr || ldat < Kt || ldwt < Kt || (ldat % 8) || (ldwt % 8))) return VT_ERR_BAD_SHAPE;
    if (Kt > 0 && ((((uintptr_t)At) | ((uintptr_t)Wt)) & 15)) return VT_ERR_BAD_ALIGN;
    if (Cq != nullptr && (scale_out == nullptr || amax == nullptr || ldcq < N || (ldcq % 4))) return VT_ERR_BAD_SHAPE;
    if (Cq != nullptr && (((uintptr_t)Cq) & 3)) return VT_ERR_BAD_ALIGN;
    GemmMxParams p{};
    p.g.C = C; p.g.bias = (const bf16_t*)bias; p.g.R = (const bf16_t*)residual; p.g.gate_txt = gate_txt; p.g.gate_vid = gate_vid;
    p.g.C2 = (bf16_t*)pre_act_out; p.g.M = M; p.g.N = N; p.g.K = K; p.g.ldc = ldc; p.g.ldr = ldr; p.g.ldc2 = ldc2;
    p.g.S = S > 0 ? S : 1; p.g.St = St; p.g.gate_bstride = gate_bstride; p.g.r_mod = 0; p.g.splits = 1;
    p.A = (const unsigned char*)A; p.W = (const unsigned char*)W; p.lda = lda; p.ldw = ldw; p.scale_a = scale_a; p.scale_w = scale_w;
    p.At = (const bf16_t*)At; p.Wt = (const bf16_t*)Wt; p.ldat = ldat; p.ldwt = ldwt; p.Kt = Kt;
    p.Cq = (unsigned char*)Cq; p.ldcq = ldcq; p.scale_out = scale_out; p.amax = amax;
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
    hipStream_t st = (hipStream_t)stream;
    if (epilogue == EPI_BIAS) launch_mxfp8<EPI_BIAS, FMT_E4M3, FMT_E4M3>(p, tiles, st);
    else if (epilogue == EPI_BIAS_GELU) launch_mxfp8<EPI_BIAS_GELU, FMT_E4M3, FMT_E4M3>(p, tiles, st);
    else launch_mxfp8<EPI_GATED_RES, FMT_E4M3, FMT_E4M3>(p, tiles, st);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// The input-gradient product of a Linear whose forward ran on vt_gemm_mxfp8: C[M, N] = epilogue((Gq[M, K] WqT[N, K]^T) scale_g scale_w
// [+ At Wt^T]).  Gq: the quantised output gradient, fmt_g 0 = e4m3 / 1 = e5m2; WqT: e4m3 bytes of the transposed weight (a column or row
// slice of it: ldw = its full row length).  epilogue: EPI_BIAS (plain store, there is no bias), EPI_DGELU (times gelu'(pre_act_in)),
// EPI_GATED_RES (+ residual, no gates).  At / Wt: the bf16 tail as vt_gemm_mxfp8 (LoRA: dt [M, ext], A3^T [N, ext]).  Cq: fp8 copy of C in format fmt_out
// (EPI_DGELU only: d(u) for the fc1 / linear1 product that follows) with scale_out and amax as vt_gemm_mxfp8.  K % 128 == 0, N % 4 == 0.
extern "C" int vt_gemm_mxfp8_dx(const void* G, int ldg, int fmt_g, const void* WT, int ldw, void* C, int ldc, int M, int N, int K,
                                const float* scale_g, const float* scale_w, int epilogue, const void* residual, int ldr,
                                const void* pre_act_in, int ldu, const void* At, int ldat, const void* Wt, int ldwt, int Kt,
                                void* Cq, int ldcq, int fmt_out, const float* scale_out, unsigned int* amax, void* stream) {
    if (M <= 0 || N <= 0 || K <= 0 || (K % 128) || (N % 4) || (ldg % 16) || (ldw % 16) || (ldc % 4) || ldg < K || ldw < K || ldc < N) return VT_ERR_BAD_SHAPE;
    if (scale_g == nullptr || scale_w == nullptr) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)G) | ((uintptr_t)WT)) & 15 || (((uintptr_t)C) & 7)) return VT_ERR_BAD_ALIGN;
    if ((fmt_g != FMT_E4M3 && fmt_g != FMT_E5M2) || (fmt_out != FMT_E4M3 && fmt_out != FMT_E5M2)) return VT_ERR_UNSUPPORTED;
    if (epilogue != EPI_BIAS && epilogue != EPI_DGELU && epilogue != EPI_GATED_RES) return VT_ERR_UNSUPPORTED;
    if (epilogue == EPI_DGELU && (pre_act_in == nullptr || ldu < N || (ldu % 4) || (((uintptr_t)pre_act_in) & 7))) return VT_ERR_BAD_SHAPE;
    if (epilogue == EPI_GATED_RES && (residual == nullptr || ldr < N || (ldr % 4) || (((uintptr_t)residual) & 7))) return VT_ERR_BAD_SHAPE;
    if (Kt < 0 || Kt > MX_MAX_KT || (Kt % 32)) return VT_ERR_BAD_SHAPE;
    if (Kt > 0 && (At == nullptr || Wt == nullptr || ldat < Kt || ldwt < Kt || (ldat % 8) || (ldwt % 8))) return VT_ERR_BAD_SHAPE;
    if (Kt > 0 && ((((uintptr_t)At) | ((uintptr_t)Wt)) & 15)) return VT_ERR_BAD_ALIGN;
    if (Cq != nullptr && epilogue != EPI_DGELU) return VT_ERR_UNSUPPORTED;
    if (Cq != nullptr && (scale_out == nullptr || amax == nullptr || ldcq < N || (ldcq % 4))) return VT_ERR_BAD_SHAPE;
    if (Cq != nullptr && (((uintptr_t)Cq) & 3)) return VT_ERR_BAD_ALIGN;
    GemmMxParams p{};
    p.g.C = C; p.g.R = (const bf16_t*)residual; p.g.U = (const bf16_t*)pre_act_in; p.g.M = M; p.g.N = N; p.g.K = K; p.g.ldc = ldc;
    p.g.ldr = ldr; p.g.ldu = ldu; p.g.S = 1; p.g.r_mod = 0; p.g.splits = 1;
    p.A = (const unsigned char*)G; p.W = (const unsigned char*)WT; p.lda = ldg; p.ldw = ldw; p.scale_a = scale_g; p.scale_w = scale_w;
    p.At = (const bf16_t*)At; p.Wt = (const bf16_t*)Wt; p.ldat = ldat; p.ldwt = ldwt; p.Kt = Kt;
    p.Cq = (unsigned char*)Cq; p.ldcq = ldcq; p.scale_out = scale_out; p.amax = amax;
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
    hipStream_t st = (hipStream_t)stream;
    const bool g5 = fmt_g == FMT_E5M2, o5 = fmt_out == FMT_E5M2;
    if (epilogue == EPI_BIAS) {
        if (g5) launch_mxfp8<EPI_BIAS, FMT_E5M2, FMT_E4M3>(p, tiles, st); else launch_mxfp8<EPI_BIAS, FMT_E4M3, FMT_E4M3>(p, tiles, st);
    } else if (epilogue == EPI_GATED_RES) {
        if (g5) launch_mxfp8<EPI_GATED_RES, FMT_E5M2, FMT_E4M3>(p, tiles, st); else launch_mxfp8<EPI_GATED_RES, FMT_E4M3, FMT_E4M3>(p, tiles, st);
    } else if (g5) {
        if (o5) launch_mxfp8<EPI_DGELU, FMT_E5M2, FMT_E5M2>(p, tiles, st); else launch_mxfp8<EPI_DGELU, FMT_E5M2, FMT_E4M3>(p, tiles, st);
    } else {
        if (o5) launch_mxfp8<EPI_DGELU, FMT_E4M3, FMT_E5M2>(p, tiles, st); else launch_mxfp8<EPI_DGELU, FMT_E4M3, FMT_E4M3>(p, tiles, st);
    }
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---- bf16 -> e4m3 with a device scale (delayed scaling: the scale was fixed before this forward), amax of the input into a slot ----
template <int FMT>
__global__ __launch_bounds__(256) void cast_fp8_scaled_kernel(const bf16_t* x, long long ldx, unsigned char* y, long long ldy, bf16_t* cp,
                                                              long long ldcp, long long M, int K, int L, int Lj, int off, const float* scale,
                                                              unsigned int* amax_bits) {
    const int nch = K >> 3;
    const long long total = M * nch;
    const float sc = scale[0];
    float mx = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long m = i / nch;
        const int c = (int)(i - m * nch) * 8;
        const long long src = L > 0 ? (m / L) * Lj + off + m % L : m;
        const u32x4 raw = *(const u32x4*)(x + src * ldx + c);
        if (cp != nullptr) *(u32x4*)(cp + m * ldcp + c) = raw;
        float v[8];
        unpack8(raw, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(v[j]));
        *(u32x2*)(y + m * ldy + c) = (u32x2){fp8x4<FMT>(v, sc), fp8x4<FMT>(v + 4, sc)};
    }
    amax_publish_block(amax_bits, mx);
}
// Row m of y (and of the bf16 copy cp, if not null) comes from row (m / L) * Lj + off + m % L of x (L = 0: row m) -- one stream's rows
// of a joint [B * Lj, K] buffer.  y = satfinite(RNE(x / scale[0])); max |x| into amax (uint32 float bits, accumulated).
static int cast_fp8_launch(const void* x, long long ldx, void* y, long long ldy, void* cp, long long ldcp, long long M, int K, int L,
                           int Lj, int off, int fmt, const float* scale, unsigned int* amax, void* stream) {
    if (M <= 0 || K <= 0 || (K % 8) || (ldx % 8) || (ldy % 8) || ldx < K || ldy < K || scale == nullptr || amax == nullptr) return VT_ERR_BAD_SHAPE;
    if (cp != nullptr && (ldcp % 8 || ldcp < K)) return VT_ERR_BAD_SHAPE;
    if (L < 0 || (L > 0 && (Lj < L || off < 0 || off + L > Lj))) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)x) & 15) || (((uintptr_t)y) & 7) || (((uintptr_t)cp) & 15)) return VT_ERR_BAD_ALIGN;
    if (fmt != FMT_E4M3 && fmt != FMT_E5M2) return VT_ERR_UNSUPPORTED;
    const long long b = (M * (K >> 3) + 255) / 256;
    const unsigned blocks = (unsigned)(b > 4096 ? 4096 : b);
    if (fmt == FMT_E5M2)
        hipLaunchKernelGGL(cast_fp8_scaled_kernel<FMT_E5M2>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx,
                           (unsigned char*)y, ldy, (bf16_t*)cp, ldcp, M, K, L, Lj, off, scale, amax);
    else
        hipLaunchKernelGGL(cast_fp8_scaled_kernel<FMT_E4M3>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx,
                           (unsigned char*)y, ldy, (bf16_t*)cp, ldcp, M, K, L, Lj, off, scale, amax);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
extern "C" int vt_cast_fp8_scaled(const void* x, long long ldx, void* y, long long ldy, void* cp, long long ldcp, long long M, int K, int L,
                                  int Lj, int off, const float* scale, unsigned int* amax, void* stream) {
    return cast_fp8_launch(x, ldx, y, ldy, cp, ldcp, M, K, L, Lj, off, FMT_E4M3, scale, amax, stream);
}
// vt_cast_fp8_scaled with the target format as an argument (0 = e4m3, 1 = e5m2: satfinite at +-57344): the gradient cast
extern "C" int vt_cast_fp8_fmt(const void* x, long long ldx, void* y, long long ldy, void* cp, long long ldcp, long long M, int K, int L,
                               int Lj, int off, int fmt, const float* scale, unsigned int* amax, void* stream) {
    return cast_fp8_launch(x, ldx, y, ldy, cp, ldcp, M, K, L, Lj, off, fmt, scale, amax, stream);
}

// ---- y = x * gate[b(m), seg(m)] (vt_gate_mul, bit for bit) plus the fp8 copy of y and max |y|: the gated gradients of the backward ----
template <int FMT>
__global__ __launch_bounds__(256) void gate_mul_fp8_kernel(const bf16_t* x, int ldx, bf16_t* y, int ldy, const float* g_txt, const float* g_vid,
                                                          int bstride, long long M, int D, int S, int St, unsigned char* q, int ldq,
                                                          const float* scale, unsigned int* amax_bits) {
    const int nch = D >> 3;
    const long long total = M * nch;
    const float sc = scale[0];
    float mx = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long m = i / nch;
        const int c = (int)(i - m * nch);
        const int b = (int)(m / S);
        const int s = (int)(m - (long long)b * S);
        const float* g = (s < St ? g_txt : g_vid) + (size_t)b * bstride + c * 8;
        float v[8];
        unpack8(*(const u32x4*)(x + (size_t)m * ldx + c * 8), v);
        const f32x4 a = *(const f32x4*)g, bq = *(const f32x4*)(g + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] *= a[j]; v[j + 4] *= bq[j]; }
        const u32x4 out = pack8(v);
        *(u32x4*)(y + (size_t)m * ldy + c * 8) = out;
        unpack8(out, v);                                   // the bf16 values as written
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(v[j]));
        *(u32x2*)(q + (size_t)m * ldq + c * 8) = (u32x2){fp8x4<FMT>(v, sc), fp8x4<FMT>(v + 4, sc)};
    }
    amax_publish_block(amax_bits, mx);
}
// x, y, gates, M, D, S, St as vt_gate_mul; q: fp8 [M, ldq] = satfinite(RNE(y / scale[0])) in format fmt (0 = e4m3, 1 = e5m2);
// max |y| into amax (uint32 float bits, accumulated)
extern "C" int vt_gate_mul_fp8(const void* x, int ldx, void* y, int ldy, const float* g_txt, const float* g_vid, int bstride, long long M,
                               int D, int S, int St, void* q, int ldq, int fmt, const float* scale, unsigned int* amax, void* stream) {
    if (M <= 0 || D <= 0 || (D % 8) || (ldx % 8) || (ldy % 8) || (ldq % 8) || ldx < D || ldy < D || ldq < D || (bstride % 4) || S <= 0)
        return VT_ERR_BAD_SHAPE;
    if (q == nullptr || scale == nullptr || amax == nullptr) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)g_txt) | ((uintptr_t)g_vid)) & 15 || (((uintptr_t)q) & 7)) return VT_ERR_BAD_ALIGN;
    if (fmt != FMT_E4M3 && fmt != FMT_E5M2) return VT_ERR_UNSUPPORTED;
    const long long total = M * (D >> 3);
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    if (fmt == FMT_E5M2)
        hipLaunchKernelGGL(gate_mul_fp8_kernel<FMT_E5M2>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (bf16_t*)y, ldy,
                           g_txt, g_vid, bstride, M, D, S, St, (unsigned char*)q, ldq, scale, amax);
    else
        hipLaunchKernelGGL(gate_mul_fp8_kernel<FMT_E4M3>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (bf16_t*)y, ldy,
                           g_txt, g_vid, bstride, M, D, S, St, (unsigned char*)q, ldq, scale, amax);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---- delayed scaling: one thread per site rolls its amax history, sets the scale for the next forward and clears the slot ----
__global__ void fp8_scale_update_kernel(unsigned int* amax_bits, float* history, float* scale, int n, int H, float fmax) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* h = history + (size_t)i * H;
    float mx = __uint_as_float(amax_bits[i]);
    for (int j = H - 1; j > 0; --j) {
        const float v = h[j - 1];
        h[j] = v;
        mx = fmaxf(mx, v);
    }
    h[0] = __uint_as_float(amax_bits[i]);
    scale[i] = mx > 0.f ? __fdiv_rn(mx, fmax) : 1.0f;
    amax_bits[i] = 0u;
}
// amax: uint32 [n] (float bits); history: fp32 [n, H], newest first; scale: fp32 [n] = max(history) / 448 (1 if that is 0).
extern "C" int vt_fp8_scale_update(unsigned int* amax, float* history, float* scale, int n, int H, void* stream) {
    if (n <= 0 || H <= 0 || amax == nullptr || history == nullptr || scale == nullptr) return VT_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(fp8_scale_update_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, amax, history, scale, n, H, 448.0f);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
// the same with the format's largest finite value as the divisor: scale = max(history) / fmax (448: e4m3, 57344: e5m2)
extern "C" int vt_fp8_scale_update_fmax(unsigned int* amax, float* history, float* scale, int n, int H, float fmax, void* stream) {
    if (n <= 0 || H <= 0 || amax == nullptr || history == nullptr || scale == nullptr || !(fmax > 0.f)) return VT_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(fp8_scale_update_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, amax, history, scale, n, H, fmax);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
