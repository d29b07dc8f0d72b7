// bf16 MFMA GEMM for gfx950:  C[M,N] = A[M,K] * W[N,K]^T  (+ fused epilogue), fp32 accumulate.
//
// Both operands are K-contiguous ("TN"), which is what every linear layer of the DiT needs in the
// forward (W = nn.Linear weight [out,in]) and, with a pre-transposed copy of the weight, in the
// backward dX = dY * W.  Reference ops replaced: every nn.Linear of diffusers' CogVideoXBlock that
// the reference reaches through videotuna/models/cogvideo_hf/cogvideo_pl.py:865-871 (SURVEY 8(a) a4,a5).
//
// Structure: 128x128x64 workgroup tile, 4 waves (2x2), each wave 64x64 = 4x4 tiles of
// v_mfma_f32_16x16x32_bf16.  Operands are staged by LDS-DMA (buffer_load ... lds; XOR-swizzled 16-byte chunks,
// conflict-free ds_read_b128), double-buffered so the loads of K-tile t+1 are in flight while tile t
// is multiplied.  Global loads are bounds-checked raw buffer loads, so ragged M / N edges read zeros.  The MFMA is issued as (W-frag, A-frag) so each lane ends up with 4
// consecutive output columns of one row; the accumulators go through LDS once so the epilogue reads
// residual / writes C in row-contiguous, fully coalesced 128-B segments.
#include "gemm_epilogue.h"

#define BM 128
#define BN 128
#define BK 64
#define CS_LD 132   // fp32 row stride of the epilogue staging tile (64 rows x 132 floats = 33 KiB)

template <int EPI, bool OUT_F32>
__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(16))) char smem[65536];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
    // XCD-aware id, then grouped ordering (8 row-tiles per group, column-tiles outer)
    const int id = xcd_remap(blockIdx.x, nbm * nbn);
    const int GM = 8;
    const int in_group = GM * nbn;
    const int group = id / in_group;
    const int first_m = group * GM;
    const int gsz = min(nbm - first_m, GM);
    const int tile_m = first_m + (id % in_group) % gsz;
    const int tile_n = (id % in_group) / gsz;
    const int row0 = tile_m * BM, col0 = tile_n * BN;

    // bounds-checked descriptors rooted at this tile's first row
    const long long a_rem = (long long)(p.M - row0) * p.lda * 2;
    const long long w_rem = (long long)(p.N - col0) * p.ldw * 2;
    __amdgpu_buffer_rsrc_t ra = make_rsrc(p.A + (size_t)row0 * p.lda, (unsigned)(a_rem > 0x7fffffffLL ? 0x7fffffffLL : a_rem));
    __amdgpu_buffer_rsrc_t rw = make_rsrc(p.W + (size_t)col0 * p.ldw, (unsigned)(w_rem > 0x7fffffffLL ? 0x7fffffffLL : w_rem));

    // ---- LDS-DMA staging: a K-tile of A (and of W) is 16 blocks of 1 KiB = 8 rows x 128 B; wave w moves blocks
    // w, w+4, w+8, w+12 of each operand.  One buffer_load..lds writes lane l at block + 16 l = (row l>>3, physical
    // chunk l&7), so the XOR swizzle is applied to the SOURCE chunk; out-of-range rows read zeros (bounds check).
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int drl = lane >> 3, dcp = lane & 7;
    int a_voff[4], w_voff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 8 * (wv + 4 * j) + drl;
        a_voff[j] = row * p.lda * 2 + ((dcp ^ drl) << 4);
        w_voff[j] = row * p.ldw * 2 + ((dcp ^ drl) << 4);
    }
    auto dma = [&](int kt, int buf) {
        const int soff = kt * BK * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            char* dst = smem + buf * 32768 + (wv + 4 * j) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)dst, 16, a_voff[j], soff, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(dst + 16384), 16, w_voff[j], soff, 0, 0);
        }
    };

    f32x4 acc[4][4];   // [tn][tm]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / BK;
    dma(0, 0);
    __syncthreads();
    const int frow = lane & 15;            // row inside a 16-row fragment
    const int fq = lane >> 4;              // k-chunk inside a 32-deep k-step
    const int fx = lane & 7;               // == (row & 7) for every fragment row this lane reads
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) dma(kt + 1, buf ^ 1);
        const char* As = smem + buf * 32768;
        const char* Ws = As + 16384;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int coff = (((ks * 4 + fq) ^ fx) << 4);
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = *(const bf16x8*)(As + (wm * 64 + t * 16 + frow) * 128 + coff);
                wf[t] = *(const bf16x8*)(Ws + (wn * 64 + t * 16 + frow) * 128 + coff);
            }
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm)
                    acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tn], af[tm], acc[tn][tm], 0, 0, 0);
        }
        __syncthreads();       // the barrier's vmcnt(0) also retires the next tile's LDS-DMA
    }

    // ---------------- epilogue: two 64-row halves through LDS ----------------
    float* Cs = (float*)smem;
    const int er = tid >> 5;              // 0..7 : row inside an 8-row pass
    const int ec = (tid & 31) * 4;        // first of this thread's 4 columns
    const int n = col0 + ec;
    float bias4[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias != nullptr && n < p.N) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bias4[j] = bf2f(p.bias[n + j]);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (wm == half) {
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) {
                    int ml = tm * 16 + frow;
                    int nl = wn * 64 + tn * 16 + fq * 4;
                    *(f32x4*)(Cs + ml * CS_LD + nl) = acc[tn][tm];
                }
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 8; ++pass) {
            const int ml = pass * 8 + er;
            const int m = row0 + half * 64 + ml;
            if (m < p.M && n < p.N) {
                f32x4 v = *(const f32x4*)(Cs + ml * CS_LD + ec);
                gemm_epilogue_store<EPI, OUT_F32>(p, m, n, v, bias4);
            }
        }
        __syncthreads();
    }
}

template <int EPI, bool F32>
static int launch(const GemmParams& p, hipStream_t st) {
    const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
    hipLaunchKernelGGL((gemm_tn_kernel<EPI, F32>), dim3(nbm * nbn), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// the bf16 matrices of the epilogue (C, C2, R, U) are accessed 8 bytes at a time by every kernel; the 256x256 kernel widens to 16 bytes
// where it finds them 16-byte aligned (gemm_big_bf16.hip, big_wide)
static bool al8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

// 256x256-tile kernel (gemm_big_bf16.hip) for the token-sized problems; 0 = choose by shape, 1 = always 128x128, 2 = always 256x256
int vt_gemm_big_dispatch(const GemmParams& p, int epilogue, int out_fp32, hipStream_t st);
int vt_gemm_pc_dispatch(const GemmParams& p, int epilogue, int out_fp32, hipStream_t st);     // gemm_pc_bf16.hip
static int g_gemm_tile = 0;
extern "C" int vt_gemm_set_tile(int mode) {
    if (mode < 0 || mode > 3) return VT_ERR_BAD_SHAPE;
    g_gemm_tile = mode;
    return VT_OK;
}
// which tiling: 1 = 128x128 (this file), 2 = 256x256 (gemm_big_bf16.hip), 3 = 256x128 producer/consumer (gemm_pc_bf16.hip).
// (r03: a 256x256 kernel with a four-stage ring of 32-deep K-tiles, counted vmcnt and half-K-tile fragment prefetch measured 5-10 % SLOWER
// than gemm_big on every shape: csrc/exp/gemm_ring_bf16.hip, profiles/r03_gemm_ring_experiment.txt)
// r01 measurements (tools/kbench.py gemm), TF/s for 128^2 / 256^2 / producer-consumer:
//   M=35552: N=5760 K=1984  828 / 1012 / 1025 | N=7680 K=1920 978 / 1099 / 1048 | N=1920 K=7680 925 /  999 / 1104
//            N=1984 K=5760  938 / 1042 / 1085 | N=1920 K=1984 957 /  913 /  975 | N=1984 K=1920 931 /  961 /  983
//   M=17776: N=5760 1015 / 1034 / 1043 | N=7680 968 / 1061 / 1024 | N=1920 K=7680 918 / 875 / 1018 | N=1984 K=5760 951 / 917 / 996
//            N=1920 K=1984 901 / 825 / 907        8192^3: 1050 / 1236 / 1211
static int pick_tile(int M, int N, int K) {
    const int mode = g_gemm_tile;
    if (mode) return mode;
    const long long t256 = (long long)((M + 255) / 256) * ((N + 255) / 256);
    const long long tpc = (long long)((M + 255) / 256) * ((N + 127) / 128);
    if (N >= 6144 && t256 >= 512) return 2;
    // r03 sweep (profiles/r03_gemm_shapes_tile_modes.txt: every shape of the four models under each tiling): the persistent 256x256 kernel also
    // wins 4-17 % wherever its tiles fill whole passes of the chip (>= 90 % of the last one, or a single pass of >= 160 tiles) and the
    // output is wide (N >= 2560: CogVideoX qkv 5760, STDiT 3840 / 4608, HunyuanVideo 3072 with K = 12288 / 15360, the UNet's GEGLU 5120),
    // at the UNet's own widths 640 / 1280, and at N = 1984 (the K-extended qkv input gradient); it loses at 1152 (4.5 tiles), at 1920 with
    // a long K (the 256x128 producer / consumer kernel splits 1920 into 15 exact tiles) and at 320
    if (K >= 512 && M >= 1024) {
        const long long passes = (t256 + 255) / 256;
        const bool full = t256 <= 256 ? t256 >= 160 : 10 * t256 >= 9 * passes * 256;
        if (full && (N >= 2560 || ((N % 640) == 0 && N <= 1280) || ((N % 256) >= 192 && K >= 4096))) return 2;
        // with the eight-phase K-loop (profiles/gemm_big8_kbench.txt: all three kernels interleaved per shape) the 256x256 kernel takes 8-26 %
        // less time than the producer / consumer kernel at N = 1920 and 1984 for every K (CogVideoX out / ff2 projections and the input gradients
        // of qkv, out and ff1: 93.75 % and 97 % of the last column tile used), also at 4.3 passes of the chip (M = 35552); it still loses
        // at 1152 (90 %) and 320.  Only the products with K < 4096 move here (DESIGN.md 8, item 2 has the rest).  What was measured:
        // the 15/16 rule at N = 1920 and 1984 only, the 85 % pass fill at M = 35552 with those two N only; no other N whose last column
        // tile is at least 15/16 used was timed
        const long long nbn = (N + 255) / 256;
        const bool most = t256 > 256 && 100 * t256 >= 85 * passes * 256;
        if ((full || most) && K < 4096 && 16LL * N >= 15 * 256 * nbn) return 2;
    }
    if (tpc >= 512 && K >= 512) return 3;
    // a few hundred rows against a large weight (the frozen T5 encoder: 452 x [4096 .. 20480] x [4096 .. 10240]): the weights
    // come from HBM, not the L2, and the producer / consumer ring keeps two (128-row tile: three) K-tiles in flight per CU
    // (11.5 -> 8.5 ms per T5 forward)
    if (M > 64 && M <= 1024 && (long long)N * K >= (1LL << 24)) return 3;
    return 1;
}

int vt_gemm_pc_bm(int M);     // gemm_pc_bf16.hip
// which kernel vt_gemm_bf16 launches for an (M, N, K) problem under the current tile mode: 1 = 128x128, 2 = 256x256, 3 = 256x128
// producer / consumer, 4 = the producer / consumer kernel's 128-row instantiation.  The three kernels sum the same MFMA products in the
// same K order, so their outputs are bit-identical and cannot tell which one ran (tests: dispatch coverage of the production shapes)
extern "C" int vt_gemm_bf16_kernel(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return VT_ERR_BAD_SHAPE;
    const int tile = pick_tile(M, N, K);
    return tile == 3 && vt_gemm_pc_bm(M) == 128 ? 4 : tile;
}

// The measured rule for the two CogVideoX block products that pick_tile leaves on the producer / consumer kernel (ff.net.2 forward and
// the input gradient of ff.net.0.proj: N = 1920, or 1984 with the LoRA K-extension columns, K = 7680 / 7744), for callers that know
// their shape and pass the answer to vt_gemm_bf16_tile.  2 = the 256x256 kernel, 0 = no opinion (pick_tile decides).
// profiles/gemm_big8_kbench.txt, M = 71104, us per launch, 256x256 default loop / producer-consumer / 128x128:
//   N=1920 K=7680 bias   1522.5 / 1804.1 / 2363.3      N=1920 K=7680 gated  1590.1 / 1916.2 / 2438.1
//   N=1920 K=1984 bias    452.9 /  528.0 /  568.3      N=1984 K=1920 bias    451.0 /  602.2 /  606.2      N=1984 K=5760 bias 1172.2 / 1436.3 / 1652.9
// The rule is pick_tile's own for K < 4096 without the K bound: the last column tile at least 15/16 used and the tiles filling whole passes
// of the chip (>= 90 % of the last one or a single pass of >= 160 tiles, or >= 85 % of all passes beyond one); only the two N that were
// measured answer 2.  pick_tile itself keeps K >= 4096 on the producer / consumer kernel: its answers are pinned by the dispatch tests.
extern "C" int vt_gemm_bf16_block_tile(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return VT_ERR_BAD_SHAPE;
    if ((N != 1920 && N != 1984) || (K % BK) != 0 || K < 512 || M < 1024) return 0;
    const long long nbn = (N + 255) / 256, t256 = (long long)((M + 255) / 256) * nbn;
    const long long passes = (t256 + 255) / 256;
    const bool full = t256 <= 256 ? t256 >= 160 : 10 * t256 >= 9 * passes * 256;
    const bool most = t256 > 256 && 100 * t256 >= 85 * passes * 256;
    return ((full || most) && 16LL * N >= 15 * 256 * nbn) ? 2 : 0;
}

// tile: 0 = pick_tile, 1 / 2 / 3 = that kernel as under vt_gemm_set_tile; a global mode set by vt_gemm_set_tile wins over it
extern "C" int vt_gemm_bf16_tile(const void* A, int lda, const void* W, int ldw, void* C, int ldc,
                            int M, int N, int K, const void* bias, int epilogue, int out_fp32,
                            const void* R, int ldr, int r_mod,
                            const float* gate_txt, const float* gate_vid, int gate_bstride, int S, int St,
                            void* C2, int ldc2, const void* U, int ldu, int tile_req, void* stream) {
    if (tile_req < 0 || tile_req > 3) return VT_ERR_BAD_SHAPE;
    if (M <= 0 || N <= 0 || K <= 0 || (K % BK) != 0 || (N % 4) != 0) return VT_ERR_BAD_SHAPE;
    if ((lda % 8) || (ldw % 8) || (ldc % 4) || lda < K || ldw < K || ldc < N) return VT_ERR_BAD_SHAPE;
    if (!al16(A) || !al16(W) || !(out_fp32 ? al16(C) : al8(C))) return VT_ERR_BAD_ALIGN;
    GemmParams p;
    p.A = (const bf16_t*)A; p.W = (const bf16_t*)W; p.C = C; p.bias = (const bf16_t*)bias;
    p.R = (const bf16_t*)R; p.gate_txt = gate_txt; p.gate_vid = gate_vid;
    p.C2 = (bf16_t*)C2; p.U = (const bf16_t*)U;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldr = ldr; p.ldc2 = ldc2; p.ldu = ldu;
    p.S = S > 0 ? S : 1; p.St = St; p.gate_bstride = gate_bstride; p.r_mod = r_mod; p.splits = 1;
    hipStream_t st = (hipStream_t)stream;
    const int tile = (g_gemm_tile == 0 && tile_req != 0) ? tile_req : pick_tile(M, N, K);
    const bool big = tile == 2;
    if (tile == 3) {                                     // producer / consumer kernel (256x128 tile)
        if (epilogue == EPI_BIAS_GELU && (out_fp32 || C2 == nullptr || (ldc2 % 4) || !al8(C2))) return VT_ERR_BAD_SHAPE;
        if (epilogue == EPI_GATED_RES && (out_fp32 || R == nullptr || (ldr % 4) || !al8(R))) return VT_ERR_BAD_SHAPE;
        if (epilogue == EPI_DGELU && (out_fp32 || U == nullptr || (ldu % 4) || !al8(U))) return VT_ERR_BAD_SHAPE;
        return vt_gemm_pc_dispatch(p, epilogue, out_fp32, st);
    }
    switch (epilogue) {
        case EPI_BIAS:
            if (big) return vt_gemm_big_dispatch(p, epilogue, out_fp32, st);
            return out_fp32 ? launch<EPI_BIAS, true>(p, st) : launch<EPI_BIAS, false>(p, st);
        case EPI_BIAS_GELU:
            if (out_fp32 || C2 == nullptr || (ldc2 % 4) || !al8(C2)) return VT_ERR_BAD_SHAPE;
            if (big) return vt_gemm_big_dispatch(p, epilogue, 0, st);
            return launch<EPI_BIAS_GELU, false>(p, st);
        case EPI_GATED_RES:
            if (out_fp32 || R == nullptr || (ldr % 4) || !al8(R)) return VT_ERR_BAD_SHAPE;
            if (C2 != nullptr && ((ldc2 % 4) || !al8(C2))) return VT_ERR_BAD_SHAPE;
            if (gate_vid != nullptr && (gate_txt == nullptr || (gate_bstride % 4) || !al16(gate_vid) || !al16(gate_txt)))
                return VT_ERR_BAD_SHAPE;
            if (big) return vt_gemm_big_dispatch(p, epilogue, 0, st);
            return launch<EPI_GATED_RES, false>(p, st);
        case EPI_DGELU:
            if (out_fp32 || U == nullptr || (ldu % 4) || !al8(U)) return VT_ERR_BAD_SHAPE;
            if (big) return vt_gemm_big_dispatch(p, epilogue, 0, st);
            return launch<EPI_DGELU, false>(p, st);
        default:
            return VT_ERR_UNSUPPORTED;
    }
}

extern "C" int vt_gemm_bf16(const void* A, int lda, const void* W, int ldw, void* C, int ldc,
                            int M, int N, int K, const void* bias, int epilogue, int out_fp32,
                            const void* R, int ldr, int r_mod,
                            const float* gate_txt, const float* gate_vid, int gate_bstride, int S, int St,
                            void* C2, int ldc2, const void* U, int ldu, void* stream) {
    return vt_gemm_bf16_tile(A, lda, W, ldw, C, ldc, M, N, K, bias, epilogue, out_fp32, R, ldr, r_mod, gate_txt, gate_vid, gate_bstride, S, St,
                             C2, ldc2, U, ldu, 0, stream);
}
