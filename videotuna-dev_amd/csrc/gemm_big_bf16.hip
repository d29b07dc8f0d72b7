// bf16 MFMA GEMM for gfx950, large-tile version:  C[M,N] = A[M,K] * W[N,K]^T (+ fused epilogue), fp32 accumulate.
//
// Same contract and epilogues as gemm_bf16.hip (the nn.Linear layers of diffusers' CogVideoXBlock reached through
// videotuna/models/cogvideo_hf/cogvideo_pl.py:865-871, SURVEY 8(a) a4,a5); used for the token-sized problems.
//
// Why a second tiling: a wave that owns a 64x64 output tile reads (64+64) x 64 bf16 = 16 KiB of LDS per 64-deep
// K-tile for 512 Ki flop -- 32 flop per LDS byte, exactly the ratio of the CU's MFMA rate (4096 flop/clk) to its LDS
// bandwidth (128 B/clk), so the 128x128 kernel can never run the matrix cores above ~50 %.  Here the workgroup tile is
// 256x256x64 with 8 waves (2 x 4), each wave owning 128x64 = 8x4 tiles of v_mfma_f32_16x16x32_bf16 (128 accumulator
// registers, two waves per SIMD): 24 KiB of LDS reads per wave per K-tile for 1 Mi flop -> the LDS pipe is ~75 % busy
// at full MFMA rate.  Operands are staged by LDS-DMA (buffer_load ... lds, XOR swizzle applied to the source chunk),
// double-buffered (2 x 64 KiB); the accumulators leave through LDS in eight 32-row slabs so that the epilogue reads
// residuals / writes C in row-contiguous 512-B segments.
#include "gemm_epilogue.h"

#define GB_BM 256
#define GB_BN 256
#define GB_BK 64
#define GB_STAGE 65536      // A 32 KiB | W 32 KiB
#define GB_CS_LD 260        // fp32 row stride of the epilogue staging slab (32 rows x 260 floats = 32.5 KiB)
// The products are issued as v_mfma_f32_16x16x32_bf16 (two 32-deep k-steps per K-tile), not as 4 x 2 tiles of v_mfma_f32_32x32x16_bf16:
// same LDS image, same LDS bytes per flop, same cycles per flop -- but the chip holds a higher clock on the 16x16x32 shape under load
// (MI355X_MICROARCH.md, DVFS item 7).
// Staggered staging: waves 0..3 issue their LDS-DMA pieces at the start of a K-tile, waves 4..7 in its middle, so the two waves of a SIMD
// are never both busy issuing DMA (the issue cost of one hides under the MFMAs of the other): +2-5 %.  The variants that were measured
// against this body (four waves, loader waves, one piece per k-step, the 32x32x16 body, the timing ablations) are in csrc/exp/README.md.

typedef int gb_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ gb_i32x4 gb_words(const void* base, unsigned bytes) {     // raw descriptor words (inline-asm operand)
    const unsigned long long a = (unsigned long long)base;
    return (gb_i32x4){(int)(unsigned)a, (int)((a >> 32) & 0xffffu), (int)bytes, 0x00020000};
}

// PERSISTENT: one workgroup per CU (128 KiB of LDS), slot = (XCD, index inside the XCD) under round-robin dispatch;
// generation g of slot s computes tile g * G + s.  The first K-tile of the NEXT output tile is fetched while the last
// K-tile of the current one is multiplied and its epilogue runs, so neither a workgroup launch nor the first HBM round
// trip of a tile is exposed.
template <int EPI, bool OUT_F32>
__global__ __launch_bounds__(512, 1) void gemm_tn_big_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * GB_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;                  // 2 x 4 waves: rows 128 wm .., columns 64 wn ..
    const int nbm = (p.M + GB_BM - 1) / GB_BM, nbn = (p.N + GB_BN - 1) / GB_BN;
    const int ntiles = nbm * nbn;
    const int spx = gridDim.x >> 3;
    const int slot = (int)(blockIdx.x & 7) * spx + (int)(blockIdx.x >> 3);
    const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

    // ---- LDS-DMA staging: a K-tile of A (and of W) is 32 blocks of 1 KiB = 8 rows x 128 B; wave w moves blocks
    // w, w+8, w+16, w+24 of each operand.  Lane l lands at (row l>>3, physical chunk l&7) of its block and fetches
    // logical chunk (l&7) ^ swz(row); rows past M / N read zeros (bounds check).
    // swz(row) = (row >> 1) & 7: a 32-row MFMA fragment is read by ds_read_b128 in the lane groups {0-3,12-15,20-27},
    // {4-11,16-19,28-31} (+32); two rows of a group collide when they have the same parity (128-B rows, 256-B bank
    // period) and the same physical chunk, and (row >> 1) & 7 is distinct over the 8 same-parity rows of every group.
    // (row & 7, the 16-row-fragment swizzle of gemm_bf16.hip, gave 47 % conflict cycles here: rows 12 and 20 collide.)
    const int drl = lane >> 3, dcp = lane & 7;
    // every wave moves 4 pieces of A and of W per K-tile itself: piece j of this wave is block wave + 8 j = rows 8 (wave + 8 j) + drl:
    // swz(row) does not depend on j (8 * 8 j / 2 is a multiple of 8), so one per-lane offset serves all pieces and the row step goes into
    // the scalar offset
    const int row0p = 8 * wave + drl;
    const int sw = (row0p >> 1) & 7;
    const int a_voff0 = row0p * p.lda * 2 + ((dcp ^ sw) << 4);
    const int w_voff0 = row0p * p.ldw * 2 + ((dcp ^ sw) << 4);
    const int a_pstep = 64 * p.lda * 2, w_pstep = 64 * p.ldw * 2;
    auto dma = [&](const GemmTile& t, int kt, int buf) {
        const int soff = kt * GB_BK * 2;
        __amdgpu_buffer_rsrc_t ra = make_rsrc(t.a, t.a_bytes), rw = make_rsrc(t.w, t.w_bytes);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            char* dst = smem + buf * GB_STAGE + (wave + 8 * j) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)dst, 16, a_voff0, soff + j * a_pstep, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(dst + 32768), 16, w_voff0, soff + j * w_pstep, 0, 0);
        }
    };
    // the same transfer through inline asm, for the cross-tile prefetch: the compiler orders every later LDS access behind
    // an LDS-DMA it knows about, which would park the whole epilogue behind the fetch.  Safe: it is older than every memory
    // operation of the epilogue (vmcnt retires in order, so each wait the compiler computes there also covers it), and the
    // next tile starts with a full barrier (vmcnt(0)).
    auto dma_hidden = [&](const GemmTile& t, int buf) {
        const gb_i32x4 ra = gb_words(t.a, t.a_bytes), rw = gb_words(t.w, t.w_bytes);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned dst = smem_lds + buf * GB_STAGE + (wave + 8 * j) * 1024;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(dst), "v"(a_voff0), "s"(ra), "s"(j * a_pstep) : "memory");
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(dst + 32768), "v"(w_voff0), "s"(rw), "s"(j * w_pstep) : "memory");
        }
    };

    const int nk = p.K / GB_BK;
    const int fr16 = lane & 15, fq = lane >> 4, fx16 = (fr16 >> 1) & 7;   // 16-row fragments: row, k-chunk of a 32-deep k-step, swz(row)
    const int er = tid >> 6;              // epilogue: 0..7, row inside an 8-row pass
    const int ec = (tid & 63) * 4;        // epilogue: first of this thread's 4 columns

    if (slot >= ntiles) return;
    GemmTile cur = gemm_tile<GB_BM, GB_BN>(p, slot, nbm, nbn);
    int buf = 0;
    dma(cur, 0, 0);
    for (int tile = slot; tile < ntiles; tile += gridDim.x) {
        const bool has_next = tile + (int)gridDim.x < ntiles;
        GemmTile nxt = cur;
        if (has_next) nxt = gemm_tile<GB_BM, GB_BN>(p, tile + gridDim.x, nbm, nbn);

        // acc16[tn][tm] = D[n][m] of a 16 x 16 tile: lane holds m = lane & 15 and the four consecutive columns n = 4 (lane >> 4) + r
        f32x4 acc16[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc16[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

        __syncthreads();                  // vmcnt(0): the first K-tile (fetched during the previous tile) has landed
        for (int kt = 0; kt < nk; ++kt) {
            const bool last = kt + 1 == nk;
            auto issue = [&]() {                // the next K-tile, or the first one of the next output tile
                if (!last) dma(cur, kt + 1, buf ^ 1);
                else if (has_next) dma_hidden(nxt, buf ^ 1);
            };
            const bool late = wave >= 4;
            if (!late) issue();
            // 16-row fragments: lane reads row (lane & 15), logical chunk 4 ks + (lane >> 4) of the 8 chunks of a 64-deep row; swz(row) =
            // (row >> 1) & 7 only depends on lane & 15 (tiles are 16-aligned) and the ds_read_b128 lane groups stay conflict-free
            const char* As = smem + buf * GB_STAGE + (wm * 128 + fr16) * 128;
            const char* Ws = smem + buf * GB_STAGE + 32768 + (wn * 64 + fr16) * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks == 1 && late) issue();
                const int coff = (((ks * 4 + fq) ^ fx16) << 4);
                bf16x8 af[8], wf[4];
#pragma unroll
                for (int t = 0; t < 8; ++t) af[t] = *(const bf16x8*)(As + t * 2048 + coff);
#pragma unroll
                for (int t = 0; t < 4; ++t) wf[t] = *(const bf16x8*)(Ws + t * 2048 + coff);
#pragma unroll
                for (int tm = 0; tm < 8; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 4; ++tn)
                        acc16[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tn], af[tm], acc16[tn][tm], 0, 0, 0);
            }
            if (!last) __syncthreads();   // its vmcnt(0) also retires the next K-tile's LDS-DMA (in the waves that issued it)
            else gemm_lds_barrier();        // the cross-tile prefetch keeps flying
            buf ^= 1;
        }

        // ---------------- epilogue: eight 32-row slabs through the stage that was just consumed ----------------
        float* Cs = (float*)(smem + (buf ^ 1) * GB_STAGE);
        const int n = cur.col0 + ec;
        float bias4[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias != nullptr && n < p.N) {
#pragma unroll
            for (int j = 0; j < 4; ++j) bias4[j] = bf2f(p.bias[n + j]);
        }
        // second operand of the epilogue (residual / saved pre-activation): fetched one slab ahead of its use
        constexpr bool HAS_AUX = EPI == EPI_GATED_RES || EPI == EPI_DGELU;
        u32x2 aux[4], auxn[4];
        auto aux_fetch = [&](int slab, u32x2* dst) {
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int m = cur.row0 + slab * 32 + pass * 8 + er;
                dst[pass] = (u32x2){0u, 0u};
                // (wave < 8 here and below is always true with 512 threads; removing it changes the generated code, so it stays)
                if (HAS_AUX && wave < 8 && m < p.M && n < p.N) dst[pass] = gemm_epilogue_aux_load<EPI>(p, m, n);
            }
        };
        aux_fetch(0, aux);
        GateCtx gctx;
        if (EPI == EPI_GATED_RES) gctx = gate_ctx_load(p, cur.row0, GB_BM, n);
#pragma unroll
        for (int slab = 0; slab < 8; ++slab) {
            if (wave < 8 && wm == (slab >> 2)) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                    for (int tn = 0; tn < 4; ++tn)
                        *(f32x4*)(Cs + (t2 * 16 + fr16) * GB_CS_LD + wn * 64 + tn * 16 + 4 * fq) = acc16[tn][(slab & 3) * 2 + t2];
            }
            gemm_lds_barrier();
            if (slab < 7) aux_fetch(slab + 1, auxn);
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int ml = pass * 8 + er;
                const int m = cur.row0 + slab * 32 + ml;
                if (wave < 8 && m < p.M && n < p.N) {
                    const f32x4 v = *(const f32x4*)(Cs + ml * GB_CS_LD + ec);
                    gemm_epilogue_store_aux<EPI, OUT_F32>(p, m, n, v, bias4, aux[pass], EPI == EPI_GATED_RES ? &gctx : nullptr);
                }
            }
            gemm_lds_barrier();
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) aux[pass] = auxn[pass];
        }
        cur = nxt;
    }
}

template <int EPI, bool F32>
static int launch_big(const GemmParams& p, hipStream_t st) {
    const int nbm = (p.M + GB_BM - 1) / GB_BM, nbn = (p.N + GB_BN - 1) / GB_BN;
    static int slots = 0;                 // persistent grid: one workgroup per CU, a multiple of 8
    if (slots == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
        slots = cus >= 8 ? cus / 8 * 8 : 8;
    }
    const int ntiles = nbm * nbn;
    const int grid = ntiles < slots ? (ntiles + 7) / 8 * 8 : slots;
    hipLaunchKernelGGL((gemm_tn_big_kernel<EPI, F32>), dim3(grid), dim3(512), 0, st, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// same validation as vt_gemm_bf16 (gemm_bf16.hip), which calls this for large problems
int vt_gemm_big_dispatch(const GemmParams& p, int epilogue, int out_fp32, hipStream_t st) {
    switch (epilogue) {
        case EPI_BIAS:
            return out_fp32 ? launch_big<EPI_BIAS, true>(p, st) : launch_big<EPI_BIAS, false>(p, st);
        case EPI_BIAS_GELU: return launch_big<EPI_BIAS_GELU, false>(p, st);
        case EPI_GATED_RES: return launch_big<EPI_GATED_RES, false>(p, st);
        case EPI_DGELU: return launch_big<EPI_DGELU, false>(p, st);
        default: return VT_ERR_UNSUPPORTED;
    }
}
