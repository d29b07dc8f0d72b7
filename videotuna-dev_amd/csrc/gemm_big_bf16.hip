// bf16 MFMA GEMM for gfx950, large-tile version:  C[M,N] = A[M,K] * W[N,K]^T (+ fused epilogue), fp32 accumulate.
//
// Same contract and epilogues as gemm_bf16.hip (the nn.Linear layers of diffusers' CogVideoXBlock reached through
// videotuna/models/cogvideo_hf/cogvideo_pl.py:865-871, SURVEY 8(a) a4,a5); used for the token-sized problems.
//
// Why a second tiling: a wave that owns a 64x64 output tile reads (64+64) x 64 bf16 = 16 KiB of LDS per 64-deep
// K-tile for 512 Ki flop -- 32 flop per LDS byte, against 16 flop per byte that the CU can feed (MFMA rate 4096 flop/clk,
// ds_read_b128 256 B/clk: MI355X_MICROARCH.md), so the 128x128 kernel keeps the LDS pipe half busy for fragments alone,
// next to the staging writes and the epilogue.  Here the workgroup tile is
// 256x256x64 with 8 waves (2 x 4), each wave owning 128x64 = 8x4 tiles of v_mfma_f32_16x16x32_bf16 (128 accumulator
// registers, two waves per SIMD): 24 KiB of LDS reads per wave per K-tile for 1 Mi flop -> 43 flop per byte, the LDS
// pipe is under 40 % busy at full MFMA rate.  Operands are staged by LDS-DMA (buffer_load ... lds, XOR swizzle applied to the source chunk),
// double-buffered (2 x 64 KiB); the accumulators leave through LDS in eight 32-row slabs so that the epilogue reads
// residuals / writes C in row-contiguous 512-B segments (16 bytes per lane where alignment allows: big_wide below).
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
//
// Two K-loops, template PHASED (vt_gemm_set_big_loop; bit-identical results, the choice per shape is big_loop_phased below):
//   two-phase   one __syncthreads() per K-tile, whose vmcnt(0) retires the next K-tile's LDS-DMA: one K-tile in flight, every K-tile
//               pays an LDS round trip behind a full drain.
//   eight-phase cdna_hip_programming.md, "The 256^2 8-phase template": four phases of 16 MFMAs per K-tile between raw s_barriers,
//               one half-tile of LDS-DMA issued per phase, one counted s_waitcnt vmcnt(6) per K-tile (three half-tiles stay in
//               flight across it), waves 4-7 one barrier behind waves 0-3 so that on every SIMD one wave multiplies while the
//               other reads fragments and issues DMA.  The default from 8 K-tiles up, from 2 where N >= 2560 (profiles/gemm_big8_kbench.txt).

typedef int gb_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ gb_i32x4 gb_words(const void* base, unsigned bytes) {     // raw descriptor words (inline-asm operand)
    const unsigned long long a = (unsigned long long)base;
    return (gb_i32x4){(int)(unsigned)a, (int)((a >> 32) & 0xffffu), (int)bytes, 0x00020000};
}

// PERSISTENT: one workgroup per CU (128 KiB of LDS), slot = (XCD, index inside the XCD) under round-robin dispatch;
// generation g of slot s computes tile g * G + s.  The first K-tile of the NEXT output tile is fetched while the last
// K-tile of the current one is multiplied and its epilogue runs, so neither a workgroup launch nor the first HBM round
// trip of a tile is exposed.
template <int EPI, bool OUT_F32, bool PHASED, bool WIDE>
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

    // eight-phase loop: the staging unit is a half-tile = 2 of the wave's 8 pieces.  h = 0: A pieces 0, 2 (rows 0-63 of both wave rows,
    // read in phase 1), 1: A pieces 1, 3 (rows 64-127 of both, phase 3), 2: W pieces 0, 1, 3: W pieces 2, 3 (phases 1 and 2).  Always
    // through inline asm: the compiler must not know of these transfers, or it drains them (vmcnt(0)) at its next LDS access.
    // (m0 is written without being named as a clobber, as in dma_hidden: it is a reserved register on this target -- the compiler
    // rejects it in a clobber list, keeps no value live in it and sets it itself right before each of its own instructions that read it.)
    auto half = [&](const gb_i32x4 ra, const gb_i32x4 rw, int kt, int b, int h) {
        const unsigned dst = smem_lds + b * GB_STAGE + wave * 1024 + (h >= 2 ? 32768 : 0);
        const int j0 = h == 0 ? 0 : h == 1 ? 1 : h == 2 ? 0 : 2, j1 = h == 0 ? 2 : h == 1 ? 3 : h == 2 ? 1 : 3;
        const int soff = kt * GB_BK * 2, pstep = h >= 2 ? w_pstep : a_pstep, voff = h >= 2 ? w_voff0 : a_voff0;
        const gb_i32x4 rs = h >= 2 ? rw : ra;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(dst + j0 * 8192), "v"(voff), "s"(rs), "s"(soff + j0 * pstep) : "memory");
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(dst + j1 * 8192), "v"(voff), "s"(rs), "s"(soff + j1 * pstep) : "memory");
    };

    const int nk = p.K / GB_BK;
    const int fr16 = lane & 15, fq = lane >> 4, fx16 = (fr16 >> 1) & 7;   // 16-row fragments: row, k-chunk of a 32-deep k-step, swz(row)
    const int er = WIDE ? tid >> 5 : tid >> 6;                  // epilogue: row inside a 16-row (WIDE) / 8-row pass
    const int ec = WIDE ? (tid & 31) * 8 : (tid & 63) * 4;      // epilogue: first of this thread's 8 (WIDE) / 4 columns

    if (slot >= ntiles) return;
    GemmTile cur = gemm_tile<GB_BM, GB_BN>(p, slot, nbm, nbn);
    int buf = 0;
    if constexpr (PHASED) {
#pragma unroll
        for (int h = 0; h < 4; ++h) half(gb_words(cur.a, cur.a_bytes), gb_words(cur.w, cur.w_bytes), 0, 0, h);
    } else {
    dma(cur, 0, 0);
    }
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

        if constexpr (!PHASED) {
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
        } else {
        // ---- eight-phase loop (cdna_hip_programming.md, "The 256^2 8-phase template"): a K-tile is four phases, one 64 x 32 quadrant of
        // the wave's 128 x 64 output each (16 MFMAs), in the order (A rows 0-63, W cols 0-31), (0-63, 32-63), (64-127, 32-63),
        // (64-127, 0-31); the fragment reads are 4 W + 8 A, 4 W, 8 A, none (the first W fragments stay in registers).  Each acc16 tile
        // still receives K-tile 0 (k-step 0, 1), K-tile 1 (k-step 0, 1), ...: bit-identical to the two-phase loop.
        // A phase is: fragment reads (W before A, order pinned), one half-tile of LDS-DMA, s_waitcnt lgkmcnt(0), s_barrier, s_setprio 1,
        // 16 MFMAs, s_setprio 0, s_barrier.  Waves 4-7 take one extra barrier before the loop and waves 0-3 one after it: in the slot
        // between two barriers one wave of every SIMD is in its MFMA half and the other in its read half.
        // Staging runs along the stream of K-tiles q = 0 .. nk-1 of this output tile followed by q = nk, the first K-tile of the next
        // one; K-tile q lives in stage buf ^ (q & 1) (so the next output tile starts in the stage its predecessor's epilogue does not
        // use).  Every phase issues one half-tile, in the order the stage is vacated:
        //   phase 1 of K-tile kt: half 1 of kt+1    (its region of the other stage was last read in phase 3 of kt-1)
        //   phase 2:              half 0 of kt+2    (this stage; last read in phase 1 of kt)
        //   phase 3:              half 2 of kt+2    (last read in phase 2)
        //   phase 4:              half 3 of kt+2    (last read in phase 2), then s_waitcnt vmcnt(6): only the three half-tiles of kt+2 stay
        //                         in flight, K-tile kt+1 has landed in this wave.
        // Write after read, by the counts: a wave retires the reads of phase p (lgkmcnt(0)) before it enters the first barrier of p;
        // the late waves enter it one slot after the early ones, and an early wave's DMA of phase p+1 is issued after it has left
        // that same barrier (its second of phase p).  So restaging one phase after the last read is ordered for both wave groups.
        // Read after write: the late waves' vmcnt(6) of phase 4 precedes their first barrier of that phase, which is the early waves'
        // second; the early waves' first read of K-tile kt+1 follows it (phase 1 of kt+1), the late waves' comes a slot later.
        // K-tile nk+1 does not exist: the last K-tile's stage is the epilogue's slab, so the halves 0, 2, 3 of K-tile 1 of the next
        // output tile are issued at its start, after the epilogue, followed by the same counted wait (which also covers the epilogue's
        // stores: they are older).  Without a next output tile nothing is in flight past K-tile nk-1 and the wait before it is vmcnt(0).
        const bool late = wave >= 4;
        const gb_i32x4 ra_c = gb_words(cur.a, cur.a_bytes), rw_c = gb_words(cur.w, cur.w_bytes);
        const gb_i32x4 ra_n = gb_words(nxt.a, nxt.a_bytes), rw_n = gb_words(nxt.w, nxt.w_bytes);
        {
            const bool own = nk > 1;
            if (own || has_next) {
                half(own ? ra_c : ra_n, own ? rw_c : rw_n, own ? 1 : 0, buf ^ 1, 0);
                half(own ? ra_c : ra_n, own ? rw_c : rw_n, own ? 1 : 0, buf ^ 1, 2);
                half(own ? ra_c : ra_n, own ? rw_c : rw_n, own ? 1 : 0, buf ^ 1, 3);
                asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            asm volatile("s_barrier" ::: "memory");
            if (late) asm volatile("s_barrier" ::: "memory");       // waves 4-7 run one barrier behind waves 0-3 through the K-loop
        }
        bf16x8 fa[4][2], fw0[2][2], fw1[2][2];            // [16-row tile][k-step]
        auto read_a = [&](const char* As, int qa) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) fa[t][ks] = *(const bf16x8*)(As + (qa * 4 + t) * 2048 + (((ks * 4 + fq) ^ fx16) << 4));
        };
        auto read_w = [&](const char* Ws, int qw, bf16x8 (&fw)[2][2]) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) fw[t][ks] = *(const bf16x8*)(Ws + (qw * 2 + t) * 2048 + (((ks * 4 + fq) ^ fx16) << 4));
        };
        auto mfma_head = [&]() {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this phase's reads are retired before the wave enters the barrier
            asm volatile("s_barrier" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
        };
        auto mfma_tail = [&]() {
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_barrier" ::: "memory");
        };
#define GB_QUADRANT(QA, QW, FW)                                                                                                   \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                               \
    _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                                  \
    _Pragma("unroll") for (int u = 0; u < 2; ++u)                                                                                  \
        acc16[(QW) * 2 + u][(QA) * 4 + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(FW[u][ks], fa[t][ks], acc16[(QW) * 2 + u][(QA) * 4 + t], 0, 0, 0);
        // STEADY: kt + 2 < nk, so every half-tile is of this output tile and the wait is vmcnt(6); otherwise one of the last two K-tiles
        auto ktile = [&](int kt, int b, auto steady) {
            constexpr bool STEADY = decltype(steady)::value;
            const bool own1 = STEADY || kt + 1 < nk, own2 = STEADY || kt + 2 < nk;
            const bool i1 = own1 || has_next;                            // K-tile kt + 1 of the stream exists (kt + 1 <= nk)
            const bool i2 = own2 || (kt + 2 == nk && has_next);          // K-tile kt + 2 of the stream exists
            const gb_i32x4 ra1 = own1 ? ra_c : ra_n, ra2 = own2 ? ra_c : ra_n, rw2 = own2 ? rw_c : rw_n;
            const int k1 = own1 ? kt + 1 : 0, k2 = own2 ? kt + 2 : 0;
            const char* As = smem + b * GB_STAGE + (wm * 128 + fr16) * 128;
            const char* Ws = smem + b * GB_STAGE + 32768 + (wn * 64 + fr16) * 128;
            // phase 1
            read_w(Ws, 0, fw0);
            __builtin_amdgcn_sched_barrier(0);
            read_a(As, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (i1) half(ra1, ra1, k1, b ^ 1, 1);
            mfma_head();
            GB_QUADRANT(0, 0, fw0)
            mfma_tail();
            // phase 2
            read_w(Ws, 1, fw1);
            __builtin_amdgcn_sched_barrier(0);
            if (i2) half(ra2, rw2, k2, b, 0);
            mfma_head();
            GB_QUADRANT(0, 1, fw1)
            mfma_tail();
            // phase 3
            read_a(As, 1);
            __builtin_amdgcn_sched_barrier(0);
            if (i2) half(ra2, rw2, k2, b, 2);
            mfma_head();
            GB_QUADRANT(1, 1, fw1)
            mfma_tail();
            // phase 4
            if (i2) half(ra2, rw2, k2, b, 3);
            if (STEADY || kt + 1 < nk) {                                 // K-tile kt + 1 is read from the next phase on
                if (i2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // last output tile of this workgroup, K-tile nk - 2 only
            }
            mfma_head();
            GB_QUADRANT(1, 0, fw0)
            mfma_tail();
        };
        int kt = 0;
        for (; kt + 4 <= nk; kt += 2) {                   // two K-tiles = eight phases per iteration
            ktile(kt, buf, std::true_type());
            ktile(kt + 1, buf ^ 1, std::true_type());
        }
        if (kt + 3 <= nk) {
            ktile(kt, buf, std::true_type());
            ++kt;
            buf ^= 1;
        }
        for (; kt < nk; ++kt) {                           // the last two K-tiles (one if nk == 1)
            ktile(kt, buf, std::false_type());
            buf ^= 1;
        }
        if (!late) asm volatile("s_barrier" ::: "memory");         // back in step for the epilogue
#undef GB_QUADRANT
        }

        // ---------------- epilogue: eight 32-row slabs through the stage that was just consumed ----------------
        // Slab s holds the 16 rows 16 s .. 16 s + 15 of BOTH wave rows (tile rows 16 s + r and 128 + 16 s + r at slab rows r and 16 + r), so
        // all eight waves scatter one 16-row fragment row each: ds_write_b128 is paced by the VGPR -> LDS transfer, which has one half per
        // SIMD pair, and the four waves of one wave row can sit on one pair (MI355X_MICROARCH.md, LDS).
        // Barriers: two per slab (scatter | read and store | next scatter), 16 per output tile, executed by every wave on every path;
        // the eight-phase loop's stagger was closed above and is reopened at the top of the next tile.  (Two alternating slabs with one
        // barrier each need a 256-float stride with an XOR swizzle; profiles/gemm_epilogue_ablation.txt: not built.)
        // WIDE (the host found every pointer and leading dimension of C / C2 / R / U 16-byte aligned and N % 8 == 0): a thread takes 8
        // consecutive columns of a row -- 32 lanes a 256-column row, a wave two rows per pass, two passes per slab -- with one 16-byte
        // store to C (fp32: two) and C2 and one 16-byte load of R / U; otherwise 4 columns, four passes, 8-byte accesses.
        constexpr int NV = WIDE ? 2 : 1;          // f32x4 column groups per thread and row
        constexpr int NP = WIDE ? 2 : 4;          // passes per slab
        constexpr int RP = 32 / NP;               // rows per pass
        float* Cs = (float*)(smem + (buf ^ 1) * GB_STAGE);
        const int n = cur.col0 + ec;
        float bias4[NV][4];
#pragma unroll
        for (int g = 0; g < NV; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) bias4[g][j] = 0.f;
        if (p.bias != nullptr && n < p.N) {        // WIDE: N % 8 == 0, so n < N covers all 8 columns
#pragma unroll
            for (int g = 0; g < NV; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) bias4[g][j] = bf2f(p.bias[n + 4 * g + j]);
        }
        auto row_of = [&](int slab, int pass) {   // output row of this thread in (slab, pass)
            const int sl = pass * RP + er;
            return cur.row0 + (sl >> 4) * 128 + slab * 16 + (sl & 15);
        };
        // second operand of the epilogue (residual / saved pre-activation): fetched two slabs ahead of its use
        constexpr bool HAS_AUX = EPI == EPI_GATED_RES || EPI == EPI_DGELU;
        u32x2 aux[3][NP][NV];
        auto aux_fetch = [&](int slab, u32x2 (&dst)[NP][NV]) {
#pragma unroll
            for (int pass = 0; pass < NP; ++pass) {
                const int m = row_of(slab, pass);
#pragma unroll
                for (int g = 0; g < NV; ++g) dst[pass][g] = (u32x2){0u, 0u};
                // (wave < 8 here and below is always true with 512 threads; removing it changes the generated code, so it stays)
                if (HAS_AUX && wave < 8 && m < p.M && n < p.N) {
                    if constexpr (WIDE) {
                        const u32x4 t = gemm_epilogue_aux_load8<EPI>(p, m, n);
                        dst[pass][0] = (u32x2){t[0], t[1]};
                        dst[pass][NV - 1] = (u32x2){t[2], t[3]};
                    } else {
                        dst[pass][0] = gemm_epilogue_aux_load<EPI>(p, m, n);
                    }
                }
            }
        };
        aux_fetch(0, aux[0]);
        aux_fetch(1, aux[1]);
        GateCtx gctx[NV];
        if (EPI == EPI_GATED_RES) {
#pragma unroll
            for (int g = 0; g < NV; ++g) gctx[g] = gate_ctx_load(p, cur.row0, GB_BM, n + 4 * g);
        }
#pragma unroll
        for (int slab = 0; slab < 8; ++slab) {
            if (wave < 8) {
#pragma unroll
                for (int tn = 0; tn < 4; ++tn)
                    *(f32x4*)(Cs + (wm * 16 + fr16) * GB_CS_LD + wn * 64 + tn * 16 + 4 * fq) = acc16[tn][slab];
            }
            gemm_lds_barrier();
            if (slab < 6) aux_fetch(slab + 2, aux[(slab + 2) % 3]);
#pragma unroll
            for (int pass = 0; pass < NP; ++pass) {
                const int m = row_of(slab, pass);
                if (wave < 8 && m < p.M && n < p.N) {
                    const float* src = Cs + (pass * RP + er) * GB_CS_LD + ec;
                    if constexpr (WIDE) {
                        // lanes 8-15 and 24-31 of a row read their two 16-byte chunks in the other order: with lane l at chunks 2 l and
                        // 2 l + 1, every lane group of ds_read_b128 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}) then covers 16 distinct
                        // 16-byte slots of the 256-byte bank row instead of 8 slots twice
                        const int par = (tid >> 3) & 1;
                        const f32x4 x0 = *(const f32x4*)(src + 4 * par), x1 = *(const f32x4*)(src + 4 * (1 - par));
                        const f32x4 v0 = par ? x1 : x0, v1 = par ? x0 : x1;
                        u32x2 c2a = (u32x2){0u, 0u}, c2b = (u32x2){0u, 0u};
                        const f32x4 r0 = gemm_epilogue_apply<EPI>(p, m, n, v0, bias4[0], aux[slab % 3][pass][0], EPI == EPI_GATED_RES ? &gctx[0] : nullptr, &c2a);
                        const f32x4 r1 = gemm_epilogue_apply<EPI>(p, m, n + 4, v1, bias4[NV - 1], aux[slab % 3][pass][NV - 1], EPI == EPI_GATED_RES ? &gctx[NV - 1] : nullptr, &c2b);
                        if (EPI == EPI_BIAS_GELU || (EPI == EPI_GATED_RES && p.C2 != nullptr))
                            *(u32x4*)(p.C2 + (size_t)m * p.ldc2 + n) = (u32x4){c2a[0], c2a[1], c2b[0], c2b[1]};
                        if (OUT_F32) {
                            float* c = (float*)p.C + (size_t)m * p.ldc + n;
                            *(f32x4*)c = r0;
                            *(f32x4*)(c + 4) = r1;
                        } else {
                            *(u32x4*)((bf16_t*)p.C + (size_t)m * p.ldc + n) = (u32x4){pack2(r0[0], r0[1]), pack2(r0[2], r0[3]), pack2(r1[0], r1[1]), pack2(r1[2], r1[3])};
                        }
                    } else {
                        const f32x4 v = *(const f32x4*)src;
                        gemm_epilogue_store_aux<EPI, OUT_F32>(p, m, n, v, bias4[0], aux[slab % 3][pass][0], EPI == EPI_GATED_RES ? &gctx[0] : nullptr);
                    }
                }
            }
            gemm_lds_barrier();
        }
        cur = nxt;
    }
}

// K-loop of gemm_tn_big_kernel: 0 = choose by shape, 1 = two-phase, 2 = eight-phase (tests and A/B timing; same results either way)
static int g_big_loop = 0;
extern "C" int vt_gemm_set_big_loop(int mode) {
    if (mode < 0 || mode > 2) return VT_ERR_BAD_SHAPE;
    g_big_loop = mode;
    return VT_OK;
}
static bool big_loop_phased(const GemmParams& p) {
    if (g_big_loop) return g_big_loop == 2;
    // profiles/gemm_big8_kbench.txt (both loops interleaved in one process): the eight-phase loop is ahead by more than the spread
    // from 8 K-tiles up at N = 640 and 5120 (and at every larger K-tile count measured; on one shape a 9 % lead is inside the
    // two-phase arm's own spread), and from 2 K-tiles up
    // at N = 2560 and 5120; it ties at 6 K-tiles with N = 640 and is behind at one K-tile (all prologue) and at N = 320 with 5
    const int nk = p.K / GB_BK;
    return nk >= 8 || (nk >= 2 && p.N >= 2560);
}

// Epilogue data movement, decided once per launch: 16-byte accesses (a thread takes 8 consecutive columns) where every matrix the epilogue
// touches allows them -- N % 8 == 0 and, for each bf16 matrix in use (C, C2, R, U), a 16-byte aligned base and ld % 8 == 0; an fp32 C
// is written 16 bytes at a time on both paths (ldc % 4 == 0 and a 16-byte base are validated by vt_gemm_bf16).  Otherwise the 8-byte path.
template <int EPI, bool F32>
static bool big_wide(const GemmParams& p) {
    auto ok = [](const void* q, int ld) { return ((((uintptr_t)q) & 15) == 0) && (ld % 8) == 0; };
    if (p.N % 8) return false;
    if (!F32 && !ok(p.C, p.ldc)) return false;
    if (EPI == EPI_BIAS_GELU && !ok(p.C2, p.ldc2)) return false;
    if (EPI == EPI_GATED_RES && (!ok(p.R, p.ldr) || (p.C2 != nullptr && !ok(p.C2, p.ldc2)))) return false;
    if (EPI == EPI_DGELU && !ok(p.U, p.ldu)) return false;
    return true;
}
// 1 / 0: the last launch of the 256x256 kernel took the 16-byte / the 8-byte epilogue path; -1 before the first (tests)
static int g_big_last_wide = -1;
extern "C" int vt_gemm_big_last_wide(void) { return g_big_last_wide; }

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
    const bool phased = big_loop_phased(p), wide = big_wide<EPI, F32>(p);
    g_big_last_wide = wide ? 1 : 0;
    if (phased && wide) hipLaunchKernelGGL((gemm_tn_big_kernel<EPI, F32, true, true>), dim3(grid), dim3(512), 0, st, p);
    else if (phased) hipLaunchKernelGGL((gemm_tn_big_kernel<EPI, F32, true, false>), dim3(grid), dim3(512), 0, st, p);
    else if (wide) hipLaunchKernelGGL((gemm_tn_big_kernel<EPI, F32, false, true>), dim3(grid), dim3(512), 0, st, p);
    else hipLaunchKernelGGL((gemm_tn_big_kernel<EPI, F32, false, false>), dim3(grid), dim3(512), 0, st, p);
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
