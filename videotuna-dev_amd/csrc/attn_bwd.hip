// Flash-attention backward (dQ, dK, dV), head_dim 64, bf16 in / fp32 accumulate, non-causal, gfx950.
//
// Autograd of the F.scaled_dot_product_attention call that the reference reaches through
// videotuna/models/cogvideo_hf/cogvideo_pl.py:865-871 (loss.backward() under PL).
// P is recomputed from Q, K and the forward's log2-domain LSE; the S x S matrices never touch HBM.
//
// This file holds the shipped kernel only.  The variants it was measured against (a body of four waves, a 32 x 32 S phase, other dQ
// shapes, timing-only ablations, the step timeline build) are recorded in exp/README.md, "Variants removed from attn_bwd.hip /
// attn_fwd.hip", with the commit at which their source can still be read and built.
//
// Workgroup.  8 waves (two per SIMD, <= 256 registers each, all in VGPRs) = 256 keys of one (batch, head); wave w owns keys
// [32w, 32w+32) and keeps dK^T and dV^T for them in 64 accumulator registers while the workgroup sweeps all queries in steps
// of 64 rows.  Two waves per SIMD so that one wave's exp2 / packing runs under the other's MFMAs.
//
// S phase (all eight waves, v_mfma_f32_16x16x32_bf16 on 16 x 16 tiles: same cycles per flop as 32x32x16, but the chip holds a
// higher clock on this shape under load).
//   * S = Q K^T and dP = dO V^T are computed with the KEY on the MFMA lane (K / V fragments live in registers for the whole
//     key block), so the fp32 tiles P and dS are, after bf16 packing, directly the B operands of dV^T += dO^T P and
//     dK^T += Q^T dS (A operands = transposed LDS reads of the dO / Q tiles, ds_read_b64_tr_b16).
//   * -lse2/c and -delta (delta = rowsum(dO*O)) are loaded as the initial accumulators of S'' and dP'.
//   * The issue order is software-pipelined and pinned by sched_barrier fences (FENCE): all operand reads of a segment are in
//     flight before its MFMAs, the next segment's reads are issued between the current segment's MFMAs.  Operand rings: PF_ROWN
//     Q / dO row operands, PF_TRN transposed dO / Q pairs.  (The compiler's own order issues every operand read right before
//     the MFMA that needs it: one LDS round trip exposed per k-step.)
//
// dQ phase (waves 0..3, v_mfma_f32_32x32x16_bf16).  Only dS crosses LDS: every wave writes its [32 keys][64 q] part of a
// [256][64] image; after one barrier waves 0..3 each compute one 32 x 32 tile of dQ (its (q-half, d-half)) over all 256 keys,
// DQ_RING k-steps of operands in flight, and add it to a fp32 dQ buffer with buffer_atomic_add_f32 (one register of a 32 x 32
// accumulator = two full 128-B row segments) -- or hand it to the next key block (chains, below) -- while waves 4..7 already
// start the next step (the dS image is double-buffered).
//
// LDS images, 128-B rows (145 KiB with the chain stage: one workgroup per CU).
//   * K block [256 keys][64 d] (B operand of dQ): 16-byte chunks XOR swz_f(row), conflict-free for the transposed reads.
//   * dS [256 keys][64 q] x 2 buffers: row = key, 8 bytes = four consecutive queries, 8-byte position = (query / 4) ^ swz4(key
//     row).  Swizzled at 8-byte granularity with four row bits so that the S phase's ds_write_b64 of a 16-lane group hit 16
//     distinct positions and the dQ phase's transposed reads stay conflict-free.
//   * Q and dO tiles [64 q][64 d] x 2 buffers: 16-byte chunks XOR (row & 6), conflict-free for the 16-row ds_read_b128
//     fragments AND the transposed reads of a 16 x 16 x 32 operand.
//   * row constants: 2 buffers x {-lse2/c, -delta} x 64 fp32.
//
// Staging.  Waves 4..7 stage the Q / dO tiles by LDS-DMA straight into the buffer the barrier before last freed (no staging
// registers, no ds_write of the tile; waves 0..3, which carry the dQ phase, stage nothing).  Everything a step fetches from
// memory is issued right after the previous step's barrier, before that step's dQ atomics.
//
// Scheduling.  The kernel is PERSISTENT: one workgroup per CU ("slot"), slot = (XCD, index inside the XCD) under round-robin
// dispatch, each slot sweeping the key blocks slot, slot + G, slot + 2G ...  Consecutive key blocks of a head therefore run
// side by side on one XCD and stream the same Q / dO tiles through its L2 at the same time.
//
// dQ hand-off chains.  fp32 atomics execute memory-side at ~340 G lane-adds/s for the whole chip whatever the locality or
// scope (tools/atomic_bench.hip); adding every key block's [S x 64] partial atomically is 7 ms of atomic-unit time per sample
// at S = 17776.  With chain_len = L > 1 (default 3), runs of up to L consecutive key blocks of a head on consecutive slots of
// one XCD form a chain in every generation: block j hands its running 64x64 fp32 dQ tile of every step to block j+1 through a
// ring of CH_R tiles in global memory (one ready and one consumed counter per wave, all counted in absolute steps so nothing is
// reset between generations), block j+1 uses the tile as the initial accumulator of its own dQ MFMAs, and only the last block
// of a chain issues atomics: ~L times fewer.  Chain neighbours that share an XCD (checked at run time through XCC_ID) keep the
// ring in that XCD's L2: plain stores, agent-scope loads; any other pair goes through memory with write-through stores and
// system-scope loads.  Tiles arrive by LDS-DMA into a stage of their own; counter loads and tile loads are issued a full step
// before they are needed.  Every wait is bounded (CH_SPIN_LIMIT) and gives up with an error word instead of hanging.
// The roles are template parameters (ROLE: bit 0 = has a chain predecessor and takes its running dQ tiles, bit 1 = has a
// successor and hands its tiles on instead of adding them atomically): with runtime flags the compiler's register allocation
// made the atomic-only path of the same binary 26 % slower.  vt_attn_bwd_set_chain(1, ..) gives the atomics-only launch.
#include "common.h"
#include <cstdlib>

// Build hooks.  VT_SUFFIX: the same source compiled a second time under another symbol suffix (libvt355_test.so: _tmo with
// CH_SPIN_LIMIT=0; tools/build_exp.sh: A/B timing of two builds in ONE process).  The shipped build defines none of them.
#ifndef VT_SUFFIX
#define VT_SUFFIX
#endif
#ifndef VT_CLK
#define VT_CLK 0      // 1 = diagnostic build (tools/build_w4.sh): the in-kernel clock of one key block's loop, d(s_memtime) / d(s_memrealtime) x 100 MHz
#endif                // (MI355X_MICROARCH.md, DVFS item 6); two probes per key block, the loop itself is untouched
#define VT_CAT_(a, b) a##b
#define VT_CAT(a, b) VT_CAT_(a, b)
#define BWD_KERNEL VT_CAT(attn_bwd_hd64_kernel, VT_SUFFIX)
#define BWD_BODY VT_CAT(attn_bwd_body, VT_SUFFIX)
#define DELTA_KERNEL VT_CAT(attn_bwd_delta_kernel, VT_SUFFIX)
#define BWD_ENTRY VT_CAT(vt_attn_bwd_hd64, VT_SUFFIX)

#define BWD_THREADS 512
#define FENCE() __builtin_amdgcn_sched_barrier(0)
#define DQ_RING 2     // k-steps of dQ operands in flight
#define PF_TRN 4      // transposed-operand pairs of a dV / dK segment in flight before its first MFMA
#define PF_ROWN 2     // depth of the ring of Q / dO row operands

struct AttnBwdParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* v;
    const bf16_t* dout;
    const float* lse2;    // [B,H,S]
    const float* delta;   // [B,H,S]
    float* dq;            // fp32 accumulation buffer, pre-zeroed
    bf16_t* dk;
    bf16_t* dv;
    int S, H, B;
    long long q_rs, k_rs, v_rs, do_rs, dq_rs, dk_rs, dv_rs;
    long long q_bs, k_bs, v_bs, do_bs, dq_bs, dk_bs, dv_bs;
    float scale, scale_log2;
    int chain_len;        // 1: one workgroup per key block, every one adds its dQ partial atomically; > 1: persistent + chains
    int* chain_ctr;       // [8] = error word                                    (zeroed by the host before the launch)
                          // [16] = STICKY time-out count: never cleared by the library (the caller zeroes it once and reads it when it likes)
    int* chain_flags;     // [slots][16]: ready[8 waves] | consumed[8 waves], in absolute steps (zeroed before the launch)
    int* chain_xcc;       // [slots] 1 + XCC_ID of the workgroup that runs the slot (0 = not started yet; zeroed before the launch)
    float* chain_tiles;   // [slots][CH_R][4 waves][4][64 lanes][4] fp32
};

// LDS map (bytes)
#define KIMG 0                   // K block image, 32 KiB
#define DSIMG 32768              // dS image, 2 x 32 KiB
#define QTILE 98304              // 2 x (Q tile 8 KiB | dO tile 8 KiB)
#define LSEOFF 131072            // 2 x (64 x -lse2/c | 64 x -delta) fp32
#define BWD_LDS 132096
#define CH_STAGE_BYTES 16384     // incoming dQ tile of the chain predecessor: 4 waves x 4 KiB, a separate LDS object so
                                 // that the compiler does not order every ds_read of a step behind the DMA that fills it
#define CH_R 4                   // ring depth (tiles of 64 q x 64 d fp32 = 16 KiB)
#define CH_HYST 1                // tiles of slack a consumer rebuilds whenever it had to wait for its producer
#ifndef CH_SPIN_LIMIT
#define CH_SPIN_LIMIT (1 << 19)   // polls (~1 us each) before a wait gives up (-DCH_SPIN_LIMIT=0: the forced-time-out test build, libvt355_test.so)
#endif
#define CH_AUX 17                // counters: sc0 | sc1 = system scope -- stores write through, loads bypass the caches

typedef __attribute__((ext_vector_type(8))) short short8v;
typedef int i32x4w __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int swz_f(int row) {
    return (((row >> 1) & 1) << 2) | (((row >> 3) & 1) << 1) | ((row >> 2) & 1);
}
__device__ __forceinline__ int swz4(int row) { return (((row >> 1) & 1) << 3) | (((row >> 3) & 1) << 2) | (((row >> 2) & 1) << 1) | (row & 1); }
__device__ __forceinline__ int swz_off(int row, int chunk) { return row * 128 + ((chunk ^ swz_f(row)) << 4); }

// two transposed 8-byte reads (rows +0..3 and rows +sec_stride) -> one 8 x bf16 MFMA operand
__device__ __forceinline__ bf16x8 tr_pair(const char* p0, const char* p1) {
    short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(p0));
    short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(p1));
    short8v v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v8);
}

// One key block (item id) on one slot: K / V fragments, the sweep over all query steps, the dK / dV epilogue.
template <bool RAGGED, bool PRESCALED, int ROLE>
__device__ __forceinline__ void BWD_BODY(const AttnBwdParams& p, char* smem, char* stage, const int id, const int slot,
                                         const int cons_end, const int base, const bool l2_prev, const bool l2_next,
                                         bool& dead) {
    constexpr bool has_prod = (ROLE & 1) != 0, has_cons = (ROLE & 2) != 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);          // 0..7
    const int r = lane & 31, h = lane >> 5, g = lane >> 4, ql = (lane & 15) >> 2, pl = lane & 3;
    const int nkb = (p.S + 255) / 256;
    const int kblk = id % nkb, bh = id / nkb;
    const int head = bh % p.H, b = bh / p.H;
    const int key0 = kblk * 256;

    const bf16_t* qb = p.q + (size_t)b * p.q_bs + head * 64;
    const bf16_t* kb_ = p.k + (size_t)b * p.k_bs + head * 64;
    const bf16_t* vb = p.v + (size_t)b * p.v_bs + head * 64;
    const bf16_t* dob = p.dout + (size_t)b * p.do_bs + head * 64;
    // rq and rdo are unused (the Q / dO tiles go through the raw descriptor words rq_w / rdo_w below).  They stay because the compiler orders
    // the kernel's scalar prologue differently without them, and this file's machine code changes only together with a measurement.
    __amdgpu_buffer_rsrc_t rq = make_rsrc(qb, (unsigned)((long long)(p.S - 1) * p.q_rs * 2 + 128));
    __amdgpu_buffer_rsrc_t rk = make_rsrc(kb_, (unsigned)((long long)(p.S - 1) * p.k_rs * 2 + 128));
    __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, (unsigned)((long long)(p.S - 1) * p.v_rs * 2 + 128));
    __amdgpu_buffer_rsrc_t rdo = make_rsrc(dob, (unsigned)((long long)(p.S - 1) * p.do_rs * 2 + 128));
    // dQ accumulation buffer of this (batch, head): rows >= S are out of range -> the atomics are dropped by hardware
    __amdgpu_buffer_rsrc_t rdq = make_rsrc(p.dq + (size_t)b * p.dq_bs + head * 64, (unsigned)((long long)(p.S - 1) * p.dq_rs * 4 + 256));
    const float* lse_b = p.lse2 + (size_t)bh * p.S;
    const float* dl_b = p.delta + (size_t)bh * p.S;

    // ---- K block image (B operand of dQ): 256 keys x 8 chunks, 4 per thread ----
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 512 * j;
        const int key = i >> 3, c = i & 7;
        u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, (int)((key0 + key) * p.k_rs * 2) + c * 16, 0, 0));
        *(u32x4*)(smem + KIMG + swz_off(key, c)) = v;
    }
    // ---- K / V fragments of this wave's 32 keys, resident for the whole key block ----
    // B operands of S = Q K^T and dP = dO V^T on 16 x 16 x 32 tiles: lane (g, c) holds K[key 16 kt + c][d = 32 s + 8 g .. + 7]
    const int c15 = lane & 15;
    bf16x8 kf16[2][2], vf16[2][2];
    float kmask16[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + 32 * w + 16 * kt + c15;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            kf16[kt][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rk, (int)(key * p.k_rs * 2) + (32 * s + 8 * g) * 2, 0, 0));
            vf16[kt][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv, (int)(key * p.v_rs * 2) + (32 * s + 8 * g) * 2, 0, 0));
        }
        kmask16[kt] = (RAGGED && key >= p.S) ? -1.0e30f : 0.f;
    }

    // ---- per-lane LDS offsets ----
    // Q / dO tile image, swizzle row & 6.  Row fragment (q-tile, k-step s): lane (g, c) reads row c, chunk 4 s + g; a q-tile is 2048 B further.
    // Transposed fragment (d-tile dt) of a 32-query k-step: group g takes the 4-row blocks at rows 4 g and 16 + 4 g (k-slot j of the group =
    // query 4 g + j for j < 4, 16 + 4 g + j - 4 above: the order in which two stacked accumulator tiles supply P / dS), columns 16 dt .. + 15
    int rowrd16[2];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) rowrd16[s_] = c15 * 128 + (((4 * s_ + g) ^ (c15 & 6)) << 4);
    int trA16[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) trA16[dt] = (4 * g + ql) * 128 + (((2 * dt + (pl >> 1)) ^ ((4 * g + ql) & 6)) << 4) + (pl & 1) * 8;
    const int qs_w = w & 1, dt_w = (w >> 1) & 1;          // dQ phase (waves 0..3): (q-half, d-half) of the 64x64 tile
    int trQA[2], trQB[2];                                 // transposed reads of the dS image (A, 8-byte swizzle) and the K image (B), [sec]
#pragma unroll
    for (int sec = 0; sec < 2; ++sec) {
        const int fx = ((ql >> 1) << 2) | (h << 1) | sec;
        const int row = (8 * h + ql + 4 * sec) * 128;
        trQA[sec] = row + (((2 * (4 * qs_w + 2 * (g & 1) + (pl >> 1)) + (pl & 1)) ^ swz4(8 * h + ql + 4 * sec)) << 3);
        trQB[sec] = row + (((4 * dt_w + 2 * (g & 1) + (pl >> 1)) ^ fx) << 4) + (pl & 1) * 8;
    }
    // dQ atomics: byte offset of (row 32 qs_w + 4 h, column 32 dt_w + r) inside a 64-row step; register i adds ((i & 3) + 8 (i >> 2)) rows
    const int dq_voff = (int)((32 * qs_w + 4 * h) * p.dq_rs * 4) + (32 * dt_w + r) * 4;
    const int dq_rowb = (int)(p.dq_rs * 4);

    // ---- dQ hand-off chain (see the header comment); only the dQ waves (w < 4) take part ----
    const int wu = w & 3;             // waves 0..3 own 4 KiB each (one 32x32 fp32 tile)
    const bool dqw = w < 4;
    constexpr int NT = 4, WTILE = 4096;
    __amdgpu_buffer_rsrc_t rfl = make_rsrc(p.chain_flags, (unsigned)gridDim.x * 64u);
    __amdgpu_buffer_rsrc_t rt_mine = make_rsrc(p.chain_tiles + (size_t)slot * (CH_R * 4096), CH_R * 16384);
    const int fl_ready_me = (slot * 16 + wu) * 4, fl_cons_me = (slot * 16 + 8 + wu) * 4;
    const int fl_ready_prod = ((slot - 1) * 16 + wu) * 4, fl_cons_next = ((slot + 1) * 16 + 8 + wu) * 4;
    const int tile_voff = wu * WTILE + lane * 16;
    const unsigned stage_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)stage;
    i32x4w rt_prod_w;                                      // the predecessor's ring as raw descriptor words (inline asm operand)
    {
        const unsigned long long a = (unsigned long long)(p.chain_tiles + (size_t)(has_prod ? slot - 1 : slot) * (CH_R * 4096));
        rt_prod_w = (i32x4w){(int)(unsigned)a, (int)((a >> 32) & 0xffffu), CH_R * 16384, 0x00020000};
    }
    // counter loads stay in a VGPR until the end-of-step barrier has waited for them anyway; only then are they moved to
    // an SGPR (a readfirstlane anywhere else makes the compiler drain every outstanding memory operation on the spot)
    auto fl_load = [&](int off) -> int { return (int)__builtin_amdgcn_raw_buffer_load_b32(rfl, off, 0, CH_AUX); };
    int spins_r = 0, spins_c = 0;      // diagnostics: polls spent waiting for the predecessor / the successor
    auto fl_wait = [&](int off, int need, int have, int& spins) {
        int it = 0;
        while (have < need && !dead) {
            ++spins;
            __builtin_amdgcn_s_sleep(4);
            have = __builtin_amdgcn_readfirstlane(fl_load(off));
            if (++it > CH_SPIN_LIMIT) { dead = true; p.chain_ctr[8] = 1; atomicAdd(p.chain_ctr + 16, 1); }
        }
    };

    // ---- staging of the Q / dO tiles (64 rows x 8 chunks each) and of the row constants, by waves 4..7 ----
    // row constants in the form the MFMA accumulators want:  S'' = Q K^T - lse2/c  and  dP' = dO V^T - delta;
    // threads t and t + 128 stage the same value (keeps the loop body free of divergent branches)
    const int stat_i = tid & 63;
    const bool stat_is_lse = (tid & 64) == 0;
    const float* stat_src = stat_is_lse ? lse_b : dl_b;
    const float stat_mul = stat_is_lse ? (PRESCALED ? -1.0f : -1.0f / p.scale_log2) : -1.0f;
    const int stat_lds = LSEOFF + (tid & 127) * 4;
    float gstat = 0.f;
    i32x4w rq_w, rdo_w;
    {
        const unsigned long long aq = (unsigned long long)qb, ad = (unsigned long long)dob;
        rq_w = (i32x4w){(int)(unsigned)aq, (int)((aq >> 32) & 0xffffu), (int)(unsigned)((long long)(p.S - 1) * p.q_rs * 2 + 128), 0x00020000};
        rdo_w = (i32x4w){(int)(unsigned)ad, (int)((ad >> 32) & 0xffffu), (int)(unsigned)((long long)(p.S - 1) * p.do_rs * 2 + 128), 0x00020000};
    }
    // wave 4 + wb owns rows [16 wb, 16 wb + 16) of both tiles: two 1-KiB pieces each (8 rows x 8 chunks; lane i fills LDS slot i of the piece,
    // i.e. row i >> 3, position i & 7, which the images' swizzle assigns to chunk (i & 7) ^ f(row): the swizzle is applied to the SOURCE)
    int dma_vq[2], dma_vdo[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = 16 * (w & 3) + 8 * j + (lane >> 3);
        const int c = (lane & 7) ^ (row & 6);
        dma_vq[j] = (int)(row * p.q_rs * 2) + c * 16;
        dma_vdo[j] = (int)(row * p.do_rs * 2) + c * 16;
    }
    const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    // tile t -> buffer t & 1, free since the barrier of step t - 2: Q pieces, then dO pieces + row constants.  Inline asm, so that the compiler does
    // not order the step's LDS reads behind them (see prefetch below); lstore's vmcnt(0) retires them before the barrier that publishes the tile
    auto gload_q = [&](int t) {
        if (!dqw) {
            const int sq = (int)((long long)t * 64 * p.q_rs * 2);
            const unsigned dst = smem_lds + QTILE + (t & 1) * 16384 + (16 * (w & 3)) * 128;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                             :: "s"(dst + j * 1024), "v"(dma_vq[j]), "s"(rq_w), "s"(sq) : "memory");
        }
    };
    auto gload_do = [&](int t) {
        if (!dqw) {
            const int q0 = t * 64;
            const int sdo = (int)((long long)q0 * p.do_rs * 2);
            const unsigned dst = smem_lds + QTILE + (t & 1) * 16384 + (16 * (w & 3)) * 128;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                             :: "s"(dst + 8192 + j * 1024), "v"(dma_vdo[j]), "s"(rdo_w), "s"(sdo) : "memory");
            int qi = q0 + stat_i;
            const bool ok = qi < p.S;
            qi = ok ? qi : p.S - 1;
            const float v = stat_src[qi] * stat_mul;
            gstat = ok ? v : 0.f;
        }
    };
    auto gload = [&](int t) { gload_q(t); gload_do(t); };
    auto lstore = [&](int buf) {                  // before the barrier that publishes the tile
        if (!dqw) {
            *(float*)(smem + stat_lds + buf * 512) = gstat;     // threads t and t + 128 write the same value
            __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0): the compiler does not know about the DMA pieces
        }
    };
    f32x4 dk16[4][2], dv16[4][2];         // [d-tile][key-tile]: dK^T / dV^T, lane (g, c) holds d = 16 dt + 4 g + i of key 16 kt + c
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 2; ++i) { dk16[c][i] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv16[c][i] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    const float sc = p.scale_log2;
    const int nsteps = (p.S + 63) / 64;
    int pf_ready = 0;
    if (has_prod && dqw) pf_ready = fl_load(fl_ready_prod);
    gload(0);
    lstore(0);
    __syncthreads();
    int s_ready = (has_prod && dqw) ? __builtin_amdgcn_readfirstlane(pf_ready) : 0;
    // everything step t1 fetches from memory: the chain predecessor's dQ tile t1 (LDS-DMA into the stage), the counter for t1 + 1, the
    // Q / dO tile t1 + 1.  Issued right after the barrier of step t1 - 1, BEFORE that step's dQ atomics -- vector-memory instructions issue
    // in order, and the loads of a wave that has just pushed 16 atomics (16 B/clk per CU) waited ~500-700 cycles for their turn
    // (profiles/r02_attn_bwd_stamps_before_L2_consumer.txt, "loads issued")
    auto prefetch = [&](int t1) {
        if (has_prod && dqw && t1 < nsteps) {
            // predecessor's tile t1 must be public.  The counter at hand is a step old, and a consumer that passes with no margin is stopped
            // again by the next hiccup of its producer, each time for a full uncached round trip that its own successors then inherit: when
            // it does have to wait, it waits until the producer is CH_HYST tiles ahead, and then coasts on that slack.
            if (s_ready < base + t1 + 1)
                fl_wait(fl_ready_prod, base + (t1 + 1 + CH_HYST < nsteps ? t1 + 1 + CH_HYST : nsteps), s_ready, spins_r);
            // LDS-DMA of the 4 x 1 KiB of this wave.  Issued through inline asm: the compiler orders every later LDS access of the step behind
            // an LDS-DMA it knows about (s_waitcnt vmcnt(0) a few instructions into the step).  Safe because the wait in front of the barrier
            // below covers them (vector memory retires in order) and the stage is read only behind that barrier.
            // Cache policy: the predecessor shares this XCD's L2 (l2_prev: its plain stores are there) -> agent-scope load, L1 bypassed;
            // otherwise system scope against its write-through stores
            if (l2_prev) {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen sc1 lds"
                                 :: "s"(stage_lds + wu * WTILE + j * 1024), "v"(tile_voff + j * 1024), "s"(rt_prod_w),
                                    "s"(((base + t1) % CH_R) * 16384) : "memory");
            } else {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen sc0 sc1 lds"
                                 :: "s"(stage_lds + wu * WTILE + j * 1024), "v"(tile_voff + j * 1024), "s"(rt_prod_w),
                                    "s"(((base + t1) % CH_R) * 16384) : "memory");
            }
            pf_ready = fl_load(fl_ready_prod);
        }
        gload(t1 + 1);                                 // past the end: bounds-checked loads return zeros
    };
    prefetch(0);
    // S'' / dP' accumulators, 16 x 16 tiles: s16[q-half][q-tile][key-tile] (lane (g, c): query 16 qt + 4 g + i, key 16 kt + c), and the ring of
    // PF_ROWN Q / dO row operands; item n of a q-half = (k-step n >> 1, q-tile n & 1), ring slot n & 1
    f32x4 s16[2][2][2], p16[2][2][2];
    bf16x8 qa16[PF_ROWN], doa16[PF_ROWN];
    // the row constants go straight into the accumulators of BOTH key tiles.  (Kept in registers of their own as the C operand of the first
    // k-step's MFMAs -- one LDS value for two tiles, no spill -- measured slower: 6.94-7.15 vs 6.66-6.77 ms at B=1, same box.)
    auto rd_init16 = [&](const float* lsel_, int qs, int qt, int which) {    // which: 0 = S'' (-lse2 / c [+ key mask]), 1 = dP' (-delta)
        const f32x4 a = *(const f32x4*)(lsel_ + 64 * which + 32 * qs + 16 * qt + 4 * g);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            if (which == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) s16[qs][qt][kt][e] = RAGGED ? a[e] + kmask16[kt] : a[e];
            } else p16[qs][qt][kt] = a;
        }
    };
    auto rd_rows16 = [&](const char* qimg_, const char* doimg_, int qs, int n) {
        const int off = qs * 4096 + (n & 1) * 2048 + rowrd16[n >> 1];
        qa16[n & 1] = *(const bf16x8*)(qimg_ + off);
        doa16[n & 1] = *(const bf16x8*)(doimg_ + off);
    };
    auto rd_first = [&](int bufn) {
        const char* qn = smem + QTILE + bufn * 16384;
        const float* ln = (const float*)(smem + LSEOFF + bufn * 512);
        rd_init16(ln, 0, 0, 0); rd_init16(ln, 0, 0, 1); rd_init16(ln, 0, 1, 0); rd_init16(ln, 0, 1, 1);
        rd_rows16(qn, qn + 8192, 0, 0); rd_rows16(qn, qn + 8192, 0, 1);
        FENCE();
    };
    for (int t = 0; t < nsteps; ++t) {
        const int buf = t & 1;
        int pf_cons = 0;
        if (has_cons && dqw) pf_cons = fl_load(fl_cons_next);
        const char* qimg = smem + QTILE + buf * 16384;
        const char* doimg = qimg + 8192;
        const float* lsel = (const float*)(smem + LSEOFF + buf * 512);
        char* dsimg = smem + DSIMG + buf * 32768;

        // ---- S phase (all waves) ----
        {
            // per q-half a segment of 16 S'' / dP' MFMAs (four items of (k-step, q-tile) x (key-tile, S | dP)), the exp2 block (P = exp2(c S''),
            // dS = P * dP', both packed to bf16 pairs), a segment of 16 dV / dK MFMAs (four d-tiles x (key-tile, dV | dK)); every segment's
            // operand reads are issued during the one before, pinned by the fences
            bf16x8 doT16[PF_TRN], qT16[PF_TRN];       // transposed dO / Q operands of the four d-tiles
            unsigned pw16[2][2][2], dw16[2][2][2];
            auto rd_tr16 = [&](int qs, int dt) {
                const int ro = qs * 4096 + trA16[dt];
                doT16[dt] = tr_pair(doimg + ro, doimg + ro + 2048);
                qT16[dt] = tr_pair(qimg + ro, qimg + ro + 2048);
            };
            rd_first(buf);
            FENCE();
#pragma unroll
            for (int qs = 0; qs < 2; ++qs) {
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int ks = n >> 1, qt = n & 1;
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt) {
                        s16[qs][qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa16[n & 1], kf16[kt][ks], s16[qs][qt][kt], 0, 0, 0);
                        p16[qs][qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(doa16[n & 1], vf16[kt][ks], p16[qs][qt][kt], 0, 0, 0);
                    }
                    if (n + 2 < 4) rd_rows16(qimg, doimg, qs, n + 2);        // into the slot these MFMAs just read
                    if (n >= 2) rd_tr16(qs, n - 2);
                    FENCE();
                }
                rd_tr16(qs, 2); rd_tr16(qs, 3);                               // land under the exp2 block
                FENCE();
#pragma unroll
                for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const float p0 = __builtin_amdgcn_exp2f(PRESCALED ? s16[qs][qt][kt][2 * i] : s16[qs][qt][kt][2 * i] * sc);
                            const float p1 = __builtin_amdgcn_exp2f(PRESCALED ? s16[qs][qt][kt][2 * i + 1] : s16[qs][qt][kt][2 * i + 1] * sc);
                            pw16[qt][kt][i] = pack2(p0, p1);
                            dw16[qt][kt][i] = pack2(p0 * p16[qs][qt][kt][2 * i], p1 * p16[qs][qt][kt][2 * i + 1]);
                        }
                FENCE();
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt) {
                        const u32x4 pb4 = {pw16[0][kt][0], pw16[0][kt][1], pw16[1][kt][0], pw16[1][kt][1]};
                        const u32x4 db4 = {dw16[0][kt][0], dw16[0][kt][1], dw16[1][kt][0], dw16[1][kt][1]};
                        dv16[dt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(doT16[dt], __builtin_bit_cast(bf16x8, pb4), dv16[dt][kt], 0, 0, 0);
                        dk16[dt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT16[dt], __builtin_bit_cast(bf16x8, db4), dk16[dt][kt], 0, 0, 0);
                    }
                    if (qs == 0) {                      // the other q-half's first reads ride under these MFMAs
                        rd_init16(lsel, 1, dt >> 1, dt & 1);
                        if (dt >= 2) rd_rows16(qimg, doimg, 1, dt - 2);
                    }
                    FENCE();
                }
                // dS image (row = key, 8 bytes = four consecutive queries): tile (qt, kt) -> row 32 w + 16 kt + c,
                // queries 32 qs + 16 qt + 4 g + (0..3) = 8-byte unit 8 qs + 4 qt + g
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    const int krow = 32 * w + 16 * kt + c15;
                    char* drow = dsimg + krow * 128;
                    const int fk = swz4(krow);
#pragma unroll
                    for (int qt = 0; qt < 2; ++qt) {
                        const u32x2 two = {dw16[qt][kt][0], dw16[qt][kt][1]};
                        *(u32x2*)(drow + (((8 * qs + 4 * qt + g) ^ fk) << 3)) = two;          // 8-byte position = (query / 4) ^ swz4(key row)
                    }
                }
                FENCE();
            }
        }
        lstore(buf ^ 1);
        // the predecessor's tile t (LDS-DMA the compiler does not know about) must have landed before the barrier: it was issued before
        // this wave's previous 16 atomics (+ 1 counter store), which may stay in flight -- vector memory completes in order
        // (step 0 has no atomics behind the DMA yet: wait for everything)
        if (has_prod && dqw) {
            if (has_cons || t == 0) __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0)
            else __builtin_amdgcn_s_waitcnt(0x4F70);                                      // vmcnt(16)
        }
        __syncthreads();

        // ---- dQ phase: one tile (32 q x 32 d) over all 256 keys on waves 0..3, then the hand-off or the atomics; waves 4..7 go on with the next step ----
        if (!dqw) prefetch(t + 1);
        if (dqw) {
            if (has_prod) s_ready = __builtin_amdgcn_readfirstlane(pf_ready);      // the barrier drained the memory pipeline
            const int s_cons = has_cons ? __builtin_amdgcn_readfirstlane(pf_cons) : 0;
            f32x16 dq_acc;
            if (has_prod) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 v = *(const f32x4*)(stage + wu * 4096 + j * 1024 + lane * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dq_acc[4 * j + e] = v[e];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) dq_acc[i] = 0.f;
            }
            if (has_prod) __builtin_amdgcn_s_waitcnt(0xc07f);                             // the stage has been read: the next DMA may land
            if (has_cons && t > 0) {
                __builtin_amdgcn_s_waitcnt(0x0F70);                                       // vmcnt(0): tile t-1 is a step old
                __builtin_amdgcn_raw_buffer_store_b32((unsigned)(base + t), rfl, fl_ready_me, 0, CH_AUX);
            }
            prefetch(t + 1);
            {
                bf16x8 fa[DQ_RING], fb[DQ_RING];              // DQ_RING k-steps of operands in flight (the compiler's order: one, waited for at once)
                auto rd_dq = [&](int s3) {
                    fa[s3 % DQ_RING] = tr_pair(dsimg + s3 * 2048 + trQA[0], dsimg + s3 * 2048 + trQA[1]);
                    fb[s3 % DQ_RING] = tr_pair(smem + KIMG + s3 * 2048 + trQB[0], smem + KIMG + s3 * 2048 + trQB[1]);
                };
#pragma unroll
                for (int s3 = 0; s3 < DQ_RING; ++s3) rd_dq(s3);
                FENCE();
#pragma unroll
                for (int s3 = 0; s3 < 16; ++s3) {
                    dq_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s3 % DQ_RING], fb[s3 % DQ_RING], dq_acc, 0, 0, 0);
                    if (s3 + DQ_RING < 16) rd_dq(s3 + DQ_RING);
                    FENCE();
                }
            }
            if (has_cons) {       // hand-off: wait for a free ring slot, store the tile (published a step later, above)
                const int a = base + t;
                int need = a - CH_R + 1;
                if (t < CH_R && need > cons_end) need = cons_end;
                if (need > 0) fl_wait(fl_cons_next, need, s_cons, spins_c);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 v = {dq_acc[4 * j], dq_acc[4 * j + 1], dq_acc[4 * j + 2], dq_acc[4 * j + 3]};
                    if (l2_next)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rt_mine, tile_voff + j * 1024, (a % CH_R) * 16384, 0);
                    else
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rt_mine, tile_voff + j * 1024, (a % CH_R) * 16384, CH_AUX);
                }
            } else {              // end of a chain: add the tile to dQ
                const int soff = (int)((long long)t * 64 * p.dq_rs * 4);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(dq_acc[i] * p.scale, rdq, dq_voff,
                                                                    soff + ((i & 3) + 8 * (i >> 2)) * dq_rowb, 0);
            }
            if (has_prod) __builtin_amdgcn_raw_buffer_store_b32((unsigned)(base + t + 1), rfl, fl_cons_me, 0, CH_AUX);
        }
    }
    if (dqw) {
        if ((has_prod || has_cons) && lane == 0 && (spins_r | spins_c)) {
            if (spins_r) atomicAdd(p.chain_ctr + 9, spins_r);
            if (spins_c) atomicAdd(p.chain_ctr + 10, spins_c);
        }
        if (has_cons) {     // the last tile
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __builtin_amdgcn_raw_buffer_store_b32((unsigned)(base + nsteps), rfl, fl_ready_me, 0, CH_AUX);
        }
    }

    // ---- epilogue: dK^T, dV^T accumulators -> dk[key][d], dv[key][d] ----
    const float dk_mul = PRESCALED ? 0.6931471805599453f : p.scale;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + 32 * w + 16 * kt + c15;
        if (key < p.S) {
            bf16_t* dkp = p.dk + (size_t)b * p.dk_bs + (size_t)key * p.dk_rs + head * 64;
            bf16_t* dvp = p.dv + (size_t)b * p.dv_bs + (size_t)key * p.dv_rs + head * 64;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                u32x2 a, c;
                a[0] = pack2(dk16[dt][kt][0] * dk_mul, dk16[dt][kt][1] * dk_mul);
                a[1] = pack2(dk16[dt][kt][2] * dk_mul, dk16[dt][kt][3] * dk_mul);
                c[0] = pack2(dv16[dt][kt][0], dv16[dt][kt][1]);
                c[1] = pack2(dv16[dt][kt][2], dv16[dt][kt][3]);
                *(u32x2*)(dkp + 16 * dt + 4 * g) = a;
                *(u32x2*)(dvp + 16 * dt + 4 * g) = c;
            }
        }
    }
}


#if VT_CLK
__device__ unsigned VT_CAT(vt_bwd_clk, VT_SUFFIX)[4];
extern "C" int VT_CAT(vt_attn_bwd_clk, VT_SUFFIX)(unsigned* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(VT_CAT(vt_bwd_clk, VT_SUFFIX)), 4 * sizeof(unsigned)) == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
#endif
template <bool PRESCALED>
__global__ __launch_bounds__(BWD_THREADS, 1) void BWD_KERNEL(AttnBwdParams p) {
    __shared__ __attribute__((aligned(16))) char smem[BWD_LDS];
    __shared__ __attribute__((aligned(16))) char stage[CH_STAGE_BYTES];
    const int nkb = (p.S + 255) / 256;
    const int nitems = nkb * p.H * p.B, nsteps = (p.S + 63) / 64;
    const int L = p.chain_len;
    // persistent grid: slot = (XCD, index inside the XCD) under round-robin dispatch; consecutive slots share an XCD, and
    // a slot sweeps the key blocks slot, slot + G, ...  (consecutive key blocks of a head run side by side on one XCD and
    // stream the same Q / dO tiles through its L2 at the same time)
    const int spx = gridDim.x >> 3;
    const int slot = (int)(blockIdx.x & 7) * spx + (int)(blockIdx.x >> 3);
    bool dead = false;
    int cons_end = 0;
    int gen = 0;
    bool l2_prev = false, l2_next = false;
    if (L > 1) {
        // Which neighbours share this workgroup's XCD (and therefore its L2)?  Every slot publishes 1 + XCC_ID once; chain
        // neighbours on the same XCD exchange their tiles through the L2 (plain stores, agent-scope loads), any other
        // pair through memory.  Round-robin dispatch puts consecutive slots on one XCD, but nothing here relies on it.
        int xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc = (xcc & 15) + 1;
        __amdgpu_buffer_rsrc_t rx = make_rsrc(p.chain_xcc, (unsigned)gridDim.x * 4u);
        if (threadIdx.x == 0) __builtin_amdgcn_raw_buffer_store_b32((unsigned)xcc, rx, slot * 4, 0, CH_AUX);
        const int j = slot % spx;
        auto peer = [&](int s2) -> int {
            int v = 0, it = 0;
            while (v == 0 && it++ < (1 << 16)) {
                v = __builtin_amdgcn_readfirstlane((int)__builtin_amdgcn_raw_buffer_load_b32(rx, s2 * 4, 0, CH_AUX));
                if (v == 0) __builtin_amdgcn_s_sleep(8);
            }
            return v;      // 0 after ~0.1 s: the neighbour never started -> treated as "another XCD"
        };
        if ((j % L) != 0) {
            l2_prev = peer(slot - 1) == xcc;
            if (threadIdx.x == 0) atomicAdd(p.chain_ctr + (l2_prev ? 11 : 12), 1);     // diagnostics: links through L2 / memory
        }
        if ((j % L) != L - 1 && j != spx - 1 && slot + 1 < (int)gridDim.x) l2_next = peer(slot + 1) == xcc;
    }
    for (int item = slot; item < nitems; item += gridDim.x, ++gen) {
        const int kblk = item % nkb;
        bool has_prod = false, has_cons = false;
        if (L > 1) {
            const int j = slot % spx;         // chains: same head, same XCD, at most L long, aligned to multiples of L
            has_prod = (j % L) != 0 && kblk != 0;
            has_cons = (j % L) != L - 1 && j != spx - 1 && kblk != nkb - 1 && item + 1 < nitems;
        }
        // block-uniform: only the last key block of a head is ragged
        const bool ragged = (kblk + 1) * 256 > p.S;
        const int role = (has_prod ? 1 : 0) | (has_cons ? 2 : 0);
        const int base = gen * nsteps;
#define VT_BWD_CALL(R, ROLE_) BWD_BODY<R, PRESCALED, ROLE_>(p, smem, stage, item, slot, cons_end, base, l2_prev, l2_next, dead)
#if VT_CLK
        unsigned long long clk0, rt0;
        asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(clk0), "=s"(rt0) :: "memory");
#endif
        switch (role) {
            case 0: if (ragged) VT_BWD_CALL(true, 0); else VT_BWD_CALL(false, 0); break;
            case 1: if (ragged) VT_BWD_CALL(true, 1); else VT_BWD_CALL(false, 1); break;     // a ragged block ends its head: never a producer
            case 2: VT_BWD_CALL(false, 2); break;
            default: VT_BWD_CALL(false, 3); break;
        }
#undef VT_BWD_CALL
#if VT_CLK
        {
            unsigned long long clk1, rt1;
            asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(clk1), "=s"(rt1) :: "memory");
            if (blockIdx.x == 40 && gen == 3 && threadIdx.x == 0) {
                VT_CAT(vt_bwd_clk, VT_SUFFIX)[0] = (unsigned)(clk1 - clk0);
                VT_CAT(vt_bwd_clk, VT_SUFFIX)[1] = (unsigned)(rt1 - rt0);
            }
        }
#endif
        if (has_cons) cons_end = (gen + 1) * nsteps;
        __syncthreads();                      // the LDS images are rebuilt by the next item
    }
}

// delta[b,h,s] = sum_d dO[b,s,h,d] * O[b,s,h,d]   (8 lanes per (s,h) row of 64 elements)
__global__ __launch_bounds__(256) void DELTA_KERNEL(const bf16_t* o, const bf16_t* dout, float* delta,
                                                            int B, int H, int S, long long o_rs, long long do_rs,
                                                            long long o_bs, long long do_bs) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid >> 3;          // (b, s, h) flattened with h fastest
    const int sub = (int)(gid & 7);
    const long long total = (long long)B * S * H;
    float acc = 0.f;
    long long bs = 0; int hh = 0;
    if (row < total) {
        hh = (int)(row % H);
        bs = row / H;
        const int s = (int)(bs % S);
        const int b = (int)(bs / S);
        u32x4 a = *(const u32x4*)(o + (size_t)b * o_bs + (size_t)s * o_rs + hh * 64 + sub * 8);
        u32x4 c = *(const u32x4*)(dout + (size_t)b * do_bs + (size_t)s * do_rs + hh * 64 + sub * 8);
        float fa[8], fc[8];
        unpack8(a, fa);
        unpack8(c, fc);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += fa[i] * fc[i];
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (row < total && sub == 0) {
        const int s = (int)(bs % S);
        const int b = (int)(bs / S);
        delta[((size_t)b * H + hh) * S + s] = acc;
    }
}

// workspace layout: [0,64) error word, diagnostics of the last launch | [64,256) sticky: int[16] = time-outs since the caller cleared it | [256, +64 slots) counters (ready[8] | consumed[8] per slot) | [.., +4 slots) XCC ids | tiles from the next 4 KiB boundary
static long long bwd_chain_xcc_off(long long slots) { return 256 + slots * 64; }
static long long bwd_chain_tiles_off(long long slots) { return (256 + slots * 68 + 4095) & ~4095LL; }
static long long bwd_chain_ws_bytes(long long slots) { return bwd_chain_tiles_off(slots) + slots * (long long)(CH_R * 16384); }
static int g_bwd_slots = 0;      // persistent grid: one workgroup per CU, a multiple of 8
// chain length: VT_BWD_CHAIN (1 = off), default 3.  (r01 .. mid-r02: 2 was measured best, 3 / 4 were 2-3 % slower.  With the 16x16x32 S phase and the
// conflict-free dS image, same box: B=1 loop 6.61-6.64 ms at 3 against 6.65-6.68 at 2 and 6.75-6.80 at 4; inside the training step 23.5-23.9 against
// 23.9 ms per B=4 launch -- equal or better, with a third fewer dQ atomics.)  The persistent grid is one workgroup per CU (the kernel's 145 KiB
// of LDS allow exactly one), so every slot is resident and chain neighbours start together.
static int g_bwd_chain = -1;
static void bwd_chain_init() {
    if (g_bwd_chain >= 0) return;
    int L = 3;
    if (const char* e = getenv("VT_BWD_CHAIN")) L = atoi(e);
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    g_bwd_slots = cus / 8 * 8;
    if (g_bwd_slots < 8) g_bwd_slots = 8;
    g_bwd_chain = L < 1 ? 1 : L;
}
static int bwd_chain_len() { bwd_chain_init(); return g_bwd_chain; }
// tuning / test knob: chain_len 1 = atomics only, 0 = default; slots 0 = one per CU, else a smaller persistent grid
// (multiple of 8, never more than the CU count) so that small problems run several generations
extern "C" int VT_CAT(vt_attn_bwd_set_chain, VT_SUFFIX)(int chain_len, int slots) {
    g_bwd_chain = -1;
    bwd_chain_init();
    if (chain_len > 0) g_bwd_chain = chain_len;
    if (slots > 0) {
        if ((slots % 8) || slots > g_bwd_slots) return VT_ERR_BAD_SHAPE;
        g_bwd_slots = slots;
    }
    return VT_OK;
}

// The launch plan of a problem: key blocks per head, workgroups, the persistent grid and the chain length the launch really uses.  The entry
// point and vt_attn_bwd_chain_plan both read it from here.
struct BwdPlan { int nkb; long long nwg, grid; int L; };
static BwdPlan bwd_plan(int B, int H, int S) {
    BwdPlan pl;
    pl.L = bwd_chain_len();
    pl.nkb = (S + 255) / 256;
    pl.nwg = (long long)pl.nkb * H * B;
    pl.grid = pl.nwg < g_bwd_slots ? (pl.nwg + 7) / 8 * 8 : g_bwd_slots;      // persistent grid, a multiple of 8
    if (pl.L > pl.grid / 8) pl.L = (int)(pl.grid / 8);
    if (pl.L > pl.nkb) pl.L = pl.nkb;
    return pl;
}
// host-only query (no launch): what vt_attn_bwd_hd64 would do for this problem under the current vt_attn_bwd_set_chain / VT_BWD_CHAIN state.
// have_ws: the caller hands a chain workspace of vt_attn_bwd_chain_ws_bytes.  chain_len 1 = every key block adds its dQ atomically;
// generations = key blocks a slot of the persistent grid sweeps at most.  Any of the three outputs may be NULL.
extern "C" int VT_CAT(vt_attn_bwd_chain_plan, VT_SUFFIX)(int B, int H, int S, int have_ws, int* chain_len, int* grid, int* generations) {
    if (B <= 0 || H <= 0 || S <= 0) return VT_ERR_BAD_SHAPE;
    const BwdPlan pl = bwd_plan(B, H, S);
    if (pl.nwg > 0x3fffffLL) return VT_ERR_BAD_SHAPE;
    if (chain_len) *chain_len = (have_ws && pl.L > 1) ? pl.L : 1;
    if (grid) *grid = (int)pl.grid;
    if (generations) *generations = (int)((pl.nwg + pl.grid - 1) / pl.grid);
    return VT_OK;
}

extern "C" int BWD_ENTRY(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                const float* lse2, float* delta_ws, float* dq_f32, void* dk, void* dv,
                                int B, int H, int S,
                                long long q_rs, long long k_rs, long long v_rs, long long o_rs, long long do_rs,
                                long long dq_rs, long long dk_rs, long long dv_rs,
                                long long q_bs, long long k_bs, long long v_bs, long long o_bs, long long do_bs,
                                long long dq_bs, long long dk_bs, long long dv_bs,
                                float softmax_scale, int q_prescaled, void* chain_ws, long long chain_ws_bytes,
                                void* stream) {
    if (B <= 0 || H <= 0 || S <= 0) return VT_ERR_BAD_SHAPE;
    if ((long long)S * dq_rs * 4 >= 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    if ((q_rs % 8) || (k_rs % 8) || (v_rs % 8) || (o_rs % 8) || (do_rs % 8) || (dk_rs % 4) || (dv_rs % 4)) return VT_ERR_BAD_SHAPE;
    if ((q_bs % 8) || (k_bs % 8) || (v_bs % 8) || (o_bs % 8) || (do_bs % 8) || (dk_bs % 4) || (dv_bs % 4)) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)o) | ((uintptr_t)dout)) & 15) return VT_ERR_BAD_ALIGN;
    if ((((uintptr_t)dk) | ((uintptr_t)dv)) & 7) return VT_ERR_BAD_ALIGN;
    const long long lim = 0x7fffffffLL;
    if ((long long)S * q_rs * 2 >= lim || (long long)S * k_rs * 2 >= lim || (long long)S * v_rs * 2 >= lim ||
        (long long)S * do_rs * 2 >= lim) return VT_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    {
        const long long total = (long long)B * S * H * 8;
        const int blocks = (int)((total + 255) / 256);
        hipLaunchKernelGGL(DELTA_KERNEL, dim3(blocks), dim3(256), 0, st, (const bf16_t*)o, (const bf16_t*)dout,
                           delta_ws, B, H, S, o_rs, do_rs, o_bs, do_bs);
    }
    AttnBwdParams p;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.dout = (const bf16_t*)dout;
    p.lse2 = lse2; p.delta = delta_ws; p.dq = dq_f32; p.dk = (bf16_t*)dk; p.dv = (bf16_t*)dv;
    p.S = S; p.H = H; p.B = B;
    p.q_rs = q_rs; p.k_rs = k_rs; p.v_rs = v_rs; p.do_rs = do_rs; p.dq_rs = dq_rs; p.dk_rs = dk_rs; p.dv_rs = dv_rs;
    p.q_bs = q_bs; p.k_bs = k_bs; p.v_bs = v_bs; p.do_bs = do_bs; p.dq_bs = dq_bs; p.dk_bs = dk_bs; p.dv_bs = dv_bs;
    p.scale = softmax_scale; p.scale_log2 = softmax_scale * 1.4426950408889634f;
    const BwdPlan pl = bwd_plan(B, H, S);
    if (pl.nwg > 0x3fffffLL) return VT_ERR_BAD_SHAPE;
    // dQ hand-off chains: need the caller's workspace and enough co-resident workgroups per XCD (see the header comment)
    p.chain_len = 1; p.chain_ctr = nullptr; p.chain_flags = nullptr; p.chain_xcc = nullptr; p.chain_tiles = nullptr;
    const int L = pl.L;
    const long long grid = pl.grid;
    if (chain_ws != nullptr && chain_ws_bytes >= 64 && !(((uintptr_t)chain_ws) & 255)) {
        char* ws = (char*)chain_ws;
        const bool on = L > 1 && chain_ws_bytes >= bwd_chain_ws_bytes(g_bwd_slots);
        // bytes [64, 256) are sticky (ints 16..: time-out count since the caller last cleared it) and survive every launch
        if (hipMemsetAsync(ws, 0, 64, st) != hipSuccess) return VT_ERR_LAUNCH;
        if (on && hipMemsetAsync(ws + 256, 0, (size_t)bwd_chain_tiles_off(g_bwd_slots) - 256, st) != hipSuccess) return VT_ERR_LAUNCH;
        if (on) {
            p.chain_len = L;
            p.chain_ctr = (int*)ws;
            p.chain_flags = (int*)(ws + 256);
            p.chain_xcc = (int*)(ws + bwd_chain_xcc_off(g_bwd_slots));
            p.chain_tiles = (float*)(ws + bwd_chain_tiles_off(g_bwd_slots));
        }
    }
    if (q_prescaled) hipLaunchKernelGGL(BWD_KERNEL<true>, dim3((unsigned)grid), dim3(BWD_THREADS), 0, st, p);
    else hipLaunchKernelGGL(BWD_KERNEL<false>, dim3((unsigned)grid), dim3(BWD_THREADS), 0, st, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// bytes of chain workspace vt_attn_bwd_hd64 wants for this problem (0: chains are disabled on this device / by VT_BWD_CHAIN=1)
extern "C" long long VT_CAT(vt_attn_bwd_chain_ws_bytes, VT_SUFFIX)(int B, int H, int S) {
    if (B <= 0 || H <= 0 || S <= 0 || bwd_chain_len() <= 1) return 0;
    return bwd_chain_ws_bytes(g_bwd_slots);
}
