// Flash-attention backward (dQ, dK, dV), head_dim 64, bf16 in / fp32 accumulate, non-causal, gfx950 -- the ONE-WAVE-PER-SIMD body.
//
// Same operation, operands, workspace and entry-point signature as csrc/attn_bwd.hip (autograd of the
// F.scaled_dot_product_attention call the reference reaches through videotuna/models/cogvideo_hf/cogvideo_pl.py:865-871).
//
// Structure: one workgroup = 4 waves (one per SIMD, the whole 512-register file each) = 256 keys of one (batch, head); wave w owns
// keys [64 w, 64 w + 64): dK^T / dV^T (128 registers) and its K / V fragments (64) are MFMA-only values (the register allocator
// keeps them in AGPRs: build with -mllvm -amdgpu-mfma-vgpr-form so that S'' / dP' -- the tiles the VALU touches -- are produced in
// VGPRs and only MFMA-only chains overflow into the accumulator half of the file).  The workgroup sweeps the queries 64 rows per
// step; a step is four (q-half, key-tile) tiles of 32 x 32 per wave, software-pipelined in SOURCE order (one wave per SIMD has no
// partner to hide anything behind): while the S'' / dP' MFMAs of tile n + 1 and the dV / dK MFMAs of tile n - 1 issue, the VALU
// runs exp2 / multiply / pack of tile n in their shadow, three instructions per MFMA gap; the dQ product of the PREVIOUS step
// (its dS image is in the other LDS buffer) fills the two slots that would otherwise be short of MFMAs:
//     s0: SdP(0)                 | LDS-DMA of the next Q / dO tile
//     s1: SdP(1) + dQ'(0..7)     | VALU(0)
//     s2: dVdK(0) + SdP(2)       | VALU(1), dS image rows of tile 0
//     s3: dVdK(1) + SdP(3)       | VALU(2), dS image rows of tile 1
//     s4: dVdK(2) + dQ'(8..15)   | VALU(3), dS image rows of tile 2
//     s5: dVdK(3)                | dS image rows of tile 3, dQ' out (16 atomics or the hand-off tile)
//     barrier
// The issue order is pinned by sched_barrier fences (one per MFMA gap); waits and hazards are the compiler's.
#include "../common.h"
#include <cstdlib>
#include <type_traits>

#ifndef VT4_SUFFIX
#define VT4_SUFFIX _w4
#endif
#define VT4_CAT_(a, b) a##b
#define VT4_CAT(a, b) VT4_CAT_(a, b)
#define BWD4_KERNEL VT4_CAT(attn_bwd_hd64_kernel, VT4_SUFFIX)
#define BWD4_DELTA VT4_CAT(attn_bwd_delta_kernel, VT4_SUFFIX)
#define BWD4_ENTRY VT4_CAT(vt_attn_bwd_hd64, VT4_SUFFIX)
#define FENCE() __builtin_amdgcn_sched_barrier(0)
#ifndef DQR
#define DQR 2          // k-steps of dQ operands in flight
#endif
#ifndef VT4_KREG
#define VT4_KREG 0     // 1 = the K operands of the dQ product (this wave's 32 d columns of all 256 keys: 64 registers) stay in registers for the whole key
#endif                 // block instead of being re-read from the K image every step (32 fewer LDS reads per step)
#ifndef VT4_PIN_ROWS
#define VT4_PIN_ROWS 0 // 1 = the Q / dO row fragments live in AGPRs as well
#endif
#ifndef VT4_STAMP
#define VT4_STAMP 0    // diagnostic builds (tools/kbench_stamp4.py; never shipped): 1 = s_memtime at the slot boundaries of one step of one workgroup + the
#endif                 // in-kernel clock; 2 = the in-kernel clock only (two probes per key block: the loop itself is untouched)
#if VT4_STAMP
__device__ unsigned VT4_CAT(vt_bwd4_stamps, VT4_SUFFIX)[64];
#endif
#if VT4_STAMP == 1
#define STAMP4(i) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_[i]) :: "memory")      // drains the LDS queue: slot times include their own tail
#else
#define STAMP4(i)
#endif
#ifndef VT4_ABL
#define VT4_ABL 0      // timing-only ablations (WRONG results), bit mask: 1 = no dQ atomics, 2 = no exp2, 4 = no transposed Q / dO reads, 8 = no dQ' operand
                       // reads, 16 = no Q / dO row-fragment reads, 32 = no step barrier
#endif

struct Bwd4Params {
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
    // dQ hand-off chains (csrc/attn_bwd.hip, header comment): same workspace layout, same counters in absolute steps
    int chain_len;        // 1: every key block adds its dQ partial atomically; > 1: chains of up to chain_len key blocks on consecutive slots of one XCD
    int* chain_ctr;       // [8] = error word, [9] / [10] = polls spent waiting, [11] / [12] = links through L2 / memory, [16] = STICKY time-out count
    int* chain_flags;     // [slots][16]: ready[8 waves] | consumed[8 waves] (waves 0..3 used)
    int* chain_xcc;       // [slots] 1 + XCC_ID of the workgroup that runs the slot
    float* chain_tiles;   // [slots][CH_R][4 waves][4][64 lanes][4] fp32
};
#ifndef CH_R
#define CH_R 4                   // ring depth (tiles of 64 q x 64 d fp32 = 16 KiB)
#endif
#ifndef CH_SPIN_LIMIT
#define CH_SPIN_LIMIT (1 << 19)  // polls (~1 us each) before a wait gives up (-DCH_SPIN_LIMIT=0: the forced-time-out test build)
#endif
#define CH_AUX 17                // sc0 | sc1: stores write through, loads bypass the caches

#define KIMG 0
#define DSIMG 32768
#define QTILE 98304
#define LSEOFF 131072
#define BWD4_LDS 132096

typedef __attribute__((ext_vector_type(8))) short short8v;
typedef int i32x4w __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int swz_f(int row) {
    return (((row >> 1) & 1) << 2) | (((row >> 3) & 1) << 1) | ((row >> 2) & 1);
}
__device__ __forceinline__ int swz4(int row) { return (((row >> 1) & 1) << 3) | (((row >> 3) & 1) << 2) | (((row >> 2) & 1) << 1) | (row & 1); }
__device__ __forceinline__ int swz_off(int row, int chunk) { return row * 128 + ((chunk ^ swz_f(row)) << 4); }

// LDS accesses by ABSOLUTE byte address = a per-lane register that is computed once per key block + a compile-time constant: the constant
// goes into the instruction's 16-bit offset field (every (register, constant) pair below stays under 64 KiB apart), so the main loop has
// no address arithmetic.  (Indexing a __shared__ array whose offset exceeds 64 KiB costs one VALU add per access.)
#define LDSP(T, addr) ((T __attribute__((address_space(3)))*)(uintptr_t)(addr))
__device__ __forceinline__ bf16x8 lds_rd128(unsigned base, int imm) { return *LDSP(const bf16x8, base + imm); }
__device__ __forceinline__ f32x4 lds_rd128f(unsigned base, int imm) { return *LDSP(const f32x4, base + imm); }
// two transposed 8-byte reads -> one 8 x bf16 MFMA operand
__device__ __forceinline__ bf16x8 tr_pair(unsigned a0, unsigned a1, int imm) {
    short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDSP(short4v, a0 + imm));
    short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDSP(short4v, a1 + imm));
    short8v v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v8);
}

// dV^T / dK^T accumulate in AGPRs for the whole key block: the MFMA is written out so that the accumulator's register class is ours
__device__ __forceinline__ void mfma_acc_agpr(f32x16& acc, const bf16x8 a, const u32x4 b) {      // A operand in an AGPR too (a pinned LDS read)
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "a"(a), "v"(b));
}
__device__ __forceinline__ void opaque(unsigned& x) { asm volatile("" : "+v"(x)); }     // keeps an address register from being re-derived as lane term + constant
template <class T> __device__ __forceinline__ void pin_agpr(T& x) { asm volatile("" : "+a"(x)); }

// ROLE: bit 0 = has a chain predecessor (its running dQ tile of every step is the initial accumulator here), bit 1 = has a successor (hands its
// tile on instead of adding it atomically).  A template parameter: each role gets its own register allocation.
template <bool RAGGED, bool PRESCALED, int ROLE>
__device__ __forceinline__ void bwd4_body(const Bwd4Params& p, char* smem, const int id, const int slot, const int cons_end, const int base,
                                          const bool l2_prev, const bool l2_next, bool& dead) {
    constexpr bool has_prod = (ROLE & 1) != 0, has_cons = (ROLE & 2) != 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);          // 0..3
    const int r = lane & 31, h = lane >> 5, g = lane >> 4, ql = (lane & 15) >> 2, pl = lane & 3;
    const int nkb = (p.S + 255) / 256;
    const int kblk = id % nkb, bh = id / nkb;
    const int head = bh % p.H, b = bh / p.H;
    const int key0 = kblk * 256;

    const bf16_t* qb = p.q + (size_t)b * p.q_bs + head * 64;
    const bf16_t* kb_ = p.k + (size_t)b * p.k_bs + head * 64;
    const bf16_t* vb = p.v + (size_t)b * p.v_bs + head * 64;
    const bf16_t* dob = p.dout + (size_t)b * p.do_bs + head * 64;
    __amdgpu_buffer_rsrc_t rk = make_rsrc(kb_, (unsigned)((long long)(p.S - 1) * p.k_rs * 2 + 128));
    __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, (unsigned)((long long)(p.S - 1) * p.v_rs * 2 + 128));
    __amdgpu_buffer_rsrc_t rdq = make_rsrc(p.dq + (size_t)b * p.dq_bs + head * 64, (unsigned)((long long)(p.S - 1) * p.dq_rs * 4 + 256));
    const float* lse_b = p.lse2 + (size_t)bh * p.S;
    const float* dl_b = p.delta + (size_t)bh * p.S;

    // ---- K block image (B operand of dQ): 256 keys x 8 chunks, 8 per thread ----
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = tid + 256 * j;
        const int key = i >> 3, c = i & 7;
        u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, (int)((key0 + key) * p.k_rs * 2) + c * 16, 0, 0));
        *(u32x4*)(smem + KIMG + swz_off(key, c)) = v;
    }
    // ---- K / V fragments of this wave's 64 keys (two 32-key tiles), resident for the whole key block ----
    bf16x8 kf[2][4], vf[2][4];
    float kmask[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + 64 * w + 32 * kt + r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            kf[kt][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rk, (int)(key * p.k_rs * 2) + (16 * s + 8 * h) * 2, 0, 0));
            vf[kt][s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv, (int)(key * p.v_rs * 2) + (16 * s + 8 * h) * 2, 0, 0));
        }
        kmask[kt] = (RAGGED && key >= p.S) ? -1.0e30f : 0.f;
    }
    // MFMA-only operands: pin them into the accumulator half of the register file (the MFMA takes A / B from either half)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 4; ++s) { pin_agpr(kf[kt][s]); pin_agpr(vf[kt][s]); }

    // ---- per-lane LDS addresses (absolute: region base included) ----
    const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    unsigned rowrd[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) rowrd[s] = smem_lds + QTILE + r * 128 + (((2 * s + h) ^ swz_f(r)) << 4);
    unsigned crd = smem_lds + LSEOFF + 16 * h;
    opaque(crd);
    unsigned trA[2][2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int sec = 0; sec < 2; ++sec) {
            const int fx = ((ql >> 1) << 2) | (sec << 1) | h;
            trA[dt][sec] = smem_lds + QTILE + (4 * h + ql + 8 * sec) * 128 + (((4 * dt + 2 * (g & 1) + (pl >> 1)) ^ fx) << 4) + (pl & 1) * 8;
        }
    const int qs_w = w & 1, dt_w = (w >> 1) & 1;          // dQ phase: (q-half, d-half) of the 64x64 tile
    unsigned trQA[2], trQB[2];
#pragma unroll
    for (int sec = 0; sec < 2; ++sec) {
        const int fx = ((ql >> 1) << 2) | (h << 1) | sec;
        const int row = (8 * h + ql + 4 * sec) * 128;
        trQA[sec] = smem_lds + DSIMG + row + (((2 * (4 * qs_w + 2 * (g & 1) + (pl >> 1)) + (pl & 1)) ^ swz4(8 * h + ql + 4 * sec)) << 3);
        trQB[sec] = smem_lds + KIMG + row + (((4 * dt_w + 2 * (g & 1) + (pl >> 1)) ^ fx) << 4) + (pl & 1) * 8;
    }
    {
#pragma unroll
        for (int i = 0; i < 4; ++i) opaque(rowrd[i]);
#pragma unroll
        for (int i = 0; i < 2; ++i) { opaque(trA[i][0]); opaque(trA[i][1]); opaque(trQA[i]); opaque(trQB[i]); }
    }
    const int dq_voff = (int)((32 * qs_w + 4 * h) * p.dq_rs * 4) + (32 * dt_w + r) * 4;
    const int dq_rowb = (int)(p.dq_rs * 4);

    // ---- dQ hand-off chain: every wave owns one 32 x 32 fp32 tile (4 KiB) of a hand-off tile, its own ready / consumed counter ----
    __amdgpu_buffer_rsrc_t rfl = make_rsrc(p.chain_flags, (unsigned)gridDim.x * 64u);
    __amdgpu_buffer_rsrc_t rt_mine = make_rsrc(p.chain_tiles + (size_t)slot * (CH_R * 4096), CH_R * 16384);
    __amdgpu_buffer_rsrc_t rt_prod = make_rsrc(p.chain_tiles + (size_t)(has_prod ? slot - 1 : slot) * (CH_R * 4096), CH_R * 16384);
    const int fl_ready_me = (slot * 16 + w) * 4, fl_cons_me = (slot * 16 + 8 + w) * 4;
    const int fl_ready_prod = ((slot - 1) * 16 + w) * 4, fl_cons_next = ((slot + 1) * 16 + 8 + w) * 4;
    const int tile_voff = w * 4096 + lane * 16;
    auto fl_load = [&](int off) -> int { return (int)__builtin_amdgcn_raw_buffer_load_b32(rfl, off, 0, CH_AUX); };
    int spins_r = 0, spins_c = 0;
    auto fl_wait = [&](int off, int need, int have, int& spins) {          // bounded: gives up with an error word instead of hanging
        int it = 0;
        while (have < need && !dead) {
            ++spins;
            __builtin_amdgcn_s_sleep(4);
            have = __builtin_amdgcn_readfirstlane(fl_load(off));
            if (++it > CH_SPIN_LIMIT) { dead = true; p.chain_ctr[8] = 1; atomicAdd(p.chain_ctr + 16, 1); }
        }
    };
    int pf_ready = 0, pf_cons = 0;        // counters polled one step ahead of their use
    f32x16 dq_next;                       // the predecessor's tile of the NEXT dQ': loaded in s5, the initial accumulator one step later
    // dS image: row = key, 8-byte unit u = query / 4 stored at unit u ^ swz4(row) (the dS image format of csrc/attn_bwd.hip: stores AND the dQ phase's
    // transposed reads are conflict-free).  This lane writes units 8 qs + 2 gg + h of key rows 64 w + 32 kt + r.
    unsigned dsw[2][4];
#pragma unroll
    for (int qs = 0; qs < 2; ++qs)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) dsw[qs][gg] = smem_lds + DSIMG + (64 * w + r) * 128 + (((8 * qs + 2 * gg + h) ^ swz4(r)) << 3);

    // ---- staging of the Q / dO tiles by LDS-DMA: wave w owns rows [16 w, 16 w + 16) of both tiles, two 1-KiB pieces each ----
    i32x4w rq_w, rdo_w;
    {
        const unsigned long long aq = (unsigned long long)qb, ad = (unsigned long long)dob;
        rq_w = (i32x4w){(int)(unsigned)aq, (int)((aq >> 32) & 0xffffu), (int)(unsigned)((long long)(p.S - 1) * p.q_rs * 2 + 128), 0x00020000};
        rdo_w = (i32x4w){(int)(unsigned)ad, (int)((ad >> 32) & 0xffffu), (int)(unsigned)((long long)(p.S - 1) * p.do_rs * 2 + 128), 0x00020000};
    }
    int dma_vq[2], dma_vdo[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = 16 * w + 8 * j + (lane >> 3);
        const int c = (lane & 7) ^ swz_f(row);
        dma_vq[j] = (int)(row * p.q_rs * 2) + c * 16;
        dma_vdo[j] = (int)(row * p.do_rs * 2) + c * 16;
    }
    const int stat_i = tid & 63;
    const bool stat_is_lse = (tid & 64) == 0;
    const float* stat_src = stat_is_lse ? lse_b : dl_b;
    const float stat_mul = stat_is_lse ? (PRESCALED ? -1.0f : -1.0f / p.scale_log2) : -1.0f;
    float gstat = 0.f;
    bool gok = false;
    auto gload = [&](int t, int buf) {        // tile t -> buffer buf = t & 1 (free since the barrier of step t - 2)
        const int sq = (int)((long long)t * 64 * p.q_rs * 2), sdo = (int)((long long)t * 64 * p.do_rs * 2);
        const unsigned dst = smem_lds + QTILE + buf * 16384 + (16 * w) * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                         :: "s"(dst + j * 1024), "v"(dma_vq[j]), "s"(rq_w), "s"(sq) : "memory");
#pragma unroll
        for (int j = 0; j < 2; ++j)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                         :: "s"(dst + 8192 + j * 1024), "v"(dma_vdo[j]), "s"(rdo_w), "s"(sdo) : "memory");
        int qi = t * 64 + stat_i;
        gok = qi < p.S;
        qi = gok ? qi : p.S - 1;
        gstat = stat_src[qi];                  // used by lstore only: nothing waits for it inside the step
    };
    auto lstore = [&](int buf) {     // before the barrier that publishes the tile
        *(float*)(smem + LSEOFF + buf * 512 + (tid & 127) * 4) = gok ? gstat * stat_mul : 0.f;      // threads t and t + 128 write the same value
    };

    f32x16 dk[2][2], dv[2][2];            // [key-tile][d-tile]: dK^T / dV^T of this wave's 64 keys
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) { dk[a][c][i] = 0.f; dv[a][c][i] = 0.f; }

    const float sc = p.scale_log2;
    const int nsteps = (p.S + 63) / 64;
    if (has_prod) pf_ready = fl_load(fl_ready_prod);
    gload(0, 0);
    lstore(0);
    gload(1, 1);                                // two tiles ahead from here on: step t's s5 fetches tile t + 2
    lstore(1);
    __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0): the compiler does not know about the DMA pieces
    __syncthreads();
#if VT4_KREG
    bf16x8 kq[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) { kq[m] = tr_pair(trQB[0], trQB[1], m * 2048); pin_agpr(kq[m]); }
#endif

    // pipeline state carried across slots
    f32x16 sacc[2], pacc[2];              // S'' / dP' of tile n in set n & 1
    unsigned pw[2][8], dw[2][8];          // packed P / dS of tile n in set n & 1
    f32x16 cS, cP;                        // row constants of the current q-half: C operand of a tile's first MFMAs
    bf16x8 qa[4], doa[4];                 // Q / dO row fragments of the current q-half
    bf16x8 doT[4], qT[4];                 // transposed dO / Q operands of the current q-half, combo c = (s2, dt): shared by its two key tiles (AGPRs)
    f32x16 dq_acc;
    bf16x8 fa[DQR], fb[DQR];              // dQ operands, DQR k-steps in flight

    // One step = 64 queries; BUF = t & 1 is a compile-time constant (the loop below is unrolled by two) so that every LDS address of the
    // step is a per-lane register that never changes + an immediate: no address arithmetic inside the loop.
    auto step = [&](const int t, auto buf_, auto do_s_, auto do_dq_) {
        constexpr int BUF = decltype(buf_)::value;
        constexpr bool DO_S = decltype(do_s_)::value, DO_DQ = decltype(do_dq_)::value;
        constexpr int QI = BUF * 16384, DOI = QI + 8192;          // immediates relative to the per-lane address registers

        auto rd_c = [&](int buf, int qs, int gg) {        // row constants of q-half qs of the tile in buffer buf, rows 8 gg + 4 h + (0..3)
            const f32x4 a = lds_rd128f(crd, buf * 512 + (32 * qs + 8 * gg) * 4);
            const f32x4 c = lds_rd128f(crd, buf * 512 + 256 + (32 * qs + 8 * gg) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { cS[4 * gg + e] = a[e]; cP[4 * gg + e] = c[e]; }
        };
        auto rd_rows = [&](int buf, int qs, int s) {
#if VT4_ABL & 16
            if (t == 0 && qs == 0 && buf == 1) { qa[s] = lds_rd128(rowrd[s], 0); doa[s] = lds_rd128(rowrd[s], 8192); }
#else
            qa[s] = lds_rd128(rowrd[s], buf * 16384 + qs * 4096);
            doa[s] = lds_rd128(rowrd[s], buf * 16384 + 8192 + qs * 4096);
#if VT4_PIN_ROWS
            pin_agpr(qa[s]); pin_agpr(doa[s]);
#endif
#endif
        };
        // MFMA i (0..7) of SdP(n): k-step i >> 1, S'' (even) or dP' (odd)
        auto sdp = [&](int n, int i) {
            const int kt = n & 1, set = n & 1, s = i >> 1;
            if ((i & 1) == 0) sacc[set] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[s], kf[kt][s], s == 0 ? cS : sacc[set], 0, 0, 0);
            else pacc[set] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(doa[s], vf[kt][s], s == 0 ? cP : pacc[set], 0, 0, 0);
        };
        // gap k (0..15) of VALU(n), spread evenly: exp2 of element k, the product of element k - 1 (never the consumer of the exp2 just issued: a
        // transcendental result needs a wait state before a dependent VALU), one pack of the pair that has just completed; the tail at k = 15
        float e_[16], d_[16];
        auto valu = [&](int n, int k) {
            const int set = n & 1, kt = n & 1;
            float x = sacc[set][k];
            if (RAGGED) x += kmask[kt];
            if (!PRESCALED) x *= sc;
#if VT4_ABL & 2
            e_[k] = x;
#else
            e_[k] = __builtin_amdgcn_exp2f(x);
#endif
            if (k >= 1) d_[k - 1] = e_[k - 1] * pacc[set][k - 1];
            if (k >= 2 && (k & 1) == 0) pw[set][(k - 2) >> 1] = pack2(e_[k - 2], e_[k - 1]);
            if (k >= 3 && (k & 1) == 1) dw[set][(k - 3) >> 1] = pack2(d_[k - 3], d_[k - 2]);
            if (k == 15) {
                d_[15] = e_[15] * pacc[set][15];
                pw[set][7] = pack2(e_[14], e_[15]);
                dw[set][7] = pack2(d_[14], d_[15]);
            }
        };
        // transposed operands of dVdK, combo c (0..3) = (s2, dt) = (c >> 1, c & 1) of q-half qs
        auto rd_tr_do = [&](int qs, int c) {
            const int ro = (32 * qs + 16 * (c >> 1)) * 128, dt = c & 1;
#if VT4_ABL & 4
            (void)ro; doT[c] = qa[dt];
#else
            doT[c] = tr_pair(trA[dt][0], trA[dt][1], DOI + ro);
            pin_agpr(doT[c]);
#endif
        };
        auto rd_tr_q = [&](int qs, int c) {
            const int ro = (32 * qs + 16 * (c >> 1)) * 128, dt = c & 1;
#if VT4_ABL & 4
            (void)ro; qT[c] = doa[dt];
#else
            qT[c] = tr_pair(trA[dt][0], trA[dt][1], QI + ro);
            pin_agpr(qT[c]);
#endif
        };
        // MFMA i (0..7) of dVdK(n): combo i >> 1, dV (even) or dK (odd)
        auto dvdk = [&](int n, int i) {
            const int kt = n & 1, set = n & 1, c = i >> 1, s2 = c >> 1, dt = c & 1;
            if ((i & 1) == 0) {
                const u32x4 pb4 = {pw[set][4 * s2], pw[set][4 * s2 + 1], pw[set][4 * s2 + 2], pw[set][4 * s2 + 3]};
                mfma_acc_agpr(dv[kt][dt], doT[c], pb4);
            } else {
                const u32x4 db4 = {dw[set][4 * s2], dw[set][4 * s2 + 1], dw[set][4 * s2 + 2], dw[set][4 * s2 + 3]};
                mfma_acc_agpr(dk[kt][dt], qT[c], db4);
            }
        };
        // dS image rows of tile n (8-byte unit 8 qs + 2 gg + h of key row 64 w + 32 kt + r, units swizzled by swz4(row): conflict-free stores)
        auto ds_wr = [&](int n, int gg) {
            const int qs = n >> 1, kt = n & 1, set = n & 1;
            const u32x2 two = {dw[set][2 * gg], dw[set][2 * gg + 1]};
            *LDSP(u32x2, dsw[qs][gg] + (BUF * 32768 + kt * 4096)) = two;
        };
        // dQ' (the previous step's dQ tile): k-step m (0..15) of 16 keys
        auto rd_dq_a = [&](int m) {
            if (m >= 16) return;
#if VT4_ABL & 8
            fa[m % DQR] = qa[m & 3];
#else
            fa[m % DQR] = tr_pair(trQA[0], trQA[1], (BUF ^ 1) * 32768 + m * 2048);
#endif
        };
        auto rd_dq_b = [&](int m) {
            if (m >= 16) return;
#if VT4_KREG
            return;
#elif VT4_ABL & 8
            fb[m % DQR] = doa[m & 3];
#else
            fb[m % DQR] = tr_pair(trQB[0], trQB[1], m * 2048);
#endif
        };
#if VT4_KREG
        auto dqm = [&](int m) { dq_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m % DQR], kq[m], dq_acc, 0, 0, 0); };
#else
        auto dqm = [&](int m) { dq_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m % DQR], fb[m % DQR], dq_acc, 0, 0, 0); };
#endif

#if VT4_STAMP == 1
        unsigned long long st_[8];
#endif
        STAMP4(0);
        // ================= s0: SdP(0) | LDS-DMA of the next tile, q-half 0's transposed operands, the first dQ' operands =================
        if (DO_DQ) {
            if (has_prod) dq_acc = dq_next;
            else {
#pragma unroll
                for (int i = 0; i < 16; ++i) dq_acc[i] = 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (DO_S) {
                sdp(0, i); FENCE();
                if ((i & 1) == 0) rd_tr_do(0, i >> 1); else rd_tr_q(0, i >> 1);      // these registers were last used by the previous step's dVdK(3)
            }
            if (DO_DQ) {
                if (i >= 8 - 2 * DQR) { if ((i & 1) == 0) rd_dq_a((i - (8 - 2 * DQR)) >> 1); else rd_dq_b((i - (8 - 2 * DQR)) >> 1); }
            }
            FENCE();
        }
        STAMP4(1);
        // ================= s1: SdP(1) + dQ'(0..7) | VALU(0), q-half 1's row operands =================
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if ((k & 1) == 0) { if (DO_S) { sdp(1, k >> 1); FENCE(); } if (DO_DQ && k >= 2) rd_dq_b((k >> 1) - 1 + DQR); }
            else if (DO_DQ) { dqm(k >> 1); FENCE(); rd_dq_a((k >> 1) + DQR); if (k == 15) rd_dq_b(7 + DQR); }
            if (DO_S) {
                valu(0, k);
                // the q-half 0 operands are free once SdP(1) has used them: fetch q-half 1's into the same registers
                if (k >= 2 && k <= 8 && (k & 1) == 0) rd_c(BUF, 1, (k >> 1) - 1);
                if ((k & 3) == 3) rd_rows(BUF, 1, k >> 2);                  // k = 3, 7, 11, 15 -> s = 0..3
            }
            FENCE();
        }
        STAMP4(2);
        // ================= s2: dVdK(0) + SdP(2) | VALU(1), dS rows of tile 0 =================
        // ================= s3: dVdK(1) + SdP(3) | VALU(2), dS rows of tile 1; q-half 1's transposed operands =================
        if (DO_S) {
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                if (n == 1) STAMP4(3);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if ((k & 1) == 0) dvdk(n, k >> 1); else sdp(n + 2, k >> 1);
                    FENCE();                                                  // the MFMA leads its gap: the fillers run in its shadow
                    valu(n + 1, k);
                    if (n == 1 && (k & 3) == 1) rd_tr_do(1, k >> 2);          // combo k >> 2: dO^T was last used at k - 1, Q^T at k + 1
                    if (n == 1 && (k & 3) == 3) rd_tr_q(1, k >> 2);
                    if ((k & 3) == 2) ds_wr(n, k >> 2);
                    FENCE();
                }
            }
        }
        STAMP4(4);
        // ================= s4: dVdK(2) + dQ'(8..15) | VALU(3), dS rows of tiles 2 and 3 =================
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if ((k & 1) == 0) { if (DO_S) { dvdk(2, k >> 1); FENCE(); } if (DO_DQ && k >= 2) rd_dq_b(7 + (k >> 1) + DQR); }
            else if (DO_DQ) { dqm(8 + (k >> 1)); FENCE(); rd_dq_a(8 + (k >> 1) + DQR); if (k == 15) rd_dq_b(15 + DQR); }
            if (DO_S) {
                valu(3, k);
                if ((k & 3) == 2) ds_wr(2, k >> 2);
                if (k == 7 || k == 11 || k == 15) ds_wr(3, (k - 7) >> 2);     // dS pairs 2 gg, 2 gg + 1 of tile 3 are packed by k = 4 gg + 5
                if (k == 15) ds_wr(3, 3);
            }
            FENCE();
        }
        STAMP4(5);
        // ================= barrier: the dS image of this step is complete, the next Q / dO tile has landed =================
        if (DO_S) {
            // the row constants were loaded right BEHIND the next tile's DMA pieces (gload): vector memory completes in order, so the wait the
            // compiler puts in front of this store covers the pieces too, and counts only the younger operations it knows (this step's
            // atomics / hand-off stores and loads, all issued after gload) -- they stay in flight
            lstore(BUF ^ 1);
        }
#if !(VT4_ABL & 32)
        __syncthreads();
#endif
        STAMP4(6);
        // ================= s5: dVdK(3) (operands in registers) | the NEXT step's first reads; everything this step moves through vector memory =================
        // tau = t - 1: the dQ' tile finished in s4; t: the tile whose product starts in the next step's s1
        const int soff = (int)((long long)(t - 1) * 64 * p.dq_rs * 4);
        if (has_cons && DO_DQ && t >= 2) {               // publish tile t - 2 (stored one step ago): its stores must have completed
            __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): everything outstanding is at least a step old
            __builtin_amdgcn_raw_buffer_store_b32((unsigned)(base + t - 1), rfl, fl_ready_me, 0, CH_AUX);
        }
        if (DO_S) {
            // LDS-DMA of tile t + 2 into the buffer tile t has just left (its last reads were before the barrier; dVdK(3)'s operands are in
            // registers): first in the step's vector-memory queue, a whole step to land.  Past the end: bounds-checked loads return zeros
            gload(t + 2, BUF);
            FENCE();
        }
        if (has_prod && DO_S) {                          // the predecessor's tile t: the initial accumulator of dQ'(t)
            int s_ready = __builtin_amdgcn_readfirstlane(pf_ready);
            if (s_ready < base + t + 1) fl_wait(fl_ready_prod, base + t + 1, s_ready, spins_r);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v = l2_prev
                    ? __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rt_prod, tile_voff + j * 1024, ((base + t) % CH_R) * 16384, 16))
                    : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rt_prod, tile_voff + j * 1024, ((base + t) % CH_R) * 16384, CH_AUX));
#pragma unroll
                for (int e = 0; e < 4; ++e) dq_next[4 * j + e] = v[e];
            }
            pf_ready = fl_load(fl_ready_prod);
            FENCE();
        }
        if (has_cons && DO_DQ) {                         // my ring slot of tile tau must have been consumed
            const int a_ = base + t - 1;
            int need = a_ - CH_R + 1;
            if (t - 1 < CH_R && need > cons_end) need = cons_end;
            const int s_cons = __builtin_amdgcn_readfirstlane(pf_cons);
            if (need > 0 && s_cons < need) fl_wait(fl_cons_next, need, s_cons, spins_c);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (DO_S) {
                dvdk(3, i); FENCE();
                if (i < 4) rd_c(BUF ^ 1, 0, i); else rd_rows(BUF ^ 1, 0, i - 4);      // their latency hides under these MFMAs, not at the next step's head
            }
            if (DO_DQ) {
                if (has_cons) {
                    if ((i & 1) == 0) {
                        const int j = i >> 1;
                        const f32x4 v = {dq_acc[4 * j], dq_acc[4 * j + 1], dq_acc[4 * j + 2], dq_acc[4 * j + 3]};
                        if (l2_next) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rt_mine, tile_voff + j * 1024, ((base + t - 1) % CH_R) * 16384, 0);
                        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rt_mine, tile_voff + j * 1024, ((base + t - 1) % CH_R) * 16384, CH_AUX);
                    }
                } else {
#pragma unroll
                    for (int j = 2 * i; j < 2 * i + 2; ++j) {
#if VT4_ABL & 1
                        asm volatile("" ::"v"(dq_acc[j]));
#else
                        __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(dq_acc[j] * p.scale, rdq, dq_voff, soff + ((j & 3) + 8 * (j >> 2)) * dq_rowb, 0);
#endif
                    }
                }
            }
            FENCE();
        }
        if (has_prod && DO_DQ) __builtin_amdgcn_raw_buffer_store_b32((unsigned)(base + t), rfl, fl_cons_me, 0, CH_AUX);     // tile tau's loads completed in s1
        if (has_cons && DO_S) pf_cons = fl_load(fl_cons_next);
#if VT4_STAMP == 1
        STAMP4(7);
        if (t == 100 && blockIdx.x == 40 && id < (int)gridDim.x) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) VT4_CAT(vt_bwd4_stamps, VT4_SUFFIX)[w * 8 + i] = (unsigned)st_[i];
            }
        }
#endif
    };

    using B0 = std::integral_constant<int, 0>; using B1 = std::integral_constant<int, 1>;
    {   // first reads of step 0 (every later step gets them from its predecessor's s5)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const f32x4 a = lds_rd128f(crd, (8 * gg) * 4), c = lds_rd128f(crd, 256 + (8 * gg) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { cS[4 * gg + e] = a[e]; cP[4 * gg + e] = c[e]; }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) { qa[s] = lds_rd128(rowrd[s], 0); doa[s] = lds_rd128(rowrd[s], 8192); }
    }
#if VT4_STAMP
    unsigned long long clk0 = 0, rt0 = 0;       // in-kernel clock of this key block's loop: d(s_memtime) / d(s_memrealtime) x 100 MHz (MI355X_MICROARCH.md, DVFS item 6)
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(clk0), "=s"(rt0) :: "memory");
#endif
    step(0, B0{}, std::true_type{}, std::false_type{});
    int t = 1;
    for (; t + 1 < nsteps; t += 2) {
        step(t, B1{}, std::true_type{}, std::true_type{});
        step(t + 1, B0{}, std::true_type{}, std::true_type{});
    }
    if (t < nsteps) { step(t, B1{}, std::true_type{}, std::true_type{}); ++t; }           // t is odd here
    if (t & 1) step(t, B1{}, std::false_type{}, std::true_type{}); else step(t, B0{}, std::false_type{}, std::true_type{});
#if VT4_STAMP
    {
        unsigned long long clk1, rt1;
        asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(clk1), "=s"(rt1) :: "memory");
        if (blockIdx.x == 40 && id >= 3 * (int)gridDim.x && id < 4 * (int)gridDim.x && threadIdx.x == 0) {      // the fourth key block of this slot: clocks have settled
            VT4_CAT(vt_bwd4_stamps, VT4_SUFFIX)[40] = (unsigned)(clk1 - clk0);
            VT4_CAT(vt_bwd4_stamps, VT4_SUFFIX)[41] = (unsigned)(rt1 - rt0);
        }
    }
#endif

    if ((has_prod || has_cons) && lane == 0 && (spins_r | spins_c)) {
        if (spins_r) atomicAdd(p.chain_ctr + 9, spins_r);
        if (spins_c) atomicAdd(p.chain_ctr + 10, spins_c);
    }
    if (has_cons) {     // the last two tiles (nsteps - 2 was stored in the last full step's s5, nsteps - 1 in the drain step's)
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __builtin_amdgcn_raw_buffer_store_b32((unsigned)(base + nsteps), rfl, fl_ready_me, 0, CH_AUX);
    }

    // ---- epilogue: dK^T, dV^T accumulators -> dk[key][d], dv[key][d] ----
    const float dk_mul = PRESCALED ? 0.6931471805599453f : p.scale;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + 64 * w + 32 * kt + r;
        if (key < p.S) {
            bf16_t* dkp = p.dk + (size_t)b * p.dk_bs + (size_t)key * p.dk_rs + head * 64;
            bf16_t* dvp = p.dv + (size_t)b * p.dv_bs + (size_t)key * p.dv_rs + head * 64;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    u32x2 a, c;
                    a[0] = pack2(dk[kt][dt][4 * gg + 0] * dk_mul, dk[kt][dt][4 * gg + 1] * dk_mul);
                    a[1] = pack2(dk[kt][dt][4 * gg + 2] * dk_mul, dk[kt][dt][4 * gg + 3] * dk_mul);
                    c[0] = pack2(dv[kt][dt][4 * gg + 0], dv[kt][dt][4 * gg + 1]);
                    c[1] = pack2(dv[kt][dt][4 * gg + 2], dv[kt][dt][4 * gg + 3]);
                    *(u32x2*)(dkp + 32 * dt + 8 * gg + 4 * h) = a;
                    *(u32x2*)(dvp + 32 * dt + 8 * gg + 4 * h) = c;
                }
        }
    }
}

template <bool PRESCALED>
__global__ __launch_bounds__(256, 1) void BWD4_KERNEL(Bwd4Params p) {
    __shared__ __attribute__((aligned(16))) char smem[BWD4_LDS];
    const int nkb = (p.S + 255) / 256;
    const int nitems = nkb * p.H * p.B, nsteps = (p.S + 63) / 64;
    const int L = p.chain_len;
    // persistent grid: slot = (XCD, index inside the XCD) under round-robin dispatch; a slot sweeps the key blocks slot, slot + G, ...: consecutive
    // key blocks of a head run side by side on one XCD and stream the same Q / dO tiles through its L2 at the same time
    const int spx = gridDim.x >> 3;
    const int slot = (int)(blockIdx.x & 7) * spx + (int)(blockIdx.x >> 3);
    bool dead = false;
    int cons_end = 0, gen = 0;
    bool l2_prev = false, l2_next = false;
    if (L > 1) {
        // chain neighbours on the same XCD exchange their tiles through its L2 (plain stores, agent-scope loads), any other pair through
        // memory: every slot publishes 1 + XCC_ID once; nothing relies on the dispatch order for correctness
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
            if (threadIdx.x == 0) atomicAdd(p.chain_ctr + (l2_prev ? 11 : 12), 1);
        }
        if ((j % L) != L - 1 && j != spx - 1 && slot + 1 < (int)gridDim.x) l2_next = peer(slot + 1) == xcc;
    }
    for (int item = slot; item < nitems; item += gridDim.x, ++gen) {
        const int kblk = item % nkb;
        bool hp = false, hc = false;
        if (L > 1) {
            const int j = slot % spx;         // chains: same head, same XCD, at most L long, aligned to multiples of L
            hp = (j % L) != 0 && kblk != 0;
            hc = (j % L) != L - 1 && j != spx - 1 && kblk != nkb - 1 && item + 1 < nitems;
        }
        const bool ragged = (kblk + 1) * 256 > p.S;      // block-uniform: only the last key block of a head is ragged
        const int role = (hp ? 1 : 0) | (hc ? 2 : 0);
        const int base = gen * (nsteps + 0);
#define VT4_CALL(R, ROLE_) bwd4_body<R, PRESCALED, ROLE_>(p, smem, item, slot, cons_end, base, l2_prev, l2_next, dead)
        switch (role) {
            case 0: if (ragged) VT4_CALL(true, 0); else VT4_CALL(false, 0); break;
            case 1: if (ragged) VT4_CALL(true, 1); else VT4_CALL(false, 1); break;     // a ragged block ends its head: never a producer
            case 2: VT4_CALL(false, 2); break;
            default: VT4_CALL(false, 3); break;
        }
#undef VT4_CALL
        if (hc) cons_end = (gen + 1) * nsteps;
        __syncthreads();                      // the LDS images are rebuilt by the next item
    }
}

// delta[b,h,s] = sum_d dO[b,s,h,d] * O[b,s,h,d]   (8 lanes per (s,h) row of 64 elements)
__global__ __launch_bounds__(256) void BWD4_DELTA(const bf16_t* o, const bf16_t* dout, float* delta, int B, int H, int S,
                                                  long long o_rs, long long do_rs, long long o_bs, long long do_bs) {
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

// workspace layout (as csrc/attn_bwd.hip): [0,64) error word + diagnostics of the last launch | [64,256) sticky: int[16] = time-outs since the caller cleared
// them | [256, +64 slots) counters | [.., +4 slots) XCC ids | tiles from the next 4 KiB boundary
static long long bwd4_xcc_off(long long slots) { return 256 + slots * 64; }
static long long bwd4_tiles_off(long long slots) { return (256 + slots * 68 + 4095) & ~4095LL; }
static long long bwd4_ws_bytes(long long slots) { return bwd4_tiles_off(slots) + slots * (long long)(CH_R * 16384); }
static int g_bwd4_slots = 0, g_bwd4_chain = -1;
static void bwd4_init() {
    if (g_bwd4_chain >= 0) return;
    int Lc = 3;
    if (const char* e = getenv("VT_BWD_CHAIN")) Lc = atoi(e);
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    g_bwd4_slots = cus / 8 * 8;
    if (g_bwd4_slots < 8) g_bwd4_slots = 8;
    g_bwd4_chain = Lc < 1 ? 1 : Lc;
}
extern "C" int VT4_CAT(vt_attn_bwd_set_chain, VT4_SUFFIX)(int chain_len, int slots) {
    g_bwd4_chain = -1;
    bwd4_init();
    if (chain_len > 0) g_bwd4_chain = chain_len;
    if (slots > 0) {
        if ((slots % 8) || slots > g_bwd4_slots) return VT_ERR_BAD_SHAPE;
        g_bwd4_slots = slots;
    }
    return VT_OK;
}
extern "C" long long VT4_CAT(vt_attn_bwd_chain_ws_bytes, VT4_SUFFIX)(int B, int H, int S) {
    bwd4_init();
    if (B <= 0 || H <= 0 || S <= 0 || g_bwd4_chain <= 1) return 0;
    return bwd4_ws_bytes(g_bwd4_slots);
}

extern "C" int BWD4_ENTRY(const void* q, const void* k, const void* v, const void* o, const void* dout,
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
        hipLaunchKernelGGL(BWD4_DELTA, dim3(blocks), dim3(256), 0, st, (const bf16_t*)o, (const bf16_t*)dout,
                           delta_ws, B, H, S, o_rs, do_rs, o_bs, do_bs);
    }
    Bwd4Params p;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.dout = (const bf16_t*)dout;
    p.lse2 = lse2; p.delta = delta_ws; p.dq = dq_f32; p.dk = (bf16_t*)dk; p.dv = (bf16_t*)dv;
    p.S = S; p.H = H; p.B = B;
    p.q_rs = q_rs; p.k_rs = k_rs; p.v_rs = v_rs; p.do_rs = do_rs; p.dq_rs = dq_rs; p.dk_rs = dk_rs; p.dv_rs = dv_rs;
    p.q_bs = q_bs; p.k_bs = k_bs; p.v_bs = v_bs; p.do_bs = do_bs; p.dq_bs = dq_bs; p.dk_bs = dk_bs; p.dv_bs = dv_bs;
    p.scale = softmax_scale; p.scale_log2 = softmax_scale * 1.4426950408889634f;
    const int nkb = (S + 255) / 256;
    const long long nwg = (long long)nkb * H * B;
    if (nwg > 0x3fffffLL) return VT_ERR_BAD_SHAPE;
    bwd4_init();
    p.chain_len = 1; p.chain_ctr = nullptr; p.chain_flags = nullptr; p.chain_xcc = nullptr; p.chain_tiles = nullptr;
    int Lc = g_bwd4_chain;
    const long long grid = nwg < g_bwd4_slots ? (nwg + 7) / 8 * 8 : g_bwd4_slots;      // persistent grid, a multiple of 8
    if (Lc > grid / 8) Lc = (int)(grid / 8);
    if (Lc > nkb) Lc = nkb;
    if (chain_ws != nullptr && chain_ws_bytes >= 64 && !(((uintptr_t)chain_ws) & 255)) {
        char* ws = (char*)chain_ws;
        const bool on = Lc > 1 && chain_ws_bytes >= bwd4_ws_bytes(g_bwd4_slots);
        // bytes [64, 256) are sticky (ints 16..: time-out count since the caller last cleared it) and survive every launch
        if (hipMemsetAsync(ws, 0, 64, st) != hipSuccess) return VT_ERR_LAUNCH;
        if (on && hipMemsetAsync(ws + 256, 0, (size_t)bwd4_tiles_off(g_bwd4_slots) - 256, st) != hipSuccess) return VT_ERR_LAUNCH;
        if (on) {
            p.chain_len = Lc;
            p.chain_ctr = (int*)ws;
            p.chain_flags = (int*)(ws + 256);
            p.chain_xcc = (int*)(ws + bwd4_xcc_off(g_bwd4_slots));
            p.chain_tiles = (float*)(ws + bwd4_tiles_off(g_bwd4_slots));
        }
    }
    if (q_prescaled) hipLaunchKernelGGL(BWD4_KERNEL<true>, dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(BWD4_KERNEL<false>, dim3((unsigned)grid), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

#if VT4_STAMP
extern "C" int VT4_CAT(vt_attn_bwd_stamps, VT4_SUFFIX)(unsigned* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(VT4_CAT(vt_bwd4_stamps, VT4_SUFFIX)), 64 * sizeof(unsigned)) == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
#endif
