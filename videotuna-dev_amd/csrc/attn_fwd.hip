// Flash-attention forward, head_dim 64, bf16 in / fp32 accumulate, non-causal, no mask, for gfx950.
//
// Replaces F.scaled_dot_product_attention inside diffusers' CogVideoXAttnProcessor2_0, reached by the
// reference at videotuna/models/cogvideo_hf/cogvideo_pl.py:865-871: joint text+video
// self-attention, q,k,v [B,30,17776,64] at the benchmark shape.
//
// Structure: one workgroup = 4 waves = 128 query rows of one (batch, head); each wave owns 32 queries.
// K/V tiles of 64 keys are staged by LDS-DMA (buffer_load ... lds; double buffered, tile t+1 in flight
// while tile t is consumed).  Scores are computed TRANSPOSED, S^T = K * Q^T with
// v_mfma_f32_32x32x16_bf16, so a lane owns one query column and 2x16 keys: the online-softmax row
// reductions are lane-local plus one cross-half exchange, and the fp32 P^T accumulator tile is, after
// bf16 packing, directly the B operand of the second product O^T += V^T * P^T (no LDS round trip for
// P).  V^T fragments come from the row-major V tile through ds_read_b64_tr_b16.
// Layout contract: q/k/v/o are addressed as ptr + b*batch_stride + s*row_stride + h*64 + d, so the
// fused QKV GEMM output [B*S, 3*H*64] is consumed in place (no head transpose copies).
// With q pre-scaled (the training path) the cross-half exchange of the row maximum is taken only when a rescale happens.
// What was measured against this kernel and not kept is recorded in exp/README.md.
#include "common.h"

struct AttnFwdParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* v;
    bf16_t* o;
    float* lse2;     // [B,H,S] fp32: log2-domain logsumexp of (score * scale_log2)
    int S, H, B;
    long long q_rs, k_rs, v_rs, o_rs;
    long long q_bs, k_bs, v_bs, o_bs;
    float scale_log2;
    const float* bias_t;   // BIAS kernels: additive score bias, TRANSPOSED [H][S keys][S queries] fp32 (same for every sample), or null
};

#define FQ 128      // queries per workgroup: 4 waves x 32
#define FWD_THREADS 256
#define FK 64       // keys per tile
#define NEG_BIG (-1.0e30f)
#define LAZY_THR 8.0f

// BIAS (T5 relative position bias; SURVEY 8(f) row 1, the frozen text encoder): scores get bias[h][q][key] added before the
// softmax.  The table is read transposed so that the 32 lanes of a half-wave (consecutive queries) load consecutive words.
template <bool PRESCALED, bool BIAS = false>
__global__ __launch_bounds__(FWD_THREADS, 2) void attn_fwd_hd64_kernel(AttnFwdParams p) {
    __shared__ __attribute__((aligned(16))) char smem[32768];   // 2 x (K 8 KiB + V 8 KiB)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nqt = (p.S + FQ - 1) / FQ;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int qt = id % nqt;
    const int bh = id / nqt;
    const int head = bh % p.H, b = bh / p.H;
    const int q0 = qt * FQ + wave * 32;

    const bf16_t* qb = p.q + (size_t)b * p.q_bs + head * 64;
    const bf16_t* kb = p.k + (size_t)b * p.k_bs + head * 64;
    const bf16_t* vb = p.v + (size_t)b * p.v_bs + head * 64;
    __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, (unsigned)((long long)(p.S - 1) * p.k_rs * 2 + 128));
    __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, (unsigned)((long long)(p.S - 1) * p.v_rs * 2 + 128));

    // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[q0+r][16s + 8h .. +7] ----
    bf16x8 qf[4];
    {
        int qrow = q0 + r;
        if (qrow > p.S - 1) qrow = p.S - 1;       // clamp: rows past the end are computed but never stored
        const bf16_t* qp = qb + (size_t)qrow * p.q_rs + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);
    }

    // Per-thread chunk assignment of the former register staging (global -> VGPR -> ds_write_b128).  Nothing reads it.  It stays because the
    // compiler orders this kernel's prologue differently without it, and this file's machine code changes only together with a measurement.
    int k_voff[2], v_voff[2], k_lds[2], v_lds[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int i = tid + FWD_THREADS * j;
        int key = i >> 3, c = i & 7;
        k_voff[j] = (int)(key * p.k_rs * 2) + c * 16;
        v_voff[j] = (int)(key * p.v_rs * 2) + c * 16;
        k_lds[j] = key * 128 + ((c ^ ((key >> 1) & 7)) << 4);
        v_lds[j] = 8192 + key * 128 + ((c ^ (((key >> 1) & 1) << 2)) << 4);
    }
    // LDS-DMA staging: a K (or V) tile of 64 keys is 8 pieces of 1 KiB = 8 rows x 128 B; wave w moves pieces w and w+4 of each.
    // Lane l lands at (row l>>3, physical chunk l&7) of its piece and fetches the logical chunk the image's swizzle puts there.
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    constexpr int NPC = 2;                       // 1-KiB pieces of K (and of V) per wave per tile
    int kd_voff[2], vd_voff[2];
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
        const int key = 8 * (wv + 4 * j) + (lane >> 3);
        kd_voff[j] = (int)(key * p.k_rs * 2) + (((lane & 7) ^ ((key >> 1) & 7)) << 4);
        vd_voff[j] = (int)(key * p.v_rs * 2) + (((lane & 7) ^ (((key >> 1) & 1) << 2)) << 4);
    }
    auto dma = [&](int t, int buf) {
        const int ks = (int)((long long)t * FK * p.k_rs * 2);
        const int vs = (int)((long long)t * FK * p.v_rs * 2);
#pragma unroll
        for (int j = 0; j < NPC; ++j) {
            char* dst = smem + buf * 16384 + (wv + 4 * j) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (__attribute__((address_space(3))) void*)dst, 16, kd_voff[j], ks, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void*)(dst + 8192), 16, vd_voff[j], vs, 0, 0);
        }
    };

    // ---- per-lane LDS read offsets ----
    int kfo[4];                                   // K fragment, k-step s: row r, chunk (2s+h) swizzled
#pragma unroll
    for (int s = 0; s < 4; ++s) kfo[s] = r * 128 + (((2 * s + h) ^ ((r >> 1) & 7)) << 4);
    int vfo[2];                                   // V^T fragment (transposed read), d-tile dt
    {
        const int g = lane >> 4;                  // 16-lane group
        const int ql = (lane & 15) >> 2;          // block row supplied by this lane
        const int pl = lane & 3;                  // 4-column piece supplied by this lane
        const int keyl = 4 * (g >> 1) + ql;       // + 32*kt2 + 16*s' (+8)
        const int x = (ql >> 1) & 1;              // ((key >> 1) & 1) for every key this lane addresses
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            int chunk = 4 * dt + 2 * (g & 1) + (pl >> 1);
            vfo[dt] = 8192 + keyl * 128 + ((chunk ^ (x << 2)) << 4) + (pl & 1) * 8;
        }
    }

    f32x16 o_acc[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { o_acc[0][i] = 0.f; o_acc[1][i] = 0.f; }
    float m_run = PRESCALED ? 0.f : NEG_BIG, l_run = 0.f;
    f32x16 negm;                                  // PRESCALED: -m_run broadcast, the initial S^T accumulator
#pragma unroll
    for (int i = 0; i < 16; ++i) negm[i] = 0.f;
    const float sc = p.scale_log2;

    const int nt = (p.S + FK - 1) / FK;
    dma(0, 0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) dma(t + 1, buf ^ 1);
        const char* base = smem + buf * 16384;

        f32x16 st[2];
        if constexpr (PRESCALED) {
            // ---- lazy-max online softmax (q carries softmax_scale*log2e): the accumulators START at -m_ref, so the
            // MFMA chain delivers s - m_ref and P = exp2(st) needs no subtraction; O and l are rescaled only when some
            // row's maximum grew by more than LAZY_THR (P then stays <= 2^LAZY_THR), which is rare after the first tiles.
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2) {
                    bf16x8 kf = *(const bf16x8*)(base + kt2 * 4096 + kfo[s]);
                    st[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], s == 0 ? negm : st[kt2], 0, 0, 0);
                }
            }
            if ((t + 1) * FK > p.S) {
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        int key = t * FK + kt2 * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        if (key >= p.S) st[kt2][i] = NEG_BIG;
                    }
            }
            float mx = st[0][0];
#pragma unroll
            for (int i = 1; i < 16; ++i) mx = fmaxf(mx, st[0][i]);
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, st[1][i]);
            if (t == 0 || !__all(mx <= LAZY_THR)) {            // wave-uniform (the two lane halves of a query each test their own keys)
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));       // the row maximum itself is needed only here: keep the cross-half exchange (an LDS
                                                               // round trip) off the common path
                const float delta = (t == 0) ? mx : fmaxf(mx, 0.f);
                const float alpha = (t == 0) ? 1.0f : __builtin_amdgcn_exp2f(-delta);
                m_run += delta;
                l_run *= alpha;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    o_acc[0][i] *= alpha; o_acc[1][i] *= alpha;
                    st[0][i] -= delta; st[1][i] -= delta;
                    negm[i] = -m_run;
                }
            }
            float psum = 0.f;
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float pv = __builtin_amdgcn_exp2f(st[kt2][i]);
                    st[kt2][i] = pv;
                    psum += pv;
                }
            l_run += psum;
        } else {
        // ---- S^T = K Q^T : 2 key sub-tiles x 4 k-steps ----
#pragma unroll
        for (int i = 0; i < 16; ++i) { st[0][i] = 0.f; st[1][i] = 0.f; }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2) {
                bf16x8 kf = *(const bf16x8*)(base + kt2 * 4096 + kfo[s]);
                st[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st[kt2], 0, 0, 0);
            }
        }
        if constexpr (BIAS) {
            int qc = q0 + r;
            qc = qc < p.S ? qc : p.S - 1;
            const float* bp = p.bias_t + ((size_t)head * p.S) * p.S + qc;
            const float isc = 1.0f / sc * 1.4426950408889634f;        // the bias is in score units: (s*scale + bias) * log2e
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    int key = t * FK + kt2 * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    key = key < p.S ? key : p.S - 1;
                    st[kt2][i] += bp[(size_t)key * p.S] * isc;
                }
        }
        // ---- mask the ragged last tile ----
        if ((t + 1) * FK > p.S) {
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    int key = t * FK + kt2 * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (key >= p.S) st[kt2][i] = NEG_BIG;
                }
        }
        // ---- online softmax (log2 domain) ----
        float mx = st[0][0];
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, st[0][i]);
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, st[1][i]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, PRESCALED ? mx : mx * sc);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float pv = __builtin_amdgcn_exp2f(PRESCALED ? st[kt2][i] - m_new : st[kt2][i] * sc - m_new);
                st[kt2][i] = pv;
                psum += pv;
            }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o_acc[0][i] *= alpha; o_acc[1][i] *= alpha; }

        }

        // ---- O^T += V^T P^T : 2 d-tiles x (2 key sub-tiles x 2 k-steps) ----
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                bf16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (bf16_t)st[kt2][8 * s2 + j];
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const char* vp = base + vfo[dt] + (kt2 * 32 + s2 * 16) * 128;
                    short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(vp));
                    short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(vp + 8 * 128));
                    typedef __attribute__((ext_vector_type(8))) short short8v;
                    short8v v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, v8), pf, o_acc[dt], 0, 0, 0);
                }
            }
        }
        __syncthreads();       // its vmcnt(0) also retires the next tile's LDS-DMA
    }

    // ---- finalize: O = O^T / l, LSE ----
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    const int qrow = q0 + r;
    if (qrow < p.S) {
        bf16_t* op = p.o + (size_t)b * p.o_bs + (size_t)qrow * p.o_rs + head * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                u32x2 w;
                w[0] = pack2(o_acc[dt][4 * g4 + 0] * inv, o_acc[dt][4 * g4 + 1] * inv);
                w[1] = pack2(o_acc[dt][4 * g4 + 2] * inv, o_acc[dt][4 * g4 + 3] * inv);
                *(u32x2*)(op + dt * 32 + 8 * g4 + 4 * h) = w;
            }
        if (h == 0) p.lse2[((size_t)b * p.H + head) * p.S + qrow] = m_run + __builtin_amdgcn_logf(l_tot);
    }
}

// The lazy-max forward on 16 x 16 x 32 tiles, launched on request only (q_prescaled == 2, ops.attn_fwd(tiles16=True)).  Same cycles per flop
// as 32x32x16 and parity-clean.  Back to back in a loop (tools/kbench.py attn, B=1) it is 3.5 % FASTER than the 32x32x16 kernel (2.48 vs 2.57 ms);
// inside the training step (bench.py, B=4, same box, two rounds) it is 1.5 % SLOWER (9.09-9.15 vs 8.94-9.03 ms per launch): a 9-ms kernel
// between GEMMs does not sit in the clock regime of a sustained loop.  The step decides, so the training path stays on the kernel above.
// A wave owns 32 queries = two q-tiles; S^T tile (key-tile kt, q-tile qt): lane (g = lane >> 4,
// c = lane & 15) holds query 16 qt + c and keys 16 kt + 4 g + (0..3), so the row statistics are lane-local up to the four lane groups
// (combined only when a rescale happens and at the end).  P^T of two stacked key tiles, packed to bf16, is the B operand of
// O^T += V^T P^T (k-slot j of group g = key 4 g + j for j < 4, 16 + 4 g + j - 4 above); the V^T fragments follow that order through two
// transposed reads each.  K image: swizzle (key >> 1) & 7 (conflict-free 16-row ds_read_b128 fragments); V image: swizzle key & 6
// (conflict-free transposed reads of a 16 x 16 x 32 operand).
__global__ __launch_bounds__(256, 2) void attn_fwd_hd64_m16_kernel(AttnFwdParams p) {
    __shared__ __attribute__((aligned(16))) char smem[32768];   // 2 x (K 8 KiB + V 8 KiB)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4, ql = (lane & 15) >> 2, pl = lane & 3;
    const int nqt = (p.S + 127) / 128;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int qtb = id % nqt;
    const int bh = id / nqt;
    const int head = bh % p.H, b = bh / p.H;
    const int q0 = qtb * 128 + wave * 32;

    const bf16_t* qb = p.q + (size_t)b * p.q_bs + head * 64;
    const bf16_t* kb = p.k + (size_t)b * p.k_bs + head * 64;
    const bf16_t* vb = p.v + (size_t)b * p.v_bs + head * 64;
    __amdgpu_buffer_rsrc_t rk = make_rsrc(kb, (unsigned)((long long)(p.S - 1) * p.k_rs * 2 + 128));
    __amdgpu_buffer_rsrc_t rv = make_rsrc(vb, (unsigned)((long long)(p.S - 1) * p.v_rs * 2 + 128));

    // Q fragments (B operand of S^T = K Q^T): lane holds Q[q0 + 16 qt + c][32 s + 8 g .. + 7]
    bf16x8 qf[2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        int qrow = q0 + 16 * qt + c;
        if (qrow > p.S - 1) qrow = p.S - 1;       // clamp: rows past the end are computed but never stored
        const bf16_t* qp = qb + (size_t)qrow * p.q_rs + 8 * g;
#pragma unroll
        for (int s = 0; s < 2; ++s) qf[qt][s] = *(const bf16x8*)(qp + 32 * s);
    }
    // LDS-DMA staging: wave w moves the 1-KiB pieces w and w + 4 (8 keys x 128 B) of K and of V; the swizzle is applied to the SOURCE chunk
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    int kd_voff[2], vd_voff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int key = 8 * (wv + 4 * j) + (lane >> 3);
        kd_voff[j] = (int)(key * p.k_rs * 2) + (((lane & 7) ^ ((key >> 1) & 7)) << 4);
        vd_voff[j] = (int)(key * p.v_rs * 2) + (((lane & 7) ^ (key & 6)) << 4);
    }
    auto dma = [&](int t, int buf) {
        const int ks = (int)((long long)t * FK * p.k_rs * 2);
        const int vs = (int)((long long)t * FK * p.v_rs * 2);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            char* dst = smem + buf * 16384 + (wv + 4 * j) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (__attribute__((address_space(3))) void*)dst, 16, kd_voff[j], ks, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void*)(dst + 8192), 16, vd_voff[j], vs, 0, 0);
        }
    };
    int kfo[2];                                   // K fragment (key-tile at + 2048 kt), k-step s: row c, chunk 4 s + g
#pragma unroll
    for (int s = 0; s < 2; ++s) kfo[s] = c * 128 + (((4 * s + g) ^ ((c >> 1) & 7)) << 4);
    int vfo[4];                                   // V^T fragment of d-tile dt: block rows 4 g + ql (second block 16 rows further), k-step at + 4096 s'
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vfo[dt] = 8192 + (4 * g + ql) * 128 + (((2 * dt + (pl >> 1)) ^ ((4 * g + ql) & 6)) << 4) + (pl & 1) * 8;

    f32x4 o16[4][2];                              // O^T tiles [d-tile][q-tile]: lane holds d = 16 dt + 4 g + (0..3) of query 16 qt + c
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) o16[dt][qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run[2] = {0.f, 0.f}, l_run[2] = {0.f, 0.f};
    f32x4 negm[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    auto group_max = [&](float x) {               // over the four lane groups of a query column
        x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), 0x401F)));      // lane ^ 16
        return fmaxf(x, __shfl_xor(x, 32, 64));
    };

    const int nt = (p.S + FK - 1) / FK;
    dma(0, 0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) dma(t + 1, buf ^ 1);
        const char* base = smem + buf * 16384;
        f32x4 st[4][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const bf16x8 kf = *(const bf16x8*)(base + kt * 2048 + kfo[s]);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt)
                    st[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][s], s == 0 ? negm[qt] : st[kt][qt], 0, 0, 0);
            }
        if ((t + 1) * FK > p.S) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (t * FK + 16 * kt + 4 * g + i >= p.S) { st[kt][0][i] = NEG_BIG; st[kt][1][i] = NEG_BIG; }
        }
        float mx[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            mx[qt] = st[0][qt][0];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int i = 0; i < 4; ++i) mx[qt] = fmaxf(mx[qt], st[kt][qt][i]);
        }
        if (t == 0 || !__all(fmaxf(mx[0], mx[1]) <= LAZY_THR)) {            // wave-uniform; the lanes' partial maxima decide
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const float mq = group_max(mx[qt]);
                const float delta = (t == 0) ? mq : fmaxf(mq, 0.f);
                const float alpha = (t == 0) ? 1.0f : __builtin_amdgcn_exp2f(-delta);
                m_run[qt] += delta;
                l_run[qt] *= alpha;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) o16[dt][qt][i] *= alpha;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) st[kt][qt][i] -= delta;
#pragma unroll
                for (int i = 0; i < 4; ++i) negm[qt][i] = -m_run[qt];
            }
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float pv = __builtin_amdgcn_exp2f(st[kt][qt][i]);
                    st[kt][qt][i] = pv;
                    psum += pv;
                }
            l_run[qt] += psum;
        }
        // O^T += V^T P^T: two 32-key k-steps x four d-tiles x two q-tiles
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 pf[2];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int j = 0; j < 4; ++j) { pf[qt][j] = (bf16_t)st[2 * s2][qt][j]; pf[qt][4 + j] = (bf16_t)st[2 * s2 + 1][qt][j]; }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const char* vp = base + vfo[dt] + s2 * 4096;
                short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(vp));
                short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(vp + 2048));
                typedef __attribute__((ext_vector_type(8))) short short8v;
                short8v v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                const bf16x8 vt = __builtin_bit_cast(bf16x8, v8);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) o16[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt, pf[qt], o16[dt][qt], 0, 0, 0);
            }
        }
        __syncthreads();       // its vmcnt(0) also retires the next tile's LDS-DMA
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        float l_tot = l_run[qt];
        l_tot += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, l_tot), 0x401F));
        l_tot += __shfl_xor(l_tot, 32, 64);
        const float inv = 1.0f / l_tot;
        const int qrow = q0 + 16 * qt + c;
        if (qrow < p.S) {
            bf16_t* op = p.o + (size_t)b * p.o_bs + (size_t)qrow * p.o_rs + head * 64;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                u32x2 w;
                w[0] = pack2(o16[dt][qt][0] * inv, o16[dt][qt][1] * inv);
                w[1] = pack2(o16[dt][qt][2] * inv, o16[dt][qt][3] * inv);
                *(u32x2*)(op + 16 * dt + 4 * g) = w;
            }
            if (g == 0) p.lse2[((size_t)b * p.H + head) * p.S + qrow] = m_run[qt] + __builtin_amdgcn_logf(l_tot);
        }
    }
}

extern "C" int vt_attn_fwd_hd64(const void* q, const void* k, const void* v, void* o, float* lse2,
                                int B, int H, int S,
                                long long q_rs, long long k_rs, long long v_rs, long long o_rs,
                                long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                                float softmax_scale, int q_prescaled, void* stream) {
    if (B <= 0 || H <= 0 || S <= 0) return VT_ERR_BAD_SHAPE;
    if ((q_rs % 8) || (k_rs % 8) || (v_rs % 8) || (o_rs % 4) || (q_bs % 8) || (k_bs % 8) || (v_bs % 8) || (o_bs % 4))
        return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) return VT_ERR_BAD_ALIGN;
    if (((uintptr_t)o) & 7) return VT_ERR_BAD_ALIGN;
    if ((long long)S * k_rs * 2 >= 0x7fffffffLL || (long long)S * v_rs * 2 >= 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    AttnFwdParams p;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (bf16_t*)o; p.lse2 = lse2;
    p.S = S; p.H = H; p.B = B;
    p.q_rs = q_rs; p.k_rs = k_rs; p.v_rs = v_rs; p.o_rs = o_rs;
    p.q_bs = q_bs; p.k_bs = k_bs; p.v_bs = v_bs; p.o_bs = o_bs;
    p.scale_log2 = softmax_scale * 1.4426950408889634f;
    p.bias_t = nullptr;
    const int nqt = (S + FQ - 1) / FQ;
    if (q_prescaled == 2)      // the 16x16x32 variant on request (ops.attn_fwd(tiles16=True))
        hipLaunchKernelGGL(attn_fwd_hd64_m16_kernel, dim3(nqt * H * B), dim3(256), 0, (hipStream_t)stream, p);
    else if (q_prescaled) hipLaunchKernelGGL(attn_fwd_hd64_kernel<true>, dim3(nqt * H * B), dim3(FWD_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(attn_fwd_hd64_kernel<false>, dim3(nqt * H * B), dim3(FWD_THREADS), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// Same kernel with an additive score bias (fp32, transposed [H][S][S]: bias_t[h][key][q]), softmax(q k^T * scale + bias) v.
// Used by the frozen T5 text encoder (relative position bias, no scaling: softmax_scale = 1); no lse output is needed there
// lse2 is written as in vt_attn_fwd_hd64 (bias included).
extern "C" int vt_attn_fwd_bias_hd64(const void* q, const void* k, const void* v, const float* bias_t, void* o, float* lse2,
                                     int B, int H, int S,
                                     long long q_rs, long long k_rs, long long v_rs, long long o_rs,
                                     long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                                     float softmax_scale, void* stream) {
    if (B <= 0 || H <= 0 || S <= 0 || bias_t == nullptr || lse2 == nullptr || !(softmax_scale > 0.f)) return VT_ERR_BAD_SHAPE;
    if ((q_rs % 8) || (k_rs % 8) || (v_rs % 8) || (o_rs % 4) || (q_bs % 8) || (k_bs % 8) || (v_bs % 8) || (o_bs % 4))
        return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) return VT_ERR_BAD_ALIGN;
    if ((((uintptr_t)o) & 7) || (((uintptr_t)bias_t) & 3)) return VT_ERR_BAD_ALIGN;
    if ((long long)S * k_rs * 2 >= 0x7fffffffLL || (long long)S * v_rs * 2 >= 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    AttnFwdParams p;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (bf16_t*)o; p.lse2 = lse2;
    p.S = S; p.H = H; p.B = B;
    p.q_rs = q_rs; p.k_rs = k_rs; p.v_rs = v_rs; p.o_rs = o_rs;
    p.q_bs = q_bs; p.k_bs = k_bs; p.v_bs = v_bs; p.o_bs = o_bs;
    p.scale_log2 = softmax_scale * 1.4426950408889634f;
    p.bias_t = bias_t;
    const int nqt = (S + FQ - 1) / FQ;
    hipLaunchKernelGGL((attn_fwd_hd64_kernel<false, true>), dim3(nqt * H * B), dim3(FWD_THREADS), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
