// Dual-context cross-attention of DynamiCrafter's spatial transformer blocks (lvdm/modules/attention.py:45-170, CrossAttention with
// img_cross_attention=True), head_dim 64, forward and backward, gfx950:
//     o = softmax(q K_a^T s) V_a  +  img_scale * softmax(q K_b^T s) V_b
// Two SEPARATE softmaxes share q: segment a = the sample's text keys (Sa <= 96, the same for every frame), segment b = the image keys
// of the query's FRAME (Sb <= 32; rows [f*rpf, (f+1)*rpf) of sample b meet image item b*nf + f, nf = Sq / rpf).  The context that is
// not 77 + t*16 long -- one image set for all frames -- is the same launch with rpf = Sq.
//
// Built on attn_small.hip's scheme (every key resident in LDS, single-pass softmax, S^T = K Q^T with the query on the lane in the
// forward, the key on the lane in the backward).  What is new:
//   * key slots: the text keys fill tiles [0, NA) (NA = ceil(Sa / 32), padded with zero keys), the image keys are tile NA.  A segment
//     is a whole number of 32-key MFMA tiles, so per-segment row maximum / sum are sums over whole accumulators: lane-local + the
//     cross-half shuffle, no extra masks.  Two log-sum-exp planes are kept, lse2[seg][b][h][row].
//   * tile / frame rule: a workgroup works on rows of ONE frame (blockIdx.x = frame * chunks-per-frame + chunk, chunks start at
//     multiples of 32 rows inside the frame, the last one is partial), so a 32-row query tile never meets two frames' image keys and
//     rpf need not be a multiple of 32.
//   * backward: only the summed o is stored, so the usual delta = rowsum(dO * O) is NOT the softmax-backward constant of either
//     segment (it is D_a + D_b).  D_a = rowsum(P_a * dP_a) and D_b = rowsum(P_b * dP_b) are formed in the kernel: a first pass computes
//     S^T and dP^T with the query on the lane (the same operand registers as S and dP, swapped), where the row sums are lane-local
//     plus one cross-half shuffle; o is not read at all.  The second pass is attn_small's (key on the lane) with per-segment lse and D.
//     img_scale is folded into P_b there (dV_b = (c P_b)^T dO, dS_b = (c P_b) * (dP_b - D_b)), so img_scale = 0 gives exact zeros.
//   * dK / dV without atomics: the four waves of a workgroup are summed through LDS in wave order, the workgroup stores one fp32
//     partial per chunk, and ad_reduce_kernel adds the chunks of a sample (text) / of a frame (image) in chunk order: two launches of
//     the same inputs give the same bits.  A frame of <= 1024 rows is one chunk and its image partial IS the result.
#include "attn_small.h"

#define AD_MAXA 96
#define AD_MAXB 32
#define AD_BWD_CHUNK 1024

struct AttnDualParams {
    const bf16_t* q; const bf16_t* ka; const bf16_t* va; const bf16_t* kb; const bf16_t* vb; const bf16_t* dout;
    bf16_t* out; float* lse2; bf16_t* dq;
    float* tk; float* tv; float* ik; float* iv;          // fp32 partials: text [B][nf*cpf][Sa][H*64], image [B*nf][cpf][Sb][H*64]
    long long q_rs, q_bs, ka_rs, ka_bs, va_rs, va_bs, kb_rs, kb_bs, vb_rs, vb_bs, o_rs, o_bs, do_rs, do_bs, dq_rs, dq_bs;
    int B, H, Sq, rpf, nf, Sa, Sb, chunk, cpf;
    float scale2;            // softmax_scale * log2(e)
    float scale, img_scale;
};

// stage the key slots of one (sample, frame, head): K row-major and, optionally, V row-major / K^T / V^T.  Slot < NA*32: text key (zeros
// from Sa on); slot NA*32 + j: image key j (zeros from Sb on).
template <int NA, bool WANT_VROW, bool WANT_KT, bool WANT_VT>
__device__ __forceinline__ void ad_stage_kv(const AttnDualParams& p, const bf16_t* ka, const bf16_t* va, const bf16_t* kb, const bf16_t* vb, char* Ks,
                                            char* Vs, char* Kt, char* Vt) {
    constexpr int SKP = (NA + 1) * 32;
    const int tid = threadIdx.x;
    for (int i = tid; i < SKP * 8; i += 256) {
        const int key = i >> 3, ch = i & 7;
        u32x4 kk = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
        if (key < NA * 32) {
            if (key < p.Sa) {
                kk = *(const u32x4*)(ka + (long long)key * p.ka_rs + ch * 8);
                vv = *(const u32x4*)(va + (long long)key * p.va_rs + ch * 8);
            }
        } else if (key - NA * 32 < p.Sb) {
            kk = *(const u32x4*)(kb + (long long)(key - NA * 32) * p.kb_rs + ch * 8);
            vv = *(const u32x4*)(vb + (long long)(key - NA * 32) * p.vb_rs + ch * 8);
        }
        *(u32x4*)(Ks + key * AS_KROW + ch * 16) = kk;
        if (WANT_VROW) *(u32x4*)(Vs + key * AS_KROW + ch * 16) = vv;
        if (WANT_KT) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *(unsigned short*)(Kt + (ch * 8 + e) * AS_TROW(SKP) + key * 2) = (unsigned short)((kk[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        }
        if (WANT_VT) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *(unsigned short*)(Vt + (ch * 8 + e) * AS_TROW(SKP) + key * 2) = (unsigned short)((vv[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        }
    }
}

// ============================================================================================================ forward
template <int NA>
__global__ __launch_bounds__(256, 2) void attn_dual_fwd_kernel(AttnDualParams p) {
    constexpr int NKT = NA + 1, SKP = NKT * 32;
    __shared__ __attribute__((aligned(16))) char Ks[SKP * AS_KROW];
    __shared__ __attribute__((aligned(16))) char Vt[64 * AS_TROW(SKP)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.y, b = blockIdx.z;
    const int f = blockIdx.x / p.cpf, c = blockIdx.x - f * p.cpf;
    const int r0 = c * p.chunk;                                      // first row of this workgroup inside the frame (chunk = 128)
    const int nq = min(p.chunk, p.rpf - r0);
    const long long row0 = (long long)f * p.rpf + r0;                // ... inside the sample
    const long long item = (long long)b * p.nf + f;                  // image item of this frame
    ad_stage_kv<NA, false, false, true>(p, p.ka + (long long)b * p.ka_bs + h * 64, p.va + (long long)b * p.va_bs + h * 64,
                                        p.kb + item * p.kb_bs + h * 64, p.vb + item * p.vb_bs + h * 64, Ks, nullptr, nullptr, Vt);
    __syncthreads();
    const int ql = lane & 31, hh = lane >> 5;
    const int qi = wave * 32 + ql;
    const bool qok = qi < nq;
    const bf16_t* qp = p.q + (long long)b * p.q_bs + (row0 + qi) * p.q_rs + h * 64;
    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        u32x4 t = {0u, 0u, 0u, 0u};
        if (qok) t = *(const u32x4*)(qp + ks * 16 + hh * 8);
        qf[ks] = __builtin_bit_cast(bf16x8, t);
    }
    f32x16 s[NKT];
    float mx[2] = {-1e30f, -1e30f};
#pragma unroll
    for (int a = 0; a < NKT; ++a) {
        const int seg = a == NA ? 1 : 0;
        const int nk = seg ? p.Sb : p.Sa - a * 32;                   // valid keys of this tile
#pragma unroll
        for (int e = 0; e < 16; ++e) s[a][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 kf = *(const bf16x8*)(Ks + (a * 32 + ql) * AS_KROW + ks * 32 + hh * 16);
            s[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[a], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[a][r] = as_crow(r, hh) < nk ? s[a][r] * p.scale2 : -1e30f;
            mx[seg] = fmaxf(mx[seg], s[a][r]);
        }
    }
    float sum[2] = {0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 2; ++g) mx[g] = fmaxf(mx[g], __shfl_xor(mx[g], 32, 64));
#pragma unroll
    for (int a = 0; a < NKT; ++a) {
        const int seg = a == NA ? 1 : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = s[a][r] > -1e29f ? __builtin_amdgcn_exp2f(s[a][r] - mx[seg]) : 0.f;
            s[a][r] = e;
            sum[seg] += e;
        }
    }
    float inv[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        sum[g] += __shfl_xor(sum[g], 32, 64);
        inv[g] = sum[g] > 0.f ? 1.0f / sum[g] : 0.f;
        if (hh == 0 && qok && p.lse2 != nullptr)
            p.lse2[(((long long)g * p.B + b) * p.H + h) * p.Sq + row0 + qi] = mx[g] + __builtin_amdgcn_logf(sum[g]);       // v_log_f32 = log2
    }
    inv[1] *= p.img_scale;
    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
#pragma unroll
    for (int a = 0; a < NKT; ++a) {
        const int seg = a == NA ? 1 : 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[a][e] *= inv[seg];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const bf16x8 pf = as_pack8(s[a], s2);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 vf = as_tfrag(Vt + (dt * 32 + ql) * AS_TROW(SKP) + a * 64, s2, hh);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, o[dt], 0, 0, 0);
            }
        }
    }
    bf16_t* ob = p.out + (long long)b * p.o_bs + row0 * p.o_rs + h * 64;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = wave * 32 + as_crow(r, hh);
            if (qr < nq) ob[(long long)qr * p.o_rs + dt * 32 + ql] = (bf16_t)o[dt][r];
        }
}

// ============================================================================================================ backward
template <int NA>
__global__ __launch_bounds__(256, 1) void attn_dual_bwd_kernel(AttnDualParams p) {
    constexpr int NKT = NA + 1, SKP = NKT * 32;
    constexpr int TR = AS_TROW(SKP);
    constexpr int WVB = 64 * 80 * 2 + 32 * TR + 512;                 // per wave: Q^T | dO^T | dS | lse_a, lse_b, D_a, D_b
    constexpr int REDB = 4 * 4 * 32 * 32 * 4;                        // cross-wave sum of one key tile: [wave][dK, dV x 2 d-halves][32][32] fp32
    __shared__ __attribute__((aligned(16))) char Ks[SKP * AS_KROW];
    __shared__ __attribute__((aligned(16))) char Vs[SKP * AS_KROW];
    __shared__ __attribute__((aligned(16))) char Kt[64 * TR];
    __shared__ __attribute__((aligned(16))) char Wv[4 * WVB > REDB ? 4 * WVB : REDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.y, b = blockIdx.z;
    const int f = blockIdx.x / p.cpf, c = blockIdx.x - f * p.cpf;
    const int r0 = c * p.chunk;                                      // chunk is a multiple of 32: tiles never straddle a frame
    const int nq = min(p.chunk, p.rpf - r0);
    const long long row0 = (long long)f * p.rpf + r0;
    const long long item = (long long)b * p.nf + f;
    ad_stage_kv<NA, true, true, false>(p, p.ka + (long long)b * p.ka_bs + h * 64, p.va + (long long)b * p.va_bs + h * 64,
                                       p.kb + item * p.kb_bs + h * 64, p.vb + item * p.vb_bs + h * 64, Ks, Vs, Kt, nullptr);
    __syncthreads();
    const int ql = lane & 31, hh = lane >> 5;
    char* Qt = Wv + wave * WVB;
    char* dOt = Qt + 64 * 80;
    char* dSs = dOt + 64 * 80;
    float* stat = (float*)(dSs + 32 * TR);            // [0,32): lse_a, [32,64): lse_b, [64,96): D_a, [96,128): D_b
    const long long qoff = (long long)b * p.q_bs + row0 * p.q_rs;
    const long long dooff = (long long)b * p.do_bs + row0 * p.do_rs;
    const long long dqoff = (long long)b * p.dq_bs + row0 * p.dq_rs;
    const long long lse_off = ((long long)b * p.H + h) * p.Sq + row0;
    const long long lse_seg = (long long)p.B * p.H * p.Sq;

    f32x16 dK[NKT][2], dV[NKT][2];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { dK[kt][dt][e] = 0.f; dV[kt][dt][e] = 0.f; }

    const int ntile = (nq + 31) / 32;
    for (int qt = wave; qt < ntile; qt += 4) {
        const int qi = qt * 32 + ql;
        const bool qok = qi < nq;
        bf16x8 qf[4], dof[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 tq = {0u, 0u, 0u, 0u}, td = {0u, 0u, 0u, 0u};
            if (qok) {
                tq = *(const u32x4*)(p.q + qoff + (long long)qi * p.q_rs + h * 64 + ks * 16 + hh * 8);
                td = *(const u32x4*)(p.dout + dooff + (long long)qi * p.do_rs + h * 64 + ks * 16 + hh * 8);
            }
            qf[ks] = __builtin_bit_cast(bf16x8, tq);
            dof[ks] = __builtin_bit_cast(bf16x8, td);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int d = ks * 16 + hh * 8 + e;
                *(unsigned short*)(Qt + d * 80 + ql * 2) = (unsigned short)((tq[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
                *(unsigned short*)(dOt + d * 80 + ql * 2) = (unsigned short)((td[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
            }
        }
        // ---- pass 1, query on the lane: D_seg = rowsum(P_seg * dP_seg) ----
        float ls[2] = {0.f, 0.f}, dl[2] = {0.f, 0.f};
        if (qok) {
            ls[0] = p.lse2[lse_off + qi];
            ls[1] = p.lse2[lse_seg + lse_off + qi];
        }
#pragma unroll
        for (int a = 0; a < NKT; ++a) {
            const int seg = a == NA ? 1 : 0;
            const int nk = seg ? p.Sb : p.Sa - a * 32;
            f32x16 St, dPt;
#pragma unroll
            for (int e = 0; e < 16; ++e) { St[e] = 0.f; dPt[e] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = *(const bf16x8*)(Ks + (a * 32 + ql) * AS_KROW + ks * 32 + hh * 16);
                const bf16x8 vf = *(const bf16x8*)(Vs + (a * 32 + ql) * AS_KROW + ks * 32 + hh * 16);
                St = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], St, 0, 0, 0);            // [key rows][query cols]
                dPt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[ks], dPt, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pr = as_crow(r, hh) < nk ? __builtin_amdgcn_exp2f(St[r] * p.scale2 - ls[seg]) : 0.f;
                dl[seg] = __builtin_fmaf(pr, dPt[r], dl[seg]);
            }
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            dl[g] += __shfl_xor(dl[g], 32, 64);
            if (hh == 0) {
                stat[g * 32 + ql] = ls[g];
                stat[64 + g * 32 + ql] = dl[g];
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- pass 2, key on the lane: P^T and dS^T feed dV and dK from registers ----
#pragma unroll
        for (int a = 0; a < NKT; ++a) {
            const int seg = a == NA ? 1 : 0;
            f32x16 S, dP;
#pragma unroll
            for (int e = 0; e < 16; ++e) { S[e] = 0.f; dP[e] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = *(const bf16x8*)(Ks + (a * 32 + ql) * AS_KROW + ks * 32 + hh * 16);
                const bf16x8 vf = *(const bf16x8*)(Vs + (a * 32 + ql) * AS_KROW + ks * 32 + hh * 16);
                S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], kf, S, 0, 0, 0);          // [query rows][key cols]
                dP = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof[ks], vf, dP, 0, 0, 0);
            }
            const int key = a * 32 + ql;
            const bool kok = seg ? ql < p.Sb : key < p.Sa;
            const float pscale = seg ? p.img_scale : 1.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = as_crow(r, hh);
                const bool ok = kok && (qt * 32 + qr) < nq;
                const float pr = ok ? pscale * __builtin_amdgcn_exp2f(S[r] * p.scale2 - stat[seg * 32 + qr]) : 0.f;
                S[r] = pr;
                dP[r] = pr * (dP[r] - stat[64 + seg * 32 + qr]) * p.scale;
                *(unsigned short*)(dSs + qr * TR + key * 2) = __builtin_bit_cast(unsigned short, (bf16_t)dP[r]);
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8 pf = as_pack8(S, s2), dsf = as_pack8(dP, s2);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const bf16x8 dob = as_tfrag(dOt + (dt * 32 + ql) * 80, s2, hh);
                    const bf16x8 qb = as_tfrag(Qt + (dt * 32 + ql) * 80, s2, hh);
                    dV[a][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, dob, dV[a][dt], 0, 0, 0);    // [key rows][d cols]
                    dK[a][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsf, qb, dK[a][dt], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // dQ[32 q][64 d] = dS K over both segments' key slots
        f32x16 dQ[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) dQ[dt][e] = 0.f;
#pragma unroll
        for (int s = 0; s < SKP / 16; ++s) {
            const bf16x8 af = *(const bf16x8*)(dSs + ql * TR + (s * 16 + hh * 8) * 2);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 bfk = *(const bf16x8*)(Kt + (dt * 32 + ql) * TR + (s * 16 + hh * 8) * 2);
                dQ[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfk, dQ[dt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = qt * 32 + as_crow(r, hh);
                if (qr < nq) p.dq[dqoff + (long long)qr * p.dq_rs + h * 64 + dt * 32 + ql] = (bf16_t)dQ[dt][r];
            }
        __builtin_amdgcn_wave_barrier();
    }
    // ---- dK / dV of this chunk: the four waves are added through LDS in wave order, one plain fp32 store per element ----
    float* red = (float*)Wv;
    const int D = p.H * 64;
    const long long tbase = ((long long)b * p.nf * p.cpf + blockIdx.x) * p.Sa;     // text partial of (sample, chunk)
    const long long ibase = (item * p.cpf + c) * p.Sb;                             // image partial of (frame, chunk)
#pragma unroll
    for (int a = 0; a < NKT; ++a) {
        __syncthreads();
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int at = as_crow(r, hh) * 32 + ql;
                red[((wave * 4 + dt) * 32 * 32) + at] = dK[a][dt][r];
                red[((wave * 4 + 2 + dt) * 32 * 32) + at] = dV[a][dt][r];
            }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int e = j * 256 + tid;                  // [dK d-half 0, 1 | dV d-half 0, 1][key 32][d 32]
            const float v = ((red[e] + red[4096 + e]) + red[8192 + e]) + red[12288 + e];
            const int plane = e >> 10, kl = (e >> 5) & 31, col = h * 64 + (plane & 1) * 32 + (e & 31);
            if (a < NA) {
                const int key = a * 32 + kl;
                if (key < p.Sa) ((plane >> 1) ? p.tv : p.tk)[(tbase + key) * D + col] = v;
            } else if (kl < p.Sb) {
                ((plane >> 1) ? p.iv : p.ik)[(ibase + kl) * D + col] = v;
            }
        }
    }
}

// out[item][e] = sum over the nch chunks of the item, in chunk order (per = floats of one partial, a multiple of 4)
__global__ __launch_bounds__(256) void ad_reduce_kernel(const float* part, float* out, int nch, long long per) {
    const long long e4 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e4 * 4 >= per) return;
    const float* src = part + (long long)blockIdx.y * nch * per + e4 * 4;
    f32x4 acc = *(const f32x4*)src;
    for (int i = 1; i < nch; ++i) acc += *(const f32x4*)(src + (long long)i * per);
    *(f32x4*)(out + (long long)blockIdx.y * per + e4 * 4) = acc;
}

static int ad_check(const void* const* ptrs, int nptr, int B, int H, int Sq, int rpf, int Sa, int Sb, const long long* strides, int nstr) {
    if (B <= 0 || H <= 0 || Sq <= 0 || rpf <= 0 || Sq % rpf || Sa <= 0 || Sa > AD_MAXA || Sb <= 0 || Sb > AD_MAXB) return VT_ERR_BAD_SHAPE;
    if (B > 65535 || H > 65535) return VT_ERR_BAD_SHAPE;
    for (int i = 0; i < nstr; ++i)
        if (strides[i] % 8) return VT_ERR_BAD_SHAPE;
    for (int i = 0; i < nptr; ++i)
        if (ptrs[i] == nullptr || (((uintptr_t)ptrs[i]) & 15)) return VT_ERR_BAD_ALIGN;
    return VT_OK;
}

static void ad_bwd_chunks(int rpf, int* chunk, int* cpf) {
    *cpf = (rpf + AD_BWD_CHUNK - 1) / AD_BWD_CHUNK;
    *chunk = (((rpf + *cpf - 1) / *cpf) + 31) / 32 * 32;
    *cpf = (rpf + *chunk - 1) / *chunk;
}

// fp32 elements of the backward's partial-sum workspace (0: every key set is met by one workgroup per head, nothing to add up)
extern "C" long long vt_attn_dual_ws_floats(int B, int H, int Sq, int rows_per_frame, int Sa, int Sb) {
    if (B <= 0 || H <= 0 || Sq <= 0 || rows_per_frame <= 0 || Sq % rows_per_frame) return -1;
    int chunk, cpf;
    ad_bwd_chunks(rows_per_frame, &chunk, &cpf);
    const long long nf = Sq / rows_per_frame, D = (long long)H * 64;
    long long n = 0;
    if (nf * cpf > 1) n += 2 * (long long)B * nf * cpf * Sa * D;
    if (cpf > 1) n += 2 * (long long)B * nf * cpf * Sb * D;
    return n;
}

// Element (sample b, row s, head h, d) of q / o at base + b*bs + s*rs + h*64 + d; text k / v [B, Sa, .] and image k_ip / v_ip
// [B * Sq / rows_per_frame, Sb, .] likewise with their strides.  lse2: fp32 [2, B, H, Sq] (text plane, image plane; log2 domain).
extern "C" int vt_attn_dual_fwd(const void* q, const void* k, const void* v, const void* k_ip, const void* v_ip, void* o, float* lse2,
                                int B, int H, int Sq, int rows_per_frame, int Sa, int Sb,
                                long long q_rs, long long q_bs, long long k_rs, long long k_bs, long long v_rs, long long v_bs,
                                long long kip_rs, long long kip_bs, long long vip_rs, long long vip_bs, long long o_rs, long long o_bs,
                                float softmax_scale, float img_scale, void* stream) {
    const long long st[12] = {q_rs, q_bs, k_rs, k_bs, v_rs, v_bs, kip_rs, kip_bs, vip_rs, vip_bs, o_rs, o_bs};
    const void* const ptrs[6] = {q, k, v, k_ip, v_ip, o};
    int rc = ad_check(ptrs, 6, B, H, Sq, rows_per_frame, Sa, Sb, st, 12);
    if (rc != VT_OK) return rc;
    AttnDualParams p = {};
    p.q = (const bf16_t*)q; p.ka = (const bf16_t*)k; p.va = (const bf16_t*)v; p.kb = (const bf16_t*)k_ip; p.vb = (const bf16_t*)v_ip;
    p.out = (bf16_t*)o; p.lse2 = lse2;
    p.q_rs = q_rs; p.q_bs = q_bs; p.ka_rs = k_rs; p.ka_bs = k_bs; p.va_rs = v_rs; p.va_bs = v_bs;
    p.kb_rs = kip_rs; p.kb_bs = kip_bs; p.vb_rs = vip_rs; p.vb_bs = vip_bs; p.o_rs = o_rs; p.o_bs = o_bs;
    p.B = B; p.H = H; p.Sq = Sq; p.rpf = rows_per_frame; p.nf = Sq / rows_per_frame; p.Sa = Sa; p.Sb = Sb;
    p.chunk = 128; p.cpf = (rows_per_frame + 127) / 128;
    p.scale = softmax_scale; p.scale2 = softmax_scale * 1.4426950408889634f; p.img_scale = img_scale;
    const dim3 grid((unsigned)(p.nf * p.cpf), H, B);
    hipStream_t s = (hipStream_t)stream;
    const int na = (Sa + 31) / 32;
    if (na == 1) hipLaunchKernelGGL((attn_dual_fwd_kernel<1>), grid, dim3(256), 0, s, p);
    else if (na == 2) hipLaunchKernelGGL((attn_dual_fwd_kernel<2>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((attn_dual_fwd_kernel<3>), grid, dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// dq bf16 like q.  dk32, dv32 fp32 [B, Sa, H*64] and dkip32, dvip32 fp32 [B * Sq / rows_per_frame, Sb, H*64], contiguous, fully
// written (no zeroing by the caller).  ws: vt_attn_dual_ws_floats(...) fp32 elements of scratch (may be NULL when that is 0).
extern "C" int vt_attn_dual_bwd(const void* q, const void* k, const void* v, const void* k_ip, const void* v_ip, const void* dout,
                                const float* lse2, void* dq, float* dk32, float* dv32, float* dkip32, float* dvip32, float* ws,
                                long long ws_floats, int B, int H, int Sq, int rows_per_frame, int Sa, int Sb,
                                long long q_rs, long long q_bs, long long k_rs, long long k_bs, long long v_rs, long long v_bs,
                                long long kip_rs, long long kip_bs, long long vip_rs, long long vip_bs, long long do_rs, long long do_bs,
                                long long dq_rs, long long dq_bs, float softmax_scale, float img_scale, void* stream) {
    const long long st[14] = {q_rs, q_bs, k_rs, k_bs, v_rs, v_bs, kip_rs, kip_bs, vip_rs, vip_bs, do_rs, do_bs, dq_rs, dq_bs};
    const void* const ptrs[12] = {q, k, v, k_ip, v_ip, dout, lse2, dq, dk32, dv32, dkip32, dvip32};
    int rc = ad_check(ptrs, 12, B, H, Sq, rows_per_frame, Sa, Sb, st, 14);
    if (rc != VT_OK) return rc;
    const long long need = vt_attn_dual_ws_floats(B, H, Sq, rows_per_frame, Sa, Sb);
    if (need > 0 && (ws == nullptr || ws_floats < need || (((uintptr_t)ws) & 15))) return VT_ERR_BAD_SHAPE;
    AttnDualParams p = {};
    p.q = (const bf16_t*)q; p.ka = (const bf16_t*)k; p.va = (const bf16_t*)v; p.kb = (const bf16_t*)k_ip; p.vb = (const bf16_t*)v_ip;
    p.dout = (const bf16_t*)dout; p.lse2 = const_cast<float*>(lse2); p.dq = (bf16_t*)dq;
    p.q_rs = q_rs; p.q_bs = q_bs; p.ka_rs = k_rs; p.ka_bs = k_bs; p.va_rs = v_rs; p.va_bs = v_bs;
    p.kb_rs = kip_rs; p.kb_bs = kip_bs; p.vb_rs = vip_rs; p.vb_bs = vip_bs; p.do_rs = do_rs; p.do_bs = do_bs; p.dq_rs = dq_rs; p.dq_bs = dq_bs;
    p.B = B; p.H = H; p.Sq = Sq; p.rpf = rows_per_frame; p.nf = Sq / rows_per_frame; p.Sa = Sa; p.Sb = Sb;
    ad_bwd_chunks(rows_per_frame, &p.chunk, &p.cpf);
    p.scale = softmax_scale; p.scale2 = softmax_scale * 1.4426950408889634f; p.img_scale = img_scale;
    const long long D = (long long)H * 64, nch = (long long)p.nf * p.cpf;
    const long long tper = (long long)Sa * D, iper = (long long)Sb * D;
    const bool tred = nch > 1, ired = p.cpf > 1;
    float* w = ws;
    p.tk = dk32; p.tv = dv32; p.ik = dkip32; p.iv = dvip32;
    if (tred) { p.tk = w; w += B * nch * tper; p.tv = w; w += B * nch * tper; }
    if (ired) { p.ik = w; w += B * nch * iper; p.iv = w; w += B * nch * iper; }
    if (nch > 0x7fffffffLL || B * (long long)p.nf > 65535) return VT_ERR_BAD_SHAPE;
    const dim3 grid((unsigned)nch, H, B);
    hipStream_t s = (hipStream_t)stream;
    const int na = (Sa + 31) / 32;
    if (na == 1) hipLaunchKernelGGL((attn_dual_bwd_kernel<1>), grid, dim3(256), 0, s, p);
    else if (na == 2) hipLaunchKernelGGL((attn_dual_bwd_kernel<2>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((attn_dual_bwd_kernel<3>), grid, dim3(256), 0, s, p);
    if (tred) {
        const dim3 g((unsigned)((tper / 4 + 255) / 256), B);
        hipLaunchKernelGGL(ad_reduce_kernel, g, dim3(256), 0, s, p.tk, dk32, (int)nch, tper);
        hipLaunchKernelGGL(ad_reduce_kernel, g, dim3(256), 0, s, p.tv, dv32, (int)nch, tper);
    }
    if (ired) {
        const dim3 g((unsigned)((iper / 4 + 255) / 256), (unsigned)(B * p.nf));
        hipLaunchKernelGGL(ad_reduce_kernel, g, dim3(256), 0, s, p.ik, dkip32, p.cpf, iper);
        hipLaunchKernelGGL(ad_reduce_kernel, g, dim3(256), 0, s, p.iv, dvip32, p.cpf, iper);
    }
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
