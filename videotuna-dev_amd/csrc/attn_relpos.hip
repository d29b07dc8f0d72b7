// Packed temporal self-attention with LEARNED RELATIVE-POSITION tables, head_dim 64, forward and backward, gfx950.
// User: both attentions of TemporalTransformer when the UNet is built with use_relative_position=True -- the VideoCrafter1 / LVDM
// layout (lvdm/modules/attention.py:19-42 RelativePosition, :126-149 the relative_position branch of CrossAttention.forward).  For one
// sequence of T rows and one head, with idx(i, j) = clamp(j - i, -P, P) + P and two tables Ek, Ev [2P+1, 64] shared by all heads:
//     S[i,j] = scale (q_i . k_j + q_i . Ek[idx]),   p = softmax_j S,   o_i = sum_j p[i,j] (v_j + Ev[idx])
//
// Packing is attn_small's masked mode (attn_small.hip is not touched: the shipped VideoCrafter2 path stays the same code): the R rows are
// R / T consecutive sequences, 32 / T of them fill a 32-row tile that attends to itself under a block-diagonal mask, one tile per wave,
// 128 rows (an "item") per workgroup pass.  q, k, v, o, dO are read once; a workgroup walks items x heads with a grid stride, so the
// tables are staged once per workgroup and the table gradients stay in registers until the workgroup is done.
//
// The table terms are MFMA products of SKEWED matrices.  Inside a sequence only the 2T-1 <= 63 distances w = j - i + T - 1 occur, so the
// workgroup stages the EXPANDED tables EkX[w] = Ek[clamp(w - (T-1), -P, P) + P] (the clamp is applied here and nowhere else) and
//     Rk = Q EkX^T [32, 64]           S[i,j]  += Rk[i, w(i,j)]
//     Pskew[i,w] = p[i,j]             o       += Pskew EvX        dEvX = Pskew^T dO      dP[i,j] += (dO EvX^T)[i, w(i,j)]
//     dSskew[i,w] = dS[i,j]           dQ      += dSskew EkX       dEkX = dSskew^T Q
// The skew maps a (lane, register) pair to a column that depends on the lane; it goes through a per-wave LDS tile (fp32 for the score
// terms, bf16 operand images for the products), never through a runtime-indexed register array.
//
// Table gradients: every wave accumulates dEkX / dEvX of all its tiles in MFMA accumulators; at the end the four waves add them into one
// LDS tile, the workgroup adds that tile with fp32 atomics into one of RP_COPIES zeroed copies of the expanded tables in the workspace
// (RP_COPIES * 2 * 64 * 64 floats: independent of R and P), and a small kernel sums the copies, folds the clamped distances and ADDS into
// d_rel_k / d_rel_v.  Because of the fp32 atomics the table gradients are NOT bitwise reproducible from run to run (dq / dk / dv are).
#include "attn_small.h"

#define RP_COPIES 32
#define RP_WS_FLOATS (RP_COPIES * 2 * 64 * 64)
#define RP_QROW 80           // bytes per row of a per-wave transposed image [64 d][32 rows + 8]

struct RelposParams {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* o; const bf16_t* dout; const bf16_t* rel_k; const bf16_t* rel_v;
    bf16_t* out; float* lse2;
    bf16_t* dq; bf16_t* dk; bf16_t* dv; float* ws;
    long long q_rs, k_rs, v_rs, o_rs, do_rs, dq_rs, dk_rs, dv_rs;
    int R, H, T, tsh, P, nitems, want_tables;
    float scale2;            // softmax_scale * log2(e)
    float scale;
};

// expanded tables of the distances w = j - i + T - 1 in [0, 2T-1); rows past 2T-2 are zeros.  Row-major images [NW][64 + 8] and
// transposed images [64][NW + 8]
template <int NWT, bool ROWK, bool ROWV, bool TRK, bool TRV>
__device__ __forceinline__ void rp_stage_tables(const RelposParams& p, char* EkX, char* EvX, char* EkXT, char* EvXT) {
    constexpr int NW = NWT * 32, PST = (NW + 8) * 2;
    for (int i = threadIdx.x; i < NW * 8; i += 256) {
        const int w = i >> 3, ch = i & 7;
        u32x4 kk = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
        if (w < 2 * p.T - 1) {
            const int row = min(max(w - (p.T - 1), -p.P), p.P) + p.P;
            kk = *(const u32x4*)(p.rel_k + (long long)row * 64 + ch * 8);
            vv = *(const u32x4*)(p.rel_v + (long long)row * 64 + ch * 8);
        }
        if (ROWK) *(u32x4*)(EkX + w * AS_KROW + ch * 16) = kk;
        if (ROWV) *(u32x4*)(EvX + w * AS_KROW + ch * 16) = vv;
        if (TRK) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *(unsigned short*)(EkXT + (ch * 8 + e) * PST + w * 2) = (unsigned short)((kk[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        }
        if (TRV) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *(unsigned short*)(EvXT + (ch * 8 + e) * PST + w * 2) = (unsigned short)((vv[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
        }
    }
}

__device__ __forceinline__ void rp_zero16(char* base, int bytes, int lane) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int i = lane * 16; i < bytes; i += 64 * 16) *(u32x4*)(base + i) = z;
}

__device__ __forceinline__ void rp_scatter8(char* img, const u32x4& t, int d0, int col) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
        *(unsigned short*)(img + (d0 + e) * RP_QROW + col * 2) = (unsigned short)((t[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
}

// ============================================================================================================ forward
// NWT: 32-column tiles of the expanded tables (1: T <= 16, 2: T = 32)
template <int NWT>
__global__ __launch_bounds__(256, 2) void attn_relpos_fwd_kernel(RelposParams p) {
    constexpr int NW = NWT * 32;
    constexpr int RST = NW + 1;                  // floats per row of the fp32 skew tile [32 q][NW]
    constexpr int PST = (NW + 8) * 2;            // bytes per row of a bf16 image with NW columns
    __shared__ __attribute__((aligned(16))) char EkX[NW * AS_KROW];
    __shared__ __attribute__((aligned(16))) char EvXT[64 * PST];
    __shared__ __attribute__((aligned(16))) char Wv[4][64 * RP_QROW + 32 * RST * 4];        // per wave: V^T | skew tile (Rk fp32, then Pskew bf16)
    static_assert(32 * RST * 4 >= 32 * PST && (32 * RST * 4) % 16 == 0, "skew tile");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = lane & 31, hh = lane >> 5;
    rp_stage_tables<NWT, true, false, false, true>(p, EkX, nullptr, nullptr, EvXT);
    __syncthreads();
    char* Vt = Wv[wave];
    float* Rs = (float*)(Vt + 64 * RP_QROW);
    char* Ps = (char*)Rs;
    const int T = p.T, tsh = p.tsh;
    const int sq = ql >> tsh;
    const long long units = (long long)p.nitems * p.H;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int h = (int)(u % p.H);
        const long long row0 = (u / p.H) * 128 + wave * 32;           // first row of this wave's tile
        if (row0 >= p.R) continue;
        const int nq = (int)min((long long)32, p.R - row0);           // rows of the tile that exist (whole sequences)
        const bool qok = ql < nq;
        bf16x8 qf[4], kf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 tq = {0u, 0u, 0u, 0u}, tk = {0u, 0u, 0u, 0u}, tv = {0u, 0u, 0u, 0u};
            if (qok) {
                const int c = h * 64 + ks * 16 + hh * 8;
                tq = *(const u32x4*)(p.q + (row0 + ql) * p.q_rs + c);
                tk = *(const u32x4*)(p.k + (row0 + ql) * p.k_rs + c);
                tv = *(const u32x4*)(p.v + (row0 + ql) * p.v_rs + c);
            }
            qf[ks] = __builtin_bit_cast(bf16x8, tq);
            kf[ks] = __builtin_bit_cast(bf16x8, tk);
            rp_scatter8(Vt, tv, ks * 16 + hh * 8, ql);
        }
        // S^T = K Q^T and Rk^T = EkX Q^T: lane = query, registers = keys / distances
        f32x16 s, rk[NWT];
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
#pragma unroll
        for (int wt = 0; wt < NWT; ++wt) {
#pragma unroll
            for (int e = 0; e < 16; ++e) rk[wt][e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 ef = *(const bf16x8*)(EkX + (wt * 32 + ql) * AS_KROW + ks * 32 + hh * 16);
                rk[wt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ef, qf[ks], rk[wt], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) Rs[ql * RST + wt * 32 + as_crow(r, hh)] = rk[wt][r];
        }
        __builtin_amdgcn_wave_barrier();
        float mx = -1e30f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kl = as_crow(r, hh);
            const bool ok = (kl >> tsh) == sq && kl < nq;
            const int w = ok ? kl - ql + T - 1 : 0;
            const float x = (s[r] + Rs[ql * RST + w]) * p.scale2;
            s[r] = ok ? x : -1e30f;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = s[r] > -1e29f ? __builtin_amdgcn_exp2f(s[r] - mx) : 0.f;
            s[r] = e;
            sum += e;
        }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = sum > 0.f ? 1.0f / sum : 0.f;
        if (hh == 0 && qok) p.lse2[(long long)h * p.R + row0 + ql] = mx + __builtin_amdgcn_logf(sum);       // v_log_f32 = log2
        __builtin_amdgcn_wave_barrier();
        rp_zero16(Ps, 32 * PST, lane);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] *= inv;
            const int kl = as_crow(r, hh);
            const bool ok = (kl >> tsh) == sq && kl < nq;
            if (ok) *(unsigned short*)(Ps + ql * PST + (kl - ql + T - 1) * 2) = __builtin_bit_cast(unsigned short, (bf16_t)s[r]);
        }
        __builtin_amdgcn_wave_barrier();
        // O = P V + Pskew EvX
        f32x16 o[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const bf16x8 pf = as_pack8(s, s2);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 vf = as_tfrag(Vt + (dt * 32 + ql) * RP_QROW, s2, hh);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, o[dt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2 * NWT; ++ks) {
            const bf16x8 af = *(const bf16x8*)(Ps + ql * PST + (ks * 16 + hh * 8) * 2);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 bf = *(const bf16x8*)(EvXT + (dt * 32 + ql) * PST + (ks * 16 + hh * 8) * 2);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, o[dt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = as_crow(r, hh);
                if (qr < nq) p.out[(row0 + qr) * p.o_rs + h * 64 + dt * 32 + ql] = (bf16_t)o[dt][r];
            }
        __builtin_amdgcn_wave_barrier();
    }
}

// ============================================================================================================ backward
// S = Q K^T, dP = dO V^T, Rk = Q EkX^T, Rv = dO EvX^T with the KEY (or the distance) on the lane and the query in the registers, so
// that P^T and dS^T feed dV = P^T dO and dK = dS^T Q from registers; dS, dSskew, dSskew^T and Pskew^T cross the wave's LDS once.
template <int NWT>
__global__ __launch_bounds__(256, 1) void attn_relpos_bwd_kernel(RelposParams p) {
    constexpr int NW = NWT * 32;
    constexpr int RST = NW + 1;
    constexpr int PST = (NW + 8) * 2;
    constexpr int SKEW = (NW * RP_QROW * 2 + 32 * PST) > 32 * RST * 4 ? (NW * RP_QROW * 2 + 32 * PST) : 32 * RST * 4;
    constexpr int WVB = 3 * 64 * RP_QROW + 32 * RP_QROW + 256 + SKEW;       // Q^T | dO^T | K^T | dS | lse, delta | skew tiles
    static_assert(SKEW % 16 == 0 && WVB % 16 == 0, "per-wave LDS");
    static_assert(4 * WVB >= 2 * NW * 64 * 4, "the table-gradient tile reuses the waves' LDS");
    __shared__ __attribute__((aligned(16))) char EkX[NW * AS_KROW];
    __shared__ __attribute__((aligned(16))) char EvX[NW * AS_KROW];
    __shared__ __attribute__((aligned(16))) char EkXT[64 * PST];
    __shared__ __attribute__((aligned(16))) char Wv[4 * WVB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = lane & 31, hh = lane >> 5;
    rp_stage_tables<NWT, true, true, true, false>(p, EkX, EvX, EkXT, nullptr);
    __syncthreads();
    char* Qt = Wv + wave * WVB;
    char* dOt = Qt + 64 * RP_QROW;
    char* Kt = dOt + 64 * RP_QROW;
    char* dSs = Kt + 64 * RP_QROW;                   // [32 q][32 keys + 8] bf16
    float* stat = (float*)(dSs + 32 * RP_QROW);      // [0,32): lse2, [32,64): delta
    char* U = (char*)(stat + 64);
    float* Rs = (float*)U;                           // fp32 [32 q][NW]: Rk, then Rv
    char* PskT = U;                                  // then: bf16 Pskew^T [NW][32 q + 8] | dSskew^T [NW][32 q + 8] | dSskew [32 q][NW + 8]
    char* DskT = PskT + NW * RP_QROW;
    char* Dsk = DskT + NW * RP_QROW;
    const int T = p.T, tsh = p.tsh;
    const int sk = ql >> tsh;                        // sequence of this lane's key inside the tile
    const bool want = p.want_tables != 0;

    f32x16 dEk[NWT][2], dEv[NWT][2];
#pragma unroll
    for (int wt = 0; wt < NWT; ++wt)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { dEk[wt][dt][e] = 0.f; dEv[wt][dt][e] = 0.f; }

    const long long units = (long long)p.nitems * p.H;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int h = (int)(u % p.H);
        const long long row0 = (u / p.H) * 128 + wave * 32;
        if (row0 >= p.R) continue;
        const int nq = (int)min((long long)32, p.R - row0);
        const bool rok = ql < nq;                    // this lane's row (a query for the loads, a key for the products) exists
        bf16x8 qf[4], dof[4], kf[4], vf[4];
        float dl = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 tq = {0u, 0u, 0u, 0u}, td = {0u, 0u, 0u, 0u}, to = {0u, 0u, 0u, 0u}, tk = {0u, 0u, 0u, 0u}, tv = {0u, 0u, 0u, 0u};
            if (rok) {
                const int c = h * 64 + ks * 16 + hh * 8;
                tq = *(const u32x4*)(p.q + (row0 + ql) * p.q_rs + c);
                tk = *(const u32x4*)(p.k + (row0 + ql) * p.k_rs + c);
                tv = *(const u32x4*)(p.v + (row0 + ql) * p.v_rs + c);
                td = *(const u32x4*)(p.dout + (row0 + ql) * p.do_rs + c);
                to = *(const u32x4*)(p.o + (row0 + ql) * p.o_rs + c);
            }
            qf[ks] = __builtin_bit_cast(bf16x8, tq);
            dof[ks] = __builtin_bit_cast(bf16x8, td);
            kf[ks] = __builtin_bit_cast(bf16x8, tk);
            vf[ks] = __builtin_bit_cast(bf16x8, tv);
            float a[8], b[8];
            unpack8(td, a); unpack8(to, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) dl += a[e] * b[e];
            rp_scatter8(Qt, tq, ks * 16 + hh * 8, ql);
            rp_scatter8(dOt, td, ks * 16 + hh * 8, ql);
            rp_scatter8(Kt, tk, ks * 16 + hh * 8, ql);
        }
        dl += __shfl_xor(dl, 32, 64);
        if (hh == 0) {
            stat[ql] = rok ? p.lse2[(long long)h * p.R + row0 + ql] : 0.f;
            stat[32 + ql] = dl;
        }
        f32x16 S, dP;
#pragma unroll
        for (int e = 0; e < 16; ++e) { S[e] = 0.f; dP[e] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], kf[ks], S, 0, 0, 0);            // [query rows][key cols]
            dP = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof[ks], vf[ks], dP, 0, 0, 0);
        }
        // the two table score terms, one after the other through the same fp32 tile: pass 0 Rk -> S, pass 1 Rv -> dP
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int wt = 0; wt < NWT; ++wt) {
                f32x16 rr;
#pragma unroll
                for (int e = 0; e < 16; ++e) rr[e] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8 ef = *(const bf16x8*)((pass == 0 ? EkX : EvX) + (wt * 32 + ql) * AS_KROW + ks * 32 + hh * 16);
                    rr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pass == 0 ? qf[ks] : dof[ks], ef, rr, 0, 0, 0);     // [query rows][distance cols]
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) Rs[as_crow(r, hh) * RST + wt * 32 + ql] = rr[r];
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = as_crow(r, hh);
                const bool ok = (qr >> tsh) == sk && rok && qr < nq;
                const float x = Rs[qr * RST + (ok ? ql - qr + T - 1 : 0)];
                if (pass == 0) S[r] += x; else dP[r] += x;
            }
            __builtin_amdgcn_wave_barrier();
        }
        rp_zero16(U, NW * RP_QROW * 2 + 32 * PST, lane);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = as_crow(r, hh);
            const bool ok = (qr >> tsh) == sk && rok && qr < nq;
            const float pr = ok ? __builtin_amdgcn_exp2f(S[r] * p.scale2 - stat[qr]) : 0.f;
            S[r] = pr;
            dP[r] = pr * (dP[r] - stat[32 + qr]) * p.scale;
            const unsigned short pb = __builtin_bit_cast(unsigned short, (bf16_t)pr);
            const unsigned short db = __builtin_bit_cast(unsigned short, (bf16_t)dP[r]);
            *(unsigned short*)(dSs + qr * RP_QROW + ql * 2) = db;
            if (ok) {
                const int w = ql - qr + T - 1;
                *(unsigned short*)(PskT + w * RP_QROW + qr * 2) = pb;
                *(unsigned short*)(DskT + w * RP_QROW + qr * 2) = db;
                *(unsigned short*)(Dsk + qr * PST + w * 2) = db;
            }
        }
        __builtin_amdgcn_wave_barrier();
        // dV = P^T dO, dK = dS^T Q: [key rows][d cols]
        f32x16 acc[2];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[dt][e] = 0.f;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8 af = as_pack8(which == 0 ? S : dP, s2);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const bf16x8 bf = as_tfrag((which == 0 ? dOt : Qt) + (dt * 32 + ql) * RP_QROW, s2, hh);
                    acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[dt], 0, 0, 0);
                }
            }
            bf16_t* dst = which == 0 ? p.dv : p.dk;
            const long long rs = which == 0 ? p.dv_rs : p.dk_rs;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = as_crow(r, hh);
                    if (key < nq) dst[(row0 + key) * rs + h * 64 + dt * 32 + ql] = (bf16_t)acc[dt][r];
                }
        }
        // dQ = dS K + dSskew EkX
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[dt][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 af = *(const bf16x8*)(dSs + ql * RP_QROW + (ks * 16 + hh * 8) * 2);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 bf = *(const bf16x8*)(Kt + (dt * 32 + ql) * RP_QROW + (ks * 16 + hh * 8) * 2);
                acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[dt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2 * NWT; ++ks) {
            const bf16x8 af = *(const bf16x8*)(Dsk + ql * PST + (ks * 16 + hh * 8) * 2);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 bf = *(const bf16x8*)(EkXT + (dt * 32 + ql) * PST + (ks * 16 + hh * 8) * 2);
                acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[dt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = as_crow(r, hh);
                if (qr < nq) p.dq[(row0 + qr) * p.dq_rs + h * 64 + dt * 32 + ql] = (bf16_t)acc[dt][r];
            }
        // dEkX += dSskew^T Q, dEvX += Pskew^T dO: [distance rows][d cols], kept in registers across the workgroup's items
        if (want) {
#pragma unroll
            for (int wt = 0; wt < NWT; ++wt)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 ak = *(const bf16x8*)(DskT + (wt * 32 + ql) * RP_QROW + (ks * 16 + hh * 8) * 2);
                    const bf16x8 av = *(const bf16x8*)(PskT + (wt * 32 + ql) * RP_QROW + (ks * 16 + hh * 8) * 2);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const bf16x8 bq = *(const bf16x8*)(Qt + (dt * 32 + ql) * RP_QROW + (ks * 16 + hh * 8) * 2);
                        const bf16x8 bd = *(const bf16x8*)(dOt + (dt * 32 + ql) * RP_QROW + (ks * 16 + hh * 8) * 2);
                        dEk[wt][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, bq, dEk[wt][dt], 0, 0, 0);
                        dEv[wt][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bd, dEv[wt][dt], 0, 0, 0);
                    }
                }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (!want) return;
    // ---- table gradients: waves -> one LDS tile [2][NW][64] fp32 (over the waves' regions) -> one copy of the workspace ----
    __syncthreads();
    float* Tg = (float*)Wv;
    for (int i = tid; i < 2 * NW * 64; i += 256) Tg[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int wt = 0; wt < NWT; ++wt)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int at = (wt * 32 + as_crow(r, hh)) * 64 + dt * 32 + ql;
                atomicAdd(Tg + at, dEk[wt][dt][r]);
                atomicAdd(Tg + NW * 64 + at, dEv[wt][dt][r]);
            }
    __syncthreads();
    float* wsc = p.ws + (size_t)(blockIdx.x % RP_COPIES) * (2 * 64 * 64);
    const int nw = 2 * T - 1;
    for (int i = tid; i < 2 * nw * 64; i += 256) {
        const int tb = i / (nw * 64), rem = i - tb * nw * 64;
        atomicAdd(wsc + tb * 64 * 64 + rem, Tg[tb * NW * 64 + rem]);
    }
}

// d_rel[t] += sum over the copies and over the distances w that the clamp folds onto table row t
__global__ __launch_bounds__(128) void attn_relpos_reduce_kernel(const float* ws, float* d_rel_k, float* d_rel_v, int T, int P) {
    const int t = blockIdx.x, tb = threadIdx.x >> 6, d = threadIdx.x & 63;
    float* dst = tb == 0 ? d_rel_k : d_rel_v;
    if (dst == nullptr) return;
    int wlo = t - P + T - 1, whi = wlo;              // the distance t - P itself ...
    if (t == 0) wlo = 0;                             // ... and, on the end rows, everything beyond it
    if (t == 2 * P) whi = 2 * T - 2;
    wlo = max(wlo, 0); whi = min(whi, 2 * T - 2);
    if (wlo > whi) return;
    float s = 0.f;
    for (int w = wlo; w <= whi; ++w)
        for (int c = 0; c < RP_COPIES; ++c) s += ws[((size_t)(c * 2 + tb) * 64 + w) * 64 + d];
    dst[(size_t)t * 64 + d] += s;
}

static int rp_check(int R, int H, int T, int P, const long long* strides, int nstr, const void* const* ptrs, int nptr) {
    if (T < 1 || T > 32 || (32 % T) || P < 1 || H < 1 || R < 1 || (R % T)) return VT_ERR_BAD_SHAPE;
    for (int i = 0; i < nstr; ++i)
        if (strides[i] < (long long)H * 64 || strides[i] % 8) return VT_ERR_BAD_SHAPE;
    for (int i = 0; i < nptr; ++i)
        if (ptrs[i] == nullptr || (((uintptr_t)ptrs[i]) & 15)) return VT_ERR_BAD_ALIGN;
    return VT_OK;
}

static void rp_fill(RelposParams& p, int R, int H, int T, int P, float softmax_scale) {
    p.R = R; p.H = H; p.T = T; p.P = P; p.nitems = (R + 127) / 128;
    p.tsh = 0;
    while ((1 << p.tsh) < T) ++p.tsh;
    p.scale = softmax_scale; p.scale2 = softmax_scale * 1.4426950408889634f;
}

// fp32 scratch of the backward's table-gradient reduction (RP_COPIES copies of the two expanded tables): independent of R, H, T and P
extern "C" long long vt_attn_relpos_workspace_bytes(void) { return (long long)RP_WS_FLOATS * 4; }

// q, k, v, o: ONE row space of R rows = R / T consecutive sequences of T rows (32 % T == 0); element (row s, head h, d) at
// base + s*rs + h*64 + d.  rel_k, rel_v: bf16 [2P+1, 64] contiguous.  lse2: fp32 [H, R], base-2 log-sum-exp of the TOTAL scaled score.
extern "C" int vt_attn_relpos_fwd(const void* q, const void* k, const void* v, const void* rel_k, const void* rel_v, void* o, float* lse2,
                                  int R, int H, int T, int P, long long q_rs, long long k_rs, long long v_rs, long long o_rs,
                                  float softmax_scale, void* stream) {
    const long long st[4] = {q_rs, k_rs, v_rs, o_rs};
    const void* const ptrs[7] = {q, k, v, rel_k, rel_v, o, lse2};
    const int rc = rp_check(R, H, T, P, st, 4, ptrs, 7);
    if (rc != VT_OK) return rc;
    RelposParams p = {};
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.rel_k = (const bf16_t*)rel_k; p.rel_v = (const bf16_t*)rel_v;
    p.out = (bf16_t*)o; p.lse2 = lse2;
    p.q_rs = q_rs; p.k_rs = k_rs; p.v_rs = v_rs; p.o_rs = o_rs;
    rp_fill(p, R, H, T, P, softmax_scale);
    const long long units = (long long)p.nitems * H;
    const dim3 grid((unsigned)(units < 2048 ? units : 2048));
    hipStream_t s = (hipStream_t)stream;
    if (T <= 16) hipLaunchKernelGGL((attn_relpos_fwd_kernel<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((attn_relpos_fwd_kernel<2>), grid, dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// dq, dk, dv: bf16 in the row space, written whole.  d_rel_k, d_rel_v: fp32 [2P+1, 64]; the gradients are ADDED into them (fp32 atomics
// on the way: not bitwise reproducible from run to run).  Either may be NULL; with both NULL (frozen tables) no table-gradient work is
// done and workspace may be NULL.  Otherwise workspace holds vt_attn_relpos_workspace_bytes() bytes (zeroed here).
extern "C" int vt_attn_relpos_bwd(const void* q, const void* k, const void* v, const void* rel_k, const void* rel_v, const void* o,
                                  const void* dout, const float* lse2, void* dq, void* dk, void* dv, float* d_rel_k, float* d_rel_v,
                                  void* workspace, int R, int H, int T, int P, long long q_rs, long long k_rs, long long v_rs,
                                  long long o_rs, long long do_rs, long long dq_rs, long long dk_rs, long long dv_rs,
                                  float softmax_scale, void* stream) {
    const long long st[8] = {q_rs, k_rs, v_rs, o_rs, do_rs, dq_rs, dk_rs, dv_rs};
    const void* const ptrs[11] = {q, k, v, rel_k, rel_v, o, dout, lse2, dq, dk, dv};
    const int rc = rp_check(R, H, T, P, st, 8, ptrs, 11);
    if (rc != VT_OK) return rc;
    const bool want = d_rel_k != nullptr || d_rel_v != nullptr;
    if (want && (workspace == nullptr || (((uintptr_t)workspace) & 15))) return VT_ERR_BAD_ALIGN;
    RelposParams p = {};
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.rel_k = (const bf16_t*)rel_k; p.rel_v = (const bf16_t*)rel_v;
    p.o = (const bf16_t*)o; p.dout = (const bf16_t*)dout; p.lse2 = const_cast<float*>(lse2);
    p.dq = (bf16_t*)dq; p.dk = (bf16_t*)dk; p.dv = (bf16_t*)dv; p.ws = (float*)workspace; p.want_tables = want ? 1 : 0;
    p.q_rs = q_rs; p.k_rs = k_rs; p.v_rs = v_rs; p.o_rs = o_rs; p.do_rs = do_rs; p.dq_rs = dq_rs; p.dk_rs = dk_rs; p.dv_rs = dv_rs;
    rp_fill(p, R, H, T, P, softmax_scale);
    hipStream_t s = (hipStream_t)stream;
    if (want && hipMemsetAsync(workspace, 0, (size_t)RP_WS_FLOATS * 4, s) != hipSuccess) return VT_ERR_LAUNCH;
    const long long units = (long long)p.nitems * H;
    const dim3 grid((unsigned)(units < 1024 ? units : 1024));
    if (T <= 16) hipLaunchKernelGGL((attn_relpos_bwd_kernel<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((attn_relpos_bwd_kernel<2>), grid, dim3(256), 0, s, p);
    if (want) hipLaunchKernelGGL(attn_relpos_reduce_kernel, dim3(2 * P + 1), dim3(128), 0, s, (const float*)workspace, d_rel_k, d_rel_v, T, P);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
