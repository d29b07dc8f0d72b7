// LoRA side-path kernels for ranks 17..128 (the "wide" layout; lora.hip holds the rank <= 16 ones).  Same semantics:
//     y = W x + b + (alpha/r) * B (A x)
// folded into the base GEMMs as a K-extension, but the extension is ext columns wide (a multiple of 64) and adapter j of a fused
// projection owns the columns [j*rp, j*rp + r) of it, rp = r rounded up to a multiple of 16; every other extension column is
// exactly zero in both operands.  All three rank-side products run on v_mfma_f32_16x16x32_bf16 (bf16 operands, fp32 sums):
//   lane l of a wave holds A[row l&15][k = 8(l>>4) .. +7] and B[k = 8(l>>4) .. +7][col l&15]; D[row 4(l>>4) + reg][col l&15].
// Operands whose reduction index is the slow one in memory (the M rows of the rank gradients, the rank rows of A in the dX
// correction) are transposed on their way into LDS.  LDS rows are padded by 8 elements: the 16-byte fragment reads of 16 rows
// then start 4 banks apart.
// lora_dropout > 0: each product's dropped form is the same kernel with the trailing LoraDrop argument (mask convention and
// semantics: see lora.hip and common.h).  Adapter j of a call is site site0 + j; element (m_g, k_g) of the logical [M_g, K_log] adapter
// input has index e = m_g * K_log + k_g.  Every dropped instantiation takes a LoraOrigin behind the LoraDrop: the map from the call's
// (m, k) to (m_g, k_g).  The _drop entry points pass the identity (the call IS the logical input); the _drop_at entry points take the
// map from the caller: one rank's rows of a sequence-parallel run, one column range of a wider input (HunyuanVideo).
#include "common.h"

#define LW_PAD 8
#define LW_KS (64 + LW_PAD)          // LDS row stride (elements) of a 64-deep reduction block

__device__ __forceinline__ bf16x8 lw_frag(const bf16_t* p) { return *(const bf16x8*)p; }
__device__ __forceinline__ unsigned int lw_half(const u32x4& v, int e) { return (e & 1) ? (v[e >> 1] >> 16) : (v[e >> 1] & 0xffffu); }
// two rows (reduction indices 2q, 2q+1) of 8 columns each -> dst[(col0 + e) * stride + 2q] as one dword per column
__device__ __forceinline__ void lw_store_pair_t(bf16_t* dst, int stride, int col0, int q, const u32x4& r0, const u32x4& r1) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
        *(unsigned int*)(dst + (size_t)(col0 + e) * stride + 2 * q) = lw_half(r0, e) | (lw_half(r1, e) << 16);
}

// ---------------- T[m, j*rp + i] = sum_k X[m,k] * A[j*r + i, k]   (j < n, i < r), zeros in every other column up to ext ----------------
// One block owns 64 rows of X and every output column, so X is read once whatever the rank.  Per 64-deep K block the X rows and
// the n*rp (padded) rows of A go through LDS; wave w owns the 16-column tiles w, w+4, ... (at most 6) of all four 16-row tiles.
// The product is taken as A X^T so that a lane ends up with 4 consecutive columns of one row: one 8-byte store.
// DROP: T[m, j*rp + i] = 1/(1-p) sum_k keep_j(m,k) X[m,k] * A[j*r + i, k] with one masked copy of the 64 x 64 X block per adapter in
// LDS: the mask is taken once per element and adapter while staging (masking the shared fragments in registers would repeat the
// Philox work in each of the four waves).  The column tiles of a wave run through the adapters in order, so the X fragments are
// reloaded only where the adapter changes.
#define LWD_TPW 6
template <typename... D>
__global__ __launch_bounds__(256) void lora_wide_down_kernel(const bf16_t* X, int ldx, const bf16_t* A, int lda, int n, int r, int rp,
                                                            int ext, bf16_t* T, int ldt, long long M, int K, D... drop) {
    constexpr bool DROP = sizeof...(D) > 0;
    const LoraDrop dr = lora_drop_arg(drop...);
    const LoraOrigin og = lora_origin_arg(drop...);
    const int nx = DROP ? n : 1;                // X blocks in LDS
    extern __shared__ __attribute__((aligned(16))) bf16_t lw_smem[];
    bf16_t* sX = lw_smem;                       // [nx][64][LW_KS]; DROP: block j = X masked for adapter j
    bf16_t* sA = lw_smem + nx * 64 * LW_KS;     // [n*rp][LW_KS], zero rows where i >= r
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int NC = n * rp, nct = NC >> 4;
    const long long row0 = (long long)blockIdx.x * 64;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    f32x4 acc[LWD_TPW][4];
#pragma unroll
    for (int i = 0; i < LWD_TPW; ++i)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[i][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned long long eb[2] = {0ull, 0ull};    // DROP: logical index of element (m, 0) of the two rows this thread stages
    if constexpr (DROP) {
#pragma unroll
        for (int it = 0; it < 2; ++it) eb[it] = lora_origin_elem(og, row0 + ((tid + 256 * it) >> 3));
    }
    for (int k0 = 0; k0 < K; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int u = tid + 256 * it, row = u >> 3, ch = u & 7;
            const long long m = row0 + row;
            u32x4 v = zero4;
            if (m < M) v = *(const u32x4*)(X + (size_t)m * ldx + k0 + 8 * ch);
            if constexpr (DROP) {
                const unsigned long long e4 = (eb[it] + k0 + 8 * ch) >> 2;
                for (int j = 0; j < n; ++j)
                    *(u32x4*)(sX + (j * 64 + row) * LW_KS + 8 * ch) = keep_mask8(v, lora_site_offset(dr.site0 + j) + e4, dr.seed, dr.thresh);
            } else {
                *(u32x4*)(sX + row * LW_KS + 8 * ch) = v;
            }
        }
        for (int u = tid; u < NC * 8; u += 256) {
            const int c = u >> 3, ch = u & 7;
            const int j = c / rp, i = c - j * rp;
            u32x4 v = zero4;
            if (i < r) v = *(const u32x4*)(A + (size_t)(j * r + i) * lda + k0 + 8 * ch);
            *(u32x4*)(sA + c * LW_KS + 8 * ch) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 xf[4];
            int jcur = -1;
            if constexpr (!DROP) {
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) xf[rt] = lw_frag(sX + (rt * 16 + fr) * LW_KS + ks * 32 + 8 * fq);
            }
#pragma unroll
            for (int i = 0; i < LWD_TPW; ++i) {
                const int t = wave + 4 * i;
                if (t < nct) {
                    if constexpr (DROP) {
                        const int j = (16 * t) / rp;
                        if (j != jcur) {
                            jcur = j;
#pragma unroll
                            for (int rt = 0; rt < 4; ++rt) xf[rt] = lw_frag(sX + (j * 64 + rt * 16 + fr) * LW_KS + ks * 32 + 8 * fq);
                        }
                    }
                    const bf16x8 af = lw_frag(sA + (t * 16 + fr) * LW_KS + ks * 32 + 8 * fq);
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) acc[i][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf[rt], acc[i][rt], 0, 0, 0);
                }
            }
        }
    }
    // D[row = column 16t + 4fq + reg][col = row fr of the row tile]
#pragma unroll
    for (int i = 0; i < LWD_TPW; ++i) {
        const int t = wave + 4 * i;
        if (t < nct) {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const long long m = row0 + rt * 16 + fr;
                if (m < M) {
                    u32x2 o;
                    if constexpr (DROP) acc[i][rt] *= dr.inv_keep;
                    o[0] = pack2(acc[i][rt][0], acc[i][rt][1]);
                    o[1] = pack2(acc[i][rt][2], acc[i][rt][3]);
                    *(u32x2*)(T + (size_t)m * ldt + t * 16 + 4 * fq) = o;
                }
            }
        }
    }
    // the rest of the extension must be exactly zero (the packed weight is zero there, but 0 * NaN is NaN)
    const int zc = (ext - NC) >> 2;
    for (int u = tid; u < 64 * zc; u += 256) {
        const int row = u / zc, cc = u - row * zc;
        const long long m = row0 + row;
        if (m < M) *(u32x2*)(T + (size_t)m * ldt + NC + 4 * cc) = u32x2{0u, 0u};
    }
}
// DROP: n_adapters masked X blocks and the padded A rows must fit the 64 KB of LDS a block gets without opting in to more
extern "C" int vt_lora_down_wide_drop_fits(int n_adapters, int rp) {
    return (size_t)n_adapters * (64 + rp) * LW_KS * sizeof(bf16_t) <= 65536 && n_adapters * rp <= 16 * 4 * LWD_TPW;
}
// dr == nullptr: no dropout
static int lora_down_wide_launch(const void* X, int ldx, const void* A, int lda, int n_adapters, int r, int rp, int ext, void* T, int ldt,
                                 long long M, int K, const LoraDrop* dr, const LoraOrigin* og, void* stream) {
    if (M <= 0 || K <= 0 || (K % 64) || n_adapters <= 0 || r <= 0 || r > 128 || rp < r || (rp % 16) ||
        n_adapters * rp > 16 * 4 * LWD_TPW || ext < n_adapters * rp || (ext % 4) || (ldx % 8) || (lda % 8) || (ldt % 4) || ldt < ext)
        return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)X) | ((uintptr_t)A)) & 15) return VT_ERR_BAD_ALIGN;
    if (((uintptr_t)T) & 7) return VT_ERR_BAD_ALIGN;
    const long long blocks = (M + 63) / 64;
    if (blocks > 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    const size_t lds = (size_t)((dr ? n_adapters : 1) * 64 + n_adapters * rp) * LW_KS * sizeof(bf16_t);
    if (dr == nullptr)
        hipLaunchKernelGGL(lora_wide_down_kernel<>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)X, ldx,
                           (const bf16_t*)A, lda, n_adapters, r, rp, ext, (bf16_t*)T, ldt, M, K);
    else
        hipLaunchKernelGGL((lora_wide_down_kernel<LoraDrop, LoraOrigin>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream,
                           (const bf16_t*)X, ldx, (const bf16_t*)A, lda, n_adapters, r, rp, ext, (bf16_t*)T, ldt, M, K, *dr, *og);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
extern "C" int vt_lora_down_wide(const void* X, int ldx, const void* A, int lda, int n_adapters, int r, int rp, int ext, void* T,
                                 int ldt, long long M, int K, void* stream) {
    return lora_down_wide_launch(X, ldx, A, lda, n_adapters, r, rp, ext, T, ldt, M, K, nullptr, nullptr, stream);
}
extern "C" int vt_lora_down_wide_drop(const void* X, int ldx, const void* A, int lda, int n_adapters, int r, int rp, int ext, void* T,
                                      int ldt, long long M, int K, float p, unsigned long long seed, int site0, void* stream) {
    if (n_adapters <= 0 || !vt_lora_down_wide_drop_fits(n_adapters, rp) || vt_lora_drop_bad(p, site0)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0);
    const LoraOrigin og = vt_lora_origin_identity(M, K);
    return lora_down_wide_launch(X, ldx, A, lda, n_adapters, r, rp, ext, T, ldt, M, K, &dr, &og, stream);
}
// _at: X holds the rows / columns of the adapters' logical input that the origin map names (common.h, LoraOrigin)
extern "C" int vt_lora_down_wide_drop_at(const void* X, int ldx, const void* A, int lda, int n_adapters, int r, int rp, int ext, void* T,
                                         int ldt, long long M, int K, float p, unsigned long long seed, int site0, long long seg_local,
                                         long long seg_global, long long n_first, long long off_first, long long off_rest, int k0,
                                         int K_log, void* stream) {
    const LoraOrigin og = {seg_local, seg_global, n_first, off_first, off_rest, k0, K_log};
    if (n_adapters <= 0 || !vt_lora_down_wide_drop_fits(n_adapters, rp) || vt_lora_drop_bad(p, site0) || vt_lora_origin_bad(og, M, K))
        return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0);
    return lora_down_wide_launch(X, ldx, A, lda, n_adapters, r, rp, ext, T, ldt, M, K, &dr, &og, stream);
}

// ---------------- out[p*osp + i*osr] += alpha * sum_m Big[m,p] * Small[m,i]   (i < R <= 128) ----------------
// A block owns 128 columns p of Big, all R columns of Small and a slice of the M rows; both operands have the reduction index m
// as their slow one, so each 64-row block is transposed into LDS ([p][m] and [i][m]).  Wave w owns the p tiles 2w, 2w+1 against
// every i tile: up to 2 x 8 accumulator tiles.  The slices add their [128, R] partial sums with fp32 atomics; the slice count is
// chosen so that about two blocks per CU exist, which keeps the atomic traffic (slices * P * R * 4 bytes) well under the bytes of
// Big itself.  Atomic sums depend on arrival order: the result is not bitwise reproducible (there is no two-stage mode here).
// I_FAST: the operand order that makes a wave's atomic instruction run along the output's fast index (i when osr == 1, else p).
// DROP: out += alpha/(1-p) * sum_m keep_s(m,p) Big[m,p] * Small[m,i] for one adapter, site s = site0: Big is masked on its way into
// LDS (each element of Big is staged once per call); alpha carries the 1 / (1 - p).
#define LWT_BLOCKS 512
template <bool I_FAST, typename... D>
__global__ __launch_bounds__(256) void lora_wide_tn_kernel(const bf16_t* Big, int ldb, const bf16_t* Small, int lds_, int R, float* out,
                                                          long long osp, long long osr, float alpha, long long M, int P,
                                                          int tiles_per_slice, D... drop) {
    constexpr bool DROP = sizeof...(D) > 0;
    const LoraDrop dr = lora_drop_arg(drop...);
    const LoraOrigin og = lora_origin_arg(drop...);
    const unsigned long long off = lora_site_offset(dr.site0);
    __shared__ __attribute__((aligned(16))) bf16_t sB[128 * LW_KS];
    __shared__ __attribute__((aligned(16))) bf16_t sS[128 * LW_KS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int p0 = blockIdx.x * 128;
    const int nit = (R + 15) >> 4;
    const long long tile0 = (long long)blockIdx.y * tiles_per_slice;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    f32x4 acc[2][8];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int it = 0; it < 8; ++it) acc[pt][it] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < tiles_per_slice; ++t) {
        const long long m0 = (tile0 + t) * 64;
        if (m0 >= M) break;
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int u = tid + 256 * it, q = u >> 4, pc = u & 15;
            const int p = p0 + 8 * pc;
            const long long m = m0 + 2 * q;
            u32x4 r0 = zero4, r1 = zero4;
            if (p < P) {
                if (m < M) r0 = *(const u32x4*)(Big + (size_t)m * ldb + p);
                if (m + 1 < M) r1 = *(const u32x4*)(Big + (size_t)(m + 1) * ldb + p);
                if constexpr (DROP) {
                    // the two rows' logical indices separately: a segment boundary of the origin map may lie between them
                    if (m < M) r0 = keep_mask8(r0, off + ((lora_origin_elem(og, m) + p) >> 2), dr.seed, dr.thresh);
                    if (m + 1 < M) r1 = keep_mask8(r1, off + ((lora_origin_elem(og, m + 1) + p) >> 2), dr.seed, dr.thresh);
                }
            }
            lw_store_pair_t(sB, LW_KS, 8 * pc, q, r0, r1);
        }
        for (int u = tid; u < nit * 16 * 32; u += 256) {
            const int q = u / (nit * 16), i = u - q * (nit * 16);
            const long long m = m0 + 2 * q;
            unsigned int lo = 0, hi = 0;
            if (i < R) {
                if (m < M) lo = *(const unsigned short*)(Small + (size_t)m * lds_ + i);
                if (m + 1 < M) hi = *(const unsigned short*)(Small + (size_t)(m + 1) * lds_ + i);
            }
            *(unsigned int*)(sS + i * LW_KS + 2 * q) = lo | (hi << 16);
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 bfr[2];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) bfr[pt] = lw_frag(sB + ((2 * wave + pt) * 16 + fr) * LW_KS + ks * 32 + 8 * fq);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                if (it < nit) {
                    const bf16x8 sf = lw_frag(sS + (it * 16 + fr) * LW_KS + ks * 32 + 8 * fq);
#pragma unroll
                    for (int pt = 0; pt < 2; ++pt)
                        acc[pt][it] = I_FAST ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[pt], sf, acc[pt][it], 0, 0, 0)
                                             : __builtin_amdgcn_mfma_f32_16x16x32_bf16(sf, bfr[pt], acc[pt][it], 0, 0, 0);
                }
            }
        }
    }
    // I_FAST: D[row = p][col = i], else D[row = i][col = p]  (row = 4fq + reg, col = fr)
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            if (it < nit) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int p = p0 + (2 * wave + pt) * 16 + (I_FAST ? 4 * fq + j : fr);
                    const int i = it * 16 + (I_FAST ? fr : 4 * fq + j);
                    if (p < P && i < R) atomicAdd(out + (size_t)p * osp + (size_t)i * osr, alpha * acc[pt][it][j]);
                }
            }
        }
}
// dr == nullptr: no dropout, else alpha carries the 1 / (1 - p)
static int lora_tn_wide_launch(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp, long long osr,
                               float alpha, long long M, int P, const LoraDrop* dr, const LoraOrigin* og, void* stream) {
    if (M <= 0 || P <= 0 || (P % 8) || R <= 0 || R > 128 || (ldb % 8) || lds_ < R || osp <= 0 || osr <= 0) return VT_ERR_BAD_SHAPE;
    if (((uintptr_t)Big) & 15) return VT_ERR_BAD_ALIGN;
    if ((((uintptr_t)Small) & 1) || (((uintptr_t)out) & 3)) return VT_ERR_BAD_ALIGN;
    const long long tiles = (M + 63) / 64;
    const int pblocks = (P + 127) / 128;
    long long slices = LWT_BLOCKS / pblocks;
    if (slices < 1) slices = 1;
    if (slices > tiles) slices = tiles;
    const long long tps = (tiles + slices - 1) / slices;
    slices = (tiles + tps - 1) / tps;
    if (tps > 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    dim3 grid((unsigned)pblocks, (unsigned)slices);
    hipStream_t st = (hipStream_t)stream;
#define LWT_ARGS (const bf16_t*)Big, ldb, (const bf16_t*)Small, lds_, R, out, osp, osr, alpha, M, P, (int)tps
    if (dr == nullptr) {
        if (osr == 1) hipLaunchKernelGGL(lora_wide_tn_kernel<true>, grid, dim3(256), 0, st, LWT_ARGS);
        else hipLaunchKernelGGL(lora_wide_tn_kernel<false>, grid, dim3(256), 0, st, LWT_ARGS);
    } else {
        if (osr == 1) hipLaunchKernelGGL((lora_wide_tn_kernel<true, LoraDrop, LoraOrigin>), grid, dim3(256), 0, st, LWT_ARGS, *dr, *og);
        else hipLaunchKernelGGL((lora_wide_tn_kernel<false, LoraDrop, LoraOrigin>), grid, dim3(256), 0, st, LWT_ARGS, *dr, *og);
    }
#undef LWT_ARGS
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
extern "C" int vt_lora_tn_wide(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp, long long osr,
                               float alpha, long long M, int P, void* stream) {
    return lora_tn_wide_launch(Big, ldb, Small, lds_, R, out, osp, osr, alpha, M, P, nullptr, nullptr, stream);
}
extern "C" int vt_lora_tn_wide_drop(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp, long long osr,
                                    float alpha, long long M, int P, float p, unsigned long long seed, int site, void* stream) {
    if (vt_lora_drop_bad(p, site)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site);
    const LoraOrigin og = vt_lora_origin_identity(M, P);
    return lora_tn_wide_launch(Big, ldb, Small, lds_, R, out, osp, osr, alpha * dr.inv_keep, M, P, &dr, &og, stream);
}
// _at: Big holds the rows / columns of the adapter's logical input that the origin map names (the P columns are k0 .. k0 + P of K_log)
extern "C" int vt_lora_tn_wide_drop_at(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp,
                                       long long osr, float alpha, long long M, int P, float p, unsigned long long seed, int site,
                                       long long seg_local, long long seg_global, long long n_first, long long off_first,
                                       long long off_rest, int k0, int K_log, void* stream) {
    const LoraOrigin og = {seg_local, seg_global, n_first, off_first, off_rest, k0, K_log};
    if (vt_lora_drop_bad(p, site) || vt_lora_origin_bad(og, M, P)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site);
    return lora_tn_wide_launch(Big, ldb, Small, lds_, R, out, osp, osr, alpha * dr.inv_keep, M, P, &dr, &og, stream);
}

// ---------------- dX[m,k] += sum_j sum_i dT[m, j*rp + i] * A[j*r + i, k]   (in place, bf16; all adapters in one pass) ----------------
// A block owns 128 rows: wave w keeps the dT fragments of its 32 rows in registers for the whole kernel (at most 12 k-steps of 32
// padded rank columns) and the block walks the K columns 64 at a time, A^T of those columns staged in LDS ([k][c], zero where the
// padded column c carries no adapter row).  A^T dT^T puts 4 consecutive columns of one row in a lane: dX is read and written once,
// 8 bytes per lane and tile.
// DROP: dX[m,k] += 1/(1-p) sum_j keep_j(m,k) sum_i dT[m, j*rp + i] * A[j*r + i, k] with an adapter-outer loop: adapter j's MFMA chain
// runs over the 32-deep steps that touch its columns [j rp, (j+1) rp) with the dT fragments of lanes whose 8 columns belong to
// another adapter zeroed (rp = 48, 80: an adapter boundary falls inside a step; a lane's 8 columns never straddle one because
// rp % 16 == 0), its sum is masked -- a lane's 4 consecutive columns of a row are one Philox counter -- and added to a running fp32
// total.
#define LWU_MAXKS 12
template <typename... D>
__global__ __launch_bounds__(256) void lora_wide_up_add_kernel(bf16_t* dX, int ldx, const bf16_t* dT, int ldt, const bf16_t* A, int lda,
                                                              int n, int r, int rp, long long M, int K, D... drop) {
    constexpr bool DROP = sizeof...(D) > 0, DGELU = sizeof...(D) > 2;       // the pack: LoraDrop, LoraOrigin [, LoraDgelu]
    const LoraDrop dr = lora_drop_arg(drop...);
    const LoraOrigin og = lora_origin_arg(drop...);
    const LoraDgelu dg = lora_dgelu_arg(drop...);
    extern __shared__ __attribute__((aligned(16))) bf16_t lw_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int NC = n * rp, NCp = (NC + 31) & ~31, nks = NCp >> 5, LS = NCp + LW_PAD;
    bf16_t* sAt = lw_smem;                      // [64][LS]
    const long long row0 = (long long)blockIdx.x * 128 + 32 * wave;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    bf16x8 dtf[2][LWU_MAXKS];
    unsigned long long eb[2] = {0ull, 0ull};    // DROP: logical index of element (m, 0) of this lane's two rows
    if constexpr (DROP) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) eb[rt] = lora_origin_elem(og, row0 + rt * 16 + fr);
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const long long m = row0 + rt * 16 + fr;
#pragma unroll
        for (int ks = 0; ks < LWU_MAXKS; ++ks) {
            u32x4 v = zero4;
            const int c = ks * 32 + 8 * fq;
            if (ks < nks && m < M && c < NC) v = *(const u32x4*)(dT + (size_t)m * ldt + c);
            dtf[rt][ks] = __builtin_bit_cast(bf16x8, v);
        }
    }
    for (int k0 = 0; k0 < K; k0 += 64) {
        // DGELU: this lane's pre-activations of the 64 columns, fetched ahead of the staging and the MFMA chain that hide their latency
        u32x2 upre[DGELU ? 2 : 1][DGELU ? 4 : 1];
        if constexpr (DGELU) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const long long m = row0 + rt * 16 + fr;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    upre[rt][ct] = m < M ? *(const u32x2*)(dg.U + (size_t)m * dg.ldu + k0 + ct * 16 + 4 * fq) : u32x2{0u, 0u};
            }
        }
        __syncthreads();
        for (int u = tid; u < NCp * 4; u += 256) {
            const int pc = u & 7, q = u >> 3;
            u32x4 rr[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = 2 * q + h;
                const int j = c / rp, i = c - j * rp;
                rr[h] = zero4;
                if (c < NC && i < r) rr[h] = *(const u32x4*)(A + (size_t)(j * r + i) * lda + k0 + 8 * pc);
            }
            lw_store_pair_t(sAt, LS, 8 * pc, q, rr[0], rr[1]);
        }
        __syncthreads();
        f32x4 acc[2][4];            // DROP: the running total of the adapters' masked sums, before the 1 / (1 - p)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (DROP) {
            const bf16x8 zero8 = __builtin_bit_cast(bf16x8, zero4);
            for (int j = 0; j < n; ++j) {
                const int c_lo = j * rp, c_hi = c_lo + rp;
                f32x4 aj[2][4];
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) aj[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < LWU_MAXKS; ++ks) {
                    if (ks < nks && ks * 32 + 32 > c_lo && ks * 32 < c_hi) {
                        const int c = ks * 32 + 8 * fq;
                        const bool mine = c >= c_lo && c < c_hi;
                        const bf16x8 d0 = mine ? dtf[0][ks] : zero8, d1 = mine ? dtf[1][ks] : zero8;
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) {
                            const bf16x8 af = lw_frag(sAt + (ct * 16 + fr) * LS + ks * 32 + 8 * fq);
                            aj[0][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, d0, aj[0][ct], 0, 0, 0);
                            aj[1][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, d1, aj[1][ct], 0, 0, 0);
                        }
                    }
                }
                // D[row = column k0 + 16ct + 4fq + reg][col = row fr of the row tile]
                const unsigned long long off = lora_site_offset(dr.site0 + j);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    const unsigned long long e4 = (eb[rt] + k0 + 4 * fq) >> 2;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        unsigned rnd[4];
                        keep_words4(off + e4 + 4 * ct, dr.seed, rnd);
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[rt][ct][q] += rnd[q] >= dr.thresh ? aj[rt][ct][q] : 0.f;
                    }
                }
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < LWU_MAXKS; ++ks) {
                if (ks < nks) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const bf16x8 af = lw_frag(sAt + (ct * 16 + fr) * LS + ks * 32 + 8 * fq);
#pragma unroll
                        for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, dtf[rt][ks], acc[rt][ct], 0, 0, 0);
                    }
                }
            }
        }
        // D[row = column k0 + 16ct + 4fq + reg][col = row fr of the row tile]
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const long long m = row0 + rt * 16 + fr;
            if (m < M) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    u32x2* px = (u32x2*)(dX + (size_t)m * ldx + k0 + ct * 16 + 4 * fq);
                    const u32x2 old = *px;
                    const float lo0 = __uint_as_float(old[0] << 16), hi0 = __uint_as_float(old[0] & 0xffff0000u);
                    const float lo1 = __uint_as_float(old[1] << 16), hi1 = __uint_as_float(old[1] & 0xffff0000u);
                    const f32x4 a = acc[rt][ct];
                    u32x2 o;
                    if constexpr (DGELU) {         // the masked sum times gelu'(U[m, k..k+3]) / (1 - p), then the one add and rounding
                        const u32x2 u2 = upre[rt][ct];
                        const float g0 = dr.inv_keep * gelu_tanh_grad_f(__uint_as_float(u2[0] << 16));
                        const float g1 = dr.inv_keep * gelu_tanh_grad_f(__uint_as_float(u2[0] & 0xffff0000u));
                        const float g2 = dr.inv_keep * gelu_tanh_grad_f(__uint_as_float(u2[1] << 16));
                        const float g3 = dr.inv_keep * gelu_tanh_grad_f(__uint_as_float(u2[1] & 0xffff0000u));
                        o[0] = pack2(lo0 + g0 * a[0], hi0 + g1 * a[1]);
                        o[1] = pack2(lo1 + g2 * a[2], hi1 + g3 * a[3]);
                    } else if constexpr (DROP) {          // one expression per element: the multiply and the add contract into an fma
                        o[0] = pack2(lo0 + dr.inv_keep * a[0], hi0 + dr.inv_keep * a[1]);
                        o[1] = pack2(lo1 + dr.inv_keep * a[2], hi1 + dr.inv_keep * a[3]);
                    } else {
                        o[0] = pack2(lo0 + a[0], hi0 + a[1]);
                        o[1] = pack2(lo1 + a[2], hi1 + a[3]);
                    }
                    *px = o;
                }
            }
        }
    }
}
// dr == nullptr: no dropout
static int lora_up_add_wide_launch(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r, int rp,
                                   long long M, int K, const LoraDrop* dr, const LoraOrigin* og, void* stream,
                                   const LoraDgelu* dg = nullptr) {
    if (M <= 0 || K <= 0 || (K % 64) || n_adapters <= 0 || r <= 0 || r > 128 || rp < r || (rp % 16) ||
        n_adapters * rp > 32 * LWU_MAXKS || (ldx % 4) || ldx < K || (ldt % 8) || ldt < n_adapters * rp || (lda % 8))
        return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)dT) | ((uintptr_t)A)) & 15) return VT_ERR_BAD_ALIGN;
    if (((uintptr_t)dX) & 7) return VT_ERR_BAD_ALIGN;
    if (dg != nullptr) {
        if (dr == nullptr || dg->U == nullptr || (dg->ldu % 4) || dg->ldu < K) return VT_ERR_BAD_SHAPE;
        if (((uintptr_t)dg->U) & 7) return VT_ERR_BAD_ALIGN;
    }
    const long long blocks = (M + 127) / 128;
    if (blocks > 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    const int NCp = (n_adapters * rp + 31) & ~31;
    const size_t lds = (size_t)64 * (NCp + LW_PAD) * sizeof(bf16_t);
    if (dr == nullptr)
        hipLaunchKernelGGL(lora_wide_up_add_kernel<>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, (bf16_t*)dX, ldx,
                           (const bf16_t*)dT, ldt, (const bf16_t*)A, lda, n_adapters, r, rp, M, K);
    else if (dg != nullptr)
        hipLaunchKernelGGL((lora_wide_up_add_kernel<LoraDrop, LoraOrigin, LoraDgelu>), dim3((unsigned)blocks), dim3(256), lds,
                           (hipStream_t)stream, (bf16_t*)dX, ldx, (const bf16_t*)dT, ldt, (const bf16_t*)A, lda, n_adapters, r, rp, M, K, *dr,
                           *og, *dg);
    else
        hipLaunchKernelGGL((lora_wide_up_add_kernel<LoraDrop, LoraOrigin>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream,
                           (bf16_t*)dX, ldx, (const bf16_t*)dT, ldt, (const bf16_t*)A, lda, n_adapters, r, rp, M, K, *dr, *og);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
extern "C" int vt_lora_up_add_wide(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r, int rp,
                                   long long M, int K, void* stream) {
    return lora_up_add_wide_launch(dX, ldx, dT, ldt, A, lda, n_adapters, r, rp, M, K, nullptr, nullptr, stream);
}
extern "C" int vt_lora_up_add_wide_drop(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r, int rp,
                                        long long M, int K, float p, unsigned long long seed, int site0, void* stream) {
    if (vt_lora_drop_bad(p, site0)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0);
    const LoraOrigin og = vt_lora_origin_identity(M, K);
    return lora_up_add_wide_launch(dX, ldx, dT, ldt, A, lda, n_adapters, r, rp, M, K, &dr, &og, stream);
}
// _at: dX holds the rows / columns of the adapters' logical input gradient that the origin map names
extern "C" int vt_lora_up_add_wide_drop_at(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r,
                                           int rp, long long M, int K, float p, unsigned long long seed, int site0, long long seg_local,
                                           long long seg_global, long long n_first, long long off_first, long long off_rest, int k0,
                                           int K_log, void* stream) {
    const LoraOrigin og = {seg_local, seg_global, n_first, off_first, off_rest, k0, K_log};
    if (vt_lora_drop_bad(p, site0) || vt_lora_origin_bad(og, M, K)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0);
    return lora_up_add_wide_launch(dX, ldx, dT, ldt, A, lda, n_adapters, r, rp, M, K, &dr, &og, stream);
}
// the dgelu form (lora.hip, lora_up_add_kernel): the masked sum times gelu'(U[m,k]), U the saved pre-activation of the GELU whose
// output the adapters read
extern "C" int vt_lora_up_add_wide_dgelu_drop(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r,
                                              int rp, const void* U, int ldu, long long M, int K, float p, unsigned long long seed,
                                              int site0, void* stream) {
    if (vt_lora_drop_bad(p, site0)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0);
    const LoraDgelu dg = {(const bf16_t*)U, ldu};
    const LoraOrigin og = vt_lora_origin_identity(M, K);
    return lora_up_add_wide_launch(dX, ldx, dT, ldt, A, lda, n_adapters, r, rp, M, K, &dr, &og, stream, &dg);
}
extern "C" int vt_lora_up_add_wide_dgelu_drop_at(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r,
                                                 int rp, const void* U, int ldu, long long M, int K, float p, unsigned long long seed,
                                                 int site0, long long seg_local, long long seg_global, long long n_first,
                                                 long long off_first, long long off_rest, int k0, int K_log, void* stream) {
    const LoraOrigin og = {seg_local, seg_global, n_first, off_first, off_rest, k0, K_log};
    if (vt_lora_drop_bad(p, site0) || vt_lora_origin_bad(og, M, K)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0);
    const LoraDgelu dg = {(const bf16_t*)U, ldu};
    return lora_up_add_wide_launch(dX, ldx, dT, ldt, A, lda, n_adapters, r, rp, M, K, &dr, &og, stream, &dg);
}

// ---------------- write (alpha/r) * B into the ext-column K-extension of the packed weight and of its transpose ----------------
// Bcat: [n_adapters * d_out, r] fp32 master (adapter j = rows [j*d_out, (j+1)*d_out)); adapter j owns the extension columns
// [j*rp, j*rp + r); every other extension element is written as zero.
__global__ void lora_pack_b_wide_kernel(const float* Bcat, bf16_t* Wext, int ldw, int n_adapters, int d_out, int r, int rp, int ext,
                                        float scale) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_adapters * d_out * ext) return;
    const int n = (int)(i / ext), c = (int)(i - (long long)n * ext);
    const int j = n / d_out;
    float v = 0.f;
    if (c >= j * rp && c < j * rp + r) v = scale * Bcat[(size_t)n * r + (c - j * rp)];
    Wext[(size_t)n * ldw + c] = f2bf(v);
}
// WT is [K + ext, N]; WText points at row K
__global__ void lora_pack_bt_wide_kernel(const float* Bcat, bf16_t* WText, int ldwt, int n_adapters, int d_out, int r, int rp, int ext,
                                         float scale) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int N = n_adapters * d_out;
    if (i >= (long long)ext * N) return;
    const int c = (int)(i / N), n = (int)(i - (long long)c * N);
    const int j = n / d_out;
    float v = 0.f;
    if (c >= j * rp && c < j * rp + r) v = scale * Bcat[(size_t)n * r + (c - j * rp)];
    WText[(size_t)c * ldwt + n] = f2bf(v);
}
static int lw_pack_args_bad(int n_adapters, int d_out, int r, int rp, int ext, int ld, int min_ld) {
    return n_adapters <= 0 || d_out <= 0 || r <= 0 || r > 128 || rp < r || ext < (n_adapters - 1) * rp + r || ld < min_ld;
}
extern "C" int vt_lora_pack_b_wide(const float* Bcat, void* Wext, int ldw, int n_adapters, int d_out, int r, int rp, int ext, float scale,
                                   void* stream) {
    if (lw_pack_args_bad(n_adapters, d_out, r, rp, ext, ldw, ext)) return VT_ERR_BAD_SHAPE;
    const long long total = (long long)n_adapters * d_out * ext;
    hipLaunchKernelGGL(lora_pack_b_wide_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Bcat,
                       (bf16_t*)Wext, ldw, n_adapters, d_out, r, rp, ext, scale);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
extern "C" int vt_lora_pack_bt_wide(const float* Bcat, void* WText, int ldwt, int n_adapters, int d_out, int r, int rp, int ext,
                                    float scale, void* stream) {
    if (lw_pack_args_bad(n_adapters, d_out, r, rp, ext, ldwt, n_adapters * d_out)) return VT_ERR_BAD_SHAPE;
    const long long total = (long long)n_adapters * d_out * ext;
    hipLaunchKernelGGL(lora_pack_bt_wide_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Bcat,
                       (bf16_t*)WText, ldwt, n_adapters, d_out, r, rp, ext, scale);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

