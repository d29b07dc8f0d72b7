// LoRA side-path kernels of the narrow K-extension layout (at most 16 rank columns per call: ranks 1..16; the kernels of ranks
// 17..128 are in lora_wide.hip).  Semantics follow peft 0.12 LoraLayer as injected by the
// reference at videotuna/models/cogvideo_hf/cogvideo_pl.py:143-149 with configs/004_cogvideox/cogvideo2b.yaml:32-38:
//     y = W x + b + (alpha/r) * B (A x)
// The engine folds the up-projection into the base GEMM by extending K: the activation buffer carries
// T = x A^T in extra columns and the weight carries (alpha/r) * B there, so forward and dX need no
// special GEMM; these kernels produce T, the rank-r gradients, and the rank-r correction of dX.
#include "common.h"
#include <cstdlib>

// lora_dropout > 0 (peft: y = W x + b + (alpha/r) B A drop(x), one nn.Dropout per adapted Linear): each of the three rank-side
// products below is one kernel template whose dropped form is a compile-time choice.  Nothing is stored: a dropped kernel
// recomputes the keep mask of adapter site s from (seed, s, element index) -- element (m, k) of the logical [M, K] adapter input
// is e = m * K + k whatever ldx is, kept iff word e % 4 of Philox(key = seed, counter = (s << 36) + e / 4) >= thresh (common.h;
// oracle/philox.py).  The n adapters that share a call (n * r = R rank columns, adapter j = columns [j r, (j+1) r), site site0 + j)
// read the same X under n different masks.  1 / (1 - p) multiplies the fp32 sums, never a re-rounded bf16 operand.
// A kernel's trailing argument pack is empty (no dropout) or one LoraDrop (common.h), so the undropped instantiation has the
// argument list and the code it had before lora_dropout existed.
static int lora_drop_args_bad(int R, int n, float p, int site0) {
    return n <= 0 || n > 3 || R <= 0 || R > 16 || (R % n) || vt_lora_drop_bad(p, site0);
}

// ---------------- T[M,16] = X[M,K] * A[R,K]^T  (R <= 16 rows valid, rest zero) -> bf16 ----------------
// one wave per 16 rows, v_mfma_f32_16x16x32_bf16; each lane streams 32 contiguous bytes of its row per
// 64-deep K block so every row is read in full 128-byte lines.
// DROP: T[m, j r + i] = 1/(1-p) sum_k keep_j(m,k) X[m,k] A[j r + i, k], one MFMA pair per adapter: the x fragment masked for adapter j
// against an A fragment that is zero in every other adapter's rows, all into the one accumulator (adapter j's MFMA adds exact zeros
// to the other columns).
template <typename... D>
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* X, int ldx, const bf16_t* A, int lda, int R,
                                                       bf16_t* T, int ldt, long long M, int K, int zero_cols, D... drop) {
    constexpr bool DROP = sizeof...(D) > 0;
    const LoraDrop dr = lora_drop_arg(drop...);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = ((long long)blockIdx.x * 4 + wave) * 16;
    if (row0 >= M) return;
    const int fr = lane & 15, fq = lane >> 4;
    long long xr = row0 + fr;
    if (xr > M - 1) xr = M - 1;
    const bf16_t* xp = X + (size_t)xr * ldx + 16 * fq;
    const bool aok = fr < R;
    const bf16_t* ap = A + (size_t)(aok ? fr : 0) * lda + 16 * fq;
    const int ja = DROP ? fr / dr.r : 0;             // the adapter that owns this lane's row of A
    const unsigned long long e4 = DROP ? ((unsigned long long)xr * K + 16 * fq) >> 2 : 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int k = 0; k < K; k += 64) {
        const u32x4 x0 = *(const u32x4*)(xp + k), x1 = *(const u32x4*)(xp + k + 8);
        const u32x4 a0 = aok ? *(const u32x4*)(ap + k) : zero;
        const u32x4 a1 = aok ? *(const u32x4*)(ap + k + 8) : zero;
        if constexpr (DROP) {
            for (int j = 0; j < dr.n; ++j) {
                const unsigned long long ctr = lora_site_offset(dr.site0 + j) + e4 + (k >> 2);
                const u32x4 m0 = keep_mask8(x0, ctr, dr.seed, dr.thresh), m1 = keep_mask8(x1, ctr + 2, dr.seed, dr.thresh);
                const bool mine = ja == j;
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, m0), __builtin_bit_cast(bf16x8, mine ? a0 : zero), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, m1), __builtin_bit_cast(bf16x8, mine ? a1 : zero), acc, 0, 0, 0);
            }
        } else {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x0), __builtin_bit_cast(bf16x8, a0), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x1), __builtin_bit_cast(bf16x8, a1), acc, 0, 0, 0);
        }
    }
    // D[row = 4*fq + reg][col = fr]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long m = row0 + 4 * fq + j;
        if (m < M) T[(size_t)m * ldt + fr] = f2bf(DROP ? dr.inv_keep * acc[j] : acc[j]);
    }
    // the rest of the K-extension must be exactly zero (the packed weight is zero there, but 0 * NaN is NaN)
    for (int idx = lane; idx < 16 * zero_cols; idx += 64) {
        const int rr = idx / zero_cols, cc = idx - rr * zero_cols;
        if (row0 + rr < M) T[(size_t)(row0 + rr) * ldt + 16 + cc] = f2bf(0.f);
    }
}
// dr == nullptr: no dropout
static int lora_down_launch(const void* X, int ldx, const void* A, int lda, int R, void* T, int ldt, long long M, int K, int zero_cols,
                            const LoraDrop* dr, void* stream) {
    if (M <= 0 || K <= 0 || (K % 64) || R <= 0 || R > 16 || (ldx % 8) || (lda % 8) || ldt < 16 + zero_cols || zero_cols < 0)
        return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)X) | ((uintptr_t)A)) & 15) return VT_ERR_BAD_ALIGN;
    const long long blocks = (M + 63) / 64;
    if (dr == nullptr)
        hipLaunchKernelGGL(lora_down_kernel<>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X, ldx,
                           (const bf16_t*)A, lda, R, (bf16_t*)T, ldt, M, K, zero_cols);
    else
        hipLaunchKernelGGL(lora_down_kernel<LoraDrop>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X, ldx,
                           (const bf16_t*)A, lda, R, (bf16_t*)T, ldt, M, K, zero_cols, *dr);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
extern "C" int vt_lora_down(const void* X, int ldx, const void* A, int lda, int R, void* T, int ldt, long long M, int K,
                            int zero_cols, void* stream) {
    return lora_down_launch(X, ldx, A, lda, R, T, ldt, M, K, zero_cols, nullptr, stream);
}
extern "C" int vt_lora_down_drop(const void* X, int ldx, const void* A, int lda, int R, int n_adapters, void* T, int ldt, long long M,
                                 int K, int zero_cols, float p, unsigned long long seed, int site0, void* stream) {
    if (lora_drop_args_bad(R, n_adapters, p, site0)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0, n_adapters, R / n_adapters);
    return lora_down_launch(X, ldx, A, lda, R, T, ldt, M, K, zero_cols, &dr, stream);
}

// ---------------- out[p*osp + r*osr] += alpha * sum_m Big[m,p] * Small[m,r] ----------------
// The output is tiny (P x R) while M is long, so the reduction is split over SK_SLICES row slices.  Contended fp32
// atomics into such a small target run at ~0.1 TB/s (MI355X_MICROARCH.md, global float atomics), so when the caller
// provides a workspace the slices write their partial [P, RR] tiles with plain stores and a second tiny kernel sums
// them in a fixed order (also bitwise reproducible); without a workspace the partials are added with atomics.
// Columns: 512-wide blocks of 128 threads (4 columns = one 8-byte load per thread and row), rows of a slice walked 16 at
// a time with all 16 loads in flight; the slice's Small rows are staged once in LDS as fp32.
// NA > 0: out += alpha/(1-p) * sum_m keep_{r / RPER}(m,p) Big[m,p] * Small[m,r], Big masked per rank-column group: a thread's 4
// columns of a row are exactly one Philox counter per adapter (P % 4 == 0).  NA adapters of RPER rank columns each are compile-time
// so that the adapter of an accumulator column is; NA == 0 is the product without a mask.
#define SK_SLICES 192          // r01 (M=35552, P=1920): with the partial sums transposed through LDS (contiguous atomics) 96 / 192 / 384 slices
                               // -> 49 / 35 / 37 us for R=4 (3.9 TB/s), 126 / 83 / 99 us for R=12; before the transpose every lane's 16 adds hit
                               // 16 lines of their own and the kernel took 90-110 us whatever the slice count
#define SK_COPIES 8
#define SK_MAXROWS 512         // rows per slice that fit the LDS staging
// acc[c][rr] += Big[m, p + c] * Small[m, rr] for one row m: raw = the thread's 4 columns of Big, srow = the staged Small row
template <int RR, int NA, int RPER>
__device__ __forceinline__ void sk_row(const u32x2 raw, const float* srow, unsigned long long e4, const LoraDrop& dr, float (&acc)[4][RR]) {
    const float b[4] = {__uint_as_float(raw[0] << 16), __uint_as_float(raw[0] & 0xffff0000u), __uint_as_float(raw[1] << 16),
                        __uint_as_float(raw[1] & 0xffff0000u)};
    float bm[NA > 0 ? NA : 1][4];
    if constexpr (NA > 0) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            unsigned rnd[4];
            keep_words4(lora_site_offset(dr.site0 + j) + e4, dr.seed, rnd);
#pragma unroll
            for (int c = 0; c < 4; ++c) bm[j][c] = rnd[c] >= dr.thresh ? b[c] : 0.f;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) bm[0][c] = b[c];
    }
#pragma unroll
    for (int r4 = 0; r4 < RR / 4; ++r4) {
        const f32x4 s = *(const f32x4*)(srow + 4 * r4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rr = 4 * r4 + j;
            const int ja = NA == 0 ? 0 : rr / RPER < NA ? rr / RPER : NA - 1;      // columns >= R carry Small = 0
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c][rr] += bm[ja][c] * s[j];
        }
    }
}
template <int RR, int NA, int RPER, typename... D>
__global__ __launch_bounds__(128) void skinny_tn_kernel(const bf16_t* Big, int ldb, const bf16_t* Small, int lds_, int R,
                                                       float* out, long long osp, long long osr, float alpha,
                                                       long long M, int P, int rows_per_slice, float* ws, D... drop) {
    static_assert((NA > 0) == (sizeof...(D) > 0), "the mask needs the dropout argument");
    const LoraDrop dr = lora_drop_arg(drop...);
    __shared__ __attribute__((aligned(16))) float sm[SK_MAXROWS * RR];
    const long long m0 = (long long)blockIdx.y * rows_per_slice;
    const int p = (blockIdx.x * 128 + threadIdx.x) * 4;
    const int rows = m0 < M ? (int)((M - m0) < rows_per_slice ? (M - m0) : rows_per_slice) : 0;
    for (int i = threadIdx.x; i < rows * RR; i += 128) {
        const int mm = i / RR, rr = i - mm * RR;
        sm[i] = rr < R ? bf2f(Small[(size_t)(m0 + mm) * lds_ + rr]) : 0.f;
    }
    __syncthreads();
    const bool valid = p < P;                    // (no early return: the epilogue below has block barriers)
    float acc[4][RR];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int rr = 0; rr < RR; ++rr) acc[c][rr] = 0.f;
    const bf16_t* bp = Big + (size_t)m0 * ldb + (valid ? p : 0);
    const unsigned long long e40 = NA > 0 ? ((unsigned long long)(dr.mbase + m0) * P + p) >> 2 : 0, estep = (unsigned long long)(P >> 2);
    int mb = 0;
    for (; valid && mb + 16 <= rows; mb += 16) {
        u32x2 raw[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) raw[u] = *(const u32x2*)(bp + (size_t)(mb + u) * ldb);
#pragma unroll
        for (int u = 0; u < 16; ++u) sk_row<RR, NA, RPER>(raw[u], sm + (mb + u) * RR, e40 + (mb + u) * estep, dr, acc);
    }
    for (; valid && mb < rows; ++mb)
        sk_row<RR, NA, RPER>(*(const u32x2*)(bp + (size_t)mb * ldb), sm + mb * RR, e40 + mb * estep, dr, acc);
    if (ws != nullptr) {
        if (!valid) return;
        // SK_COPIES zeroed copies of the [P, RR] result: slice s adds into copy s % SK_COPIES, so an address sees
        // SK_SLICES / SK_COPIES adds instead of SK_SLICES (same-address fp32 atomics serialise at ~0.5 us each)
        float* w = ws + ((size_t)(blockIdx.y % SK_COPIES) * P + p) * RR;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int rr = 0; rr < RR; ++rr)
                if (rr < R) atomicAdd(w + c * RR + rr, acc[c][rr]);
    } else {
        // A lane's 16 partial sums are 16 different cache lines for its neighbours' (a wave instruction = 64 lines with one
        // dword each: ~17 G adds/s, 20x below the atomic units' rate).  Transpose through LDS so that every atomic instruction
        // adds 64 CONSECUTIVE floats of the output: [p][r] order when the r index is the fast one (osr == 1), else [r][p].
        __syncthreads();                                   // every thread of the block is done with the staged Small rows
        const int pl = threadIdx.x * 4;                    // first of this thread's 4 columns inside the block's 512
        const int pb0 = blockIdx.x * 512;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int rr = 0; rr < RR; ++rr) sm[(pl + c) * RR + rr] = alpha * acc[c][rr];     // 512 x RR floats <= SK_MAXROWS x RR
        __syncthreads();
        if (osr == 1) {
            for (int i = threadIdx.x; i < 512 * RR; i += 128) {
                const int pp = i / RR, rr = i - pp * RR;
                if (rr < R && pb0 + pp < P) atomicAdd(out + (size_t)(pb0 + pp) * osp + rr, sm[i]);
            }
        } else {
            for (int rr = 0; rr < R; ++rr)
                for (int pp = threadIdx.x; pp < 512; pp += 128)
                    if (pb0 + pp < P) atomicAdd(out + (size_t)(pb0 + pp) * osp + (size_t)rr * osr, sm[pp * RR + rr]);
        }
    }
}
template <int RR>
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const float* ws, int nslices, float* out, long long osp, long long osr,
                                                           float alpha, int P, int R) {
    const int i = blockIdx.x * 256 + threadIdx.x;          // one (p, rr) pair per thread
    if (i >= P * RR) return;
    const int p = i / RR, rr = i - p * RR;
    if (rr >= R) return;
    float s = 0.f;
    for (int k = 0; k < nslices; ++k) s += ws[(size_t)k * P * RR + i];
    out[(size_t)p * osp + (size_t)rr * osr] += alpha * s;
}
extern "C" long long vt_skinny_tn_workspace_bytes(int P) { return (long long)SK_COPIES * P * 16 * 4; }
#define SK_ARGS bg, ldb, smp, lds_, R, out, osp, osr, alpha, mc, P, rps, workspace
#define SK_DROP_LAUNCH(RR_, NA_, RPER_) \
    hipLaunchKernelGGL((skinny_tn_kernel<RR_, NA_, RPER_, LoraDrop>), grid, dim3(128), 0, st, SK_ARGS, drm)
// nsl row slices per launch; dr == nullptr: no dropout, else alpha carries the 1 / (1 - p)
static int skinny_tn_launch(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp, long long osr,
                            float alpha, long long M, int P, float* workspace, int nsl, const LoraDrop* dr, void* stream) {
    if (M <= 0 || P <= 0 || (P % 4) || R <= 0 || R > 16 || (ldb % 4)) return VT_ERR_BAD_SHAPE;
    if (((uintptr_t)Big) & 7) return VT_ERR_BAD_ALIGN;
    if (workspace != nullptr && (((uintptr_t)workspace) & 15)) return VT_ERR_BAD_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const long long chunk = (long long)nsl * SK_MAXROWS;          // rows handled per launch
    const int RRw = R <= 4 ? 4 : 16;
    if (workspace != nullptr && hipMemsetAsync(workspace, 0, (size_t)SK_COPIES * P * RRw * 4, st) != hipSuccess) return VT_ERR_LAUNCH;
    for (long long mbase = 0; mbase < M; mbase += chunk) {
        const long long mc = (M - mbase) < chunk ? (M - mbase) : chunk;
        const int rps = (int)((mc + nsl - 1) / nsl);
        dim3 grid((P + 511) / 512, nsl);
        const bf16_t* bg = (const bf16_t*)Big + (size_t)mbase * ldb;
        const bf16_t* smp = (const bf16_t*)Small + (size_t)mbase * lds_;
        if (dr == nullptr) {
            if (R <= 4) hipLaunchKernelGGL((skinny_tn_kernel<4, 0, 1>), grid, dim3(128), 0, st, SK_ARGS);
            else hipLaunchKernelGGL((skinny_tn_kernel<16, 0, 1>), grid, dim3(128), 0, st, SK_ARGS);
        } else {
            LoraDrop drm = *dr;
            drm.mbase = mbase;
            if (dr->n == 1) {
                if (R <= 4) SK_DROP_LAUNCH(4, 1, 16); else SK_DROP_LAUNCH(16, 1, 16);
            } else if (dr->r == 1) SK_DROP_LAUNCH(4, 3, 1);
            else if (dr->r == 2) SK_DROP_LAUNCH(16, 3, 2);
            else if (dr->r == 3) SK_DROP_LAUNCH(16, 3, 3);
            else if (dr->r == 4) SK_DROP_LAUNCH(16, 3, 4);
            else SK_DROP_LAUNCH(16, 3, 5);
        }
    }
    if (workspace != nullptr) {
        if (R <= 4) hipLaunchKernelGGL(skinny_reduce_kernel<4>, dim3((P * 4 + 255) / 256), dim3(256), 0, st, workspace, SK_COPIES, out, osp, osr, alpha, P, R);
        else hipLaunchKernelGGL(skinny_reduce_kernel<16>, dim3((P * 16 + 255) / 256), dim3(256), 0, st, workspace, SK_COPIES, out, osp, osr, alpha, P, R);
    }
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
#undef SK_DROP_LAUNCH
#undef SK_ARGS
extern "C" int vt_skinny_tn(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp,
                            long long osr, float alpha, long long M, int P, float* workspace, void* stream) {
    static int slices_env = -1;
    if (slices_env < 0) { const char* e = getenv("VT_SK_SLICES"); slices_env = e ? atoi(e) : 0; }
    const int nsl = (slices_env > 0 && slices_env <= 1024) ? slices_env : SK_SLICES;
    return skinny_tn_launch(Big, ldb, Small, lds_, R, out, osp, osr, alpha, M, P, workspace, nsl, nullptr, stream);
}
extern "C" int vt_skinny_tn_drop(const void* Big, int ldb, const void* Small, int lds_, int R, int n_adapters, float* out, long long osp,
                                 long long osr, float alpha, long long M, int P, float* workspace, float p, unsigned long long seed,
                                 int site0, void* stream) {
    if (lora_drop_args_bad(R, n_adapters, p, site0) || n_adapters == 2) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0, n_adapters, R / n_adapters);
    return skinny_tn_launch(Big, ldb, Small, lds_, R, out, osp, osr, alpha * dr.inv_keep, M, P, workspace, SK_SLICES, &dr, stream);
}

// ---------------- dX[m,k] += sum_r dT[m,r] * A[r,k]   (in place, bf16) ----------------
// DROP: dX[m,k] += 1/(1-p) sum_j keep_j(m,k) sum_i dT[m, j r + i] * A[j r + i, k]: each adapter's partial sum is masked before the
// adapters are added
// DGELU (a LoraDrop and a LoraDgelu trail): dX[m,k] += gelu'(U[m,k]) 1/(1-p) sum_j keep_j(m,k) sum_i ..., the dropped correction of an adapter
// whose input is gelu(U) (ff.net.2) added to a dX that already carries gelu'(U) (x) (dY W): the mask sits between dT A and the GELU, so
// this term cannot ride in the W^T product's K-extension.  gelu' is the EPI_DGELU epilogue's function; it multiplies the fp32 sum.
template <typename... D>
__global__ __launch_bounds__(256) void lora_up_add_kernel(bf16_t* dX, int ldx, const bf16_t* dT, int ldt, const bf16_t* A, int lda,
                                                         int R, long long M, int K, D... drop) {
    constexpr bool DROP = sizeof...(D) > 0, DGELU = sizeof...(D) > 1;
    const LoraDrop dr = lora_drop_arg(drop...);
    const LoraDgelu dg = lora_dgelu_arg(drop...);
    const int n = DROP ? dr.n : 1, r = DROP ? dr.r : R;          // no dropout: one group of all R rank rows
    const int nch = K >> 3;
    const long long total = M * nch;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long m = i / nch;
        const int c = (int)(i - m * nch);
        float v[8];
        unpack8(*(const u32x4*)(dX + (size_t)m * ldx + c * 8), v);
        float g[8];
        if constexpr (DGELU) {
            unpack8(*(const u32x4*)(dg.U + (size_t)m * dg.ldu + c * 8), g);
#pragma unroll
            for (int q = 0; q < 8; ++q) g[q] = dr.inv_keep * gelu_tanh_grad_f(g[q]);
        }
        for (int j = 0; j < n; ++j) {
            float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float(&acc)[8] = DROP ? s : v;          // without a mask the sum goes straight into v
            for (int ri = j * r; ri < (j + 1) * r; ++ri) {
                const float t = bf2f(dT[(size_t)m * ldt + ri]);
                float a[8];
                unpack8(*(const u32x4*)(A + (size_t)ri * lda + c * 8), a);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] += t * a[q];
            }
            if constexpr (DROP) {
                unsigned rnd[8];
                const unsigned long long ctr = lora_site_offset(dr.site0 + j) + (((unsigned long long)m * K + 8 * c) >> 2);
                keep_words4(ctr, dr.seed, rnd);
                keep_words4(ctr + 1, dr.seed, rnd + 4);
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] += rnd[q] >= dr.thresh ? (DGELU ? g[q] : dr.inv_keep) * s[q] : 0.f;
            }
        }
        *(u32x4*)(dX + (size_t)m * ldx + c * 8) = pack8(v);
    }
}
// dr == nullptr: no dropout
static int lora_up_add_launch(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int R, long long M, int K,
                              const LoraDrop* dr, void* stream, const LoraDgelu* dg = nullptr) {
    if (M <= 0 || K <= 0 || (K % 8) || R <= 0 || R > 16 || (ldx % 8) || (lda % 8)) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)dX) | ((uintptr_t)A)) & 15) return VT_ERR_BAD_ALIGN;
    if (dg != nullptr) {
        if (dr == nullptr || dg->U == nullptr || (dg->ldu % 8) || dg->ldu < K || ldx < K || ldt < R) return VT_ERR_BAD_SHAPE;
        if (((uintptr_t)dg->U) & 15) return VT_ERR_BAD_ALIGN;
    }
    long long total = M * (K >> 3), b = (total + 255) / 256;
    const dim3 grid((unsigned)(b > 8192 ? 8192 : b));
    if (dr == nullptr)
        hipLaunchKernelGGL(lora_up_add_kernel<>, grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)dX, ldx, (const bf16_t*)dT, ldt,
                           (const bf16_t*)A, lda, R, M, K);
    else if (dg != nullptr)
        hipLaunchKernelGGL((lora_up_add_kernel<LoraDrop, LoraDgelu>), grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)dX, ldx,
                           (const bf16_t*)dT, ldt, (const bf16_t*)A, lda, R, M, K, *dr, *dg);
    else
        hipLaunchKernelGGL(lora_up_add_kernel<LoraDrop>, grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)dX, ldx, (const bf16_t*)dT, ldt,
                           (const bf16_t*)A, lda, R, M, K, *dr);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
extern "C" int vt_lora_up_add(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int R, long long M, int K,
                              void* stream) {
    return lora_up_add_launch(dX, ldx, dT, ldt, A, lda, R, M, K, nullptr, stream);
}
extern "C" int vt_lora_up_add_drop(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int R, int n_adapters, long long M,
                                   int K, float p, unsigned long long seed, int site0, void* stream) {
    if (lora_drop_args_bad(R, n_adapters, p, site0)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0, n_adapters, R / n_adapters);
    return lora_up_add_launch(dX, ldx, dT, ldt, A, lda, R, M, K, &dr, stream);
}
extern "C" int vt_lora_up_add_dgelu_drop(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int R, int n_adapters,
                                         const void* U, int ldu, long long M, int K, float p, unsigned long long seed, int site0,
                                         void* stream) {
    if (lora_drop_args_bad(R, n_adapters, p, site0)) return VT_ERR_BAD_SHAPE;
    const LoraDrop dr = vt_lora_drop(p, seed, site0, n_adapters, R / n_adapters);
    const LoraDgelu dg = {(const bf16_t*)U, ldu};
    return lora_up_add_launch(dX, ldx, dT, ldt, A, lda, R, M, K, &dr, stream, &dg);
}

// ---------------- write (alpha/r) * B[n, r] into the K-extension columns of the packed weight ----------------
// Bcat: [n_adapters * d_out, r] fp32 master (adapter j = rows [j*d_out, (j+1)*d_out)); Wext points at column K of the
// packed weight [n_adapters*d_out, ldw]; adapter j owns extension columns [j*r, (j+1)*r); the rest of the
// 64-column extension stays zero.
__global__ void lora_pack_b_kernel(const float* Bcat, bf16_t* Wext, int ldw, int n_adapters, int d_out, int r, float scale) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int total = n_adapters * d_out * 64;
    if (i >= total) return;
    const int n = i >> 6, c = i & 63;
    const int j = n / d_out;
    float v = 0.f;
    if (c >= j * r && c < (j + 1) * r) v = scale * Bcat[(size_t)n * r + (c - j * r)];
    Wext[(size_t)n * ldw + c] = f2bf(v);
}
extern "C" int vt_lora_pack_b(const float* Bcat, void* Wext, int ldw, int n_adapters, int d_out, int r, float scale,
                              void* stream) {
    if (n_adapters <= 0 || d_out <= 0 || r <= 0 || n_adapters * r > 64) return VT_ERR_BAD_SHAPE;
    const int total = n_adapters * d_out * 64;
    hipLaunchKernelGGL(lora_pack_b_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, Bcat, (bf16_t*)Wext, ldw,
                       n_adapters, d_out, r, scale);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// same for the transposed packed weight used by dX = dY * W:  WT is [K + 64, N]; rows K.. hold (alpha/r) * B^T
__global__ void lora_pack_bt_kernel(const float* Bcat, bf16_t* WText, int ldwt, int n_adapters, int d_out, int r, float scale) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int N = n_adapters * d_out;
    if (i >= 64 * N) return;
    const int c = i / N, n = i - c * N;
    const int j = n / d_out;
    float v = 0.f;
    if (c >= j * r && c < (j + 1) * r) v = scale * Bcat[(size_t)n * r + (c - j * r)];
    WText[(size_t)c * ldwt + n] = f2bf(v);
}
extern "C" int vt_lora_pack_bt(const float* Bcat, void* WText, int ldwt, int n_adapters, int d_out, int r, float scale,
                               void* stream) {
    if (n_adapters <= 0 || d_out <= 0 || r <= 0 || n_adapters * r > 64) return VT_ERR_BAD_SHAPE;
    const int total = n_adapters * d_out * 64;
    hipLaunchKernelGGL(lora_pack_bt_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, Bcat, (bf16_t*)WText, ldwt,
                       n_adapters, d_out, r, scale);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
