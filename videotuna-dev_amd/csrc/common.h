// Shared device helpers for the vt355 HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define VT_OK 0
#define VT_ERR_BAD_SHAPE (-1)
#define VT_ERR_BAD_ALIGN (-2)
#define VT_ERR_LAUNCH (-3)
#define VT_ERR_UNSUPPORTED (-4)

#define WAVE 64

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
    return __uint_as_float(((unsigned int)b) << 16);
}
__device__ __forceinline__ float bf2f(bf16_t x) { return (float)x; }
__device__ __forceinline__ bf16_t f2bf(float x) { return (bf16_t)x; }

// unpack 8 bf16 (one 16-byte chunk held as 4 dwords) into 8 floats
__device__ __forceinline__ void unpack8(const u32x4& v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(v[i] << 16);
        f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ unsigned int pack2(float lo, float hi) {
    bf16x2 p;
    p[0] = (bf16_t)lo;
    p[1] = (bf16_t)hi;
    return __builtin_bit_cast(unsigned int, p);
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = pack2(f[2 * i], f[2 * i + 1]);
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// max |x| into an amax slot: a uint32 holding non-negative float bits (they order as the floats do), cleared between the kernels that
// publish to it.  Thousands of waves publishing to ONE address serialise in the L2 atomic unit (profiles/r05_amax_publish_ab.txt), so a
// publisher first reads the slot -- it only grows while producers run, a stale read is a smaller value -- and skips the atomic when it
// could not raise it.  VT_AMAX_ALWAYS_ATOMIC: the unconditional atomic, for that A/B only.
__device__ __forceinline__ void amax_publish(unsigned int* slot, float v) {
    const unsigned int b = __float_as_uint(v);
#ifdef VT_AMAX_ALWAYS_ATOMIC
    atomicMax(slot, b);
#else
    if (b > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, b);
#endif
}

// tanh-GELU as x * sigmoid(2u), u = k0 (x + k1 x^3): sigmoid(2u) = 1 - 1 / (2^(2 log2e u) + 1) with the hardware exp2 / rcp
// (no IEEE division: these run in GEMM epilogues while the matrix pipe waits).  Saturates correctly: 2^w = inf -> s = 1,
// 2^w = 0 -> s = 0.
__device__ __forceinline__ float gelu_sigmoid_f(float x, float x2) {
    const float c0 = 2.0f * 1.4426950408889634f * 0.7978845608028654f, c1 = c0 * 0.044715f;
    const float w = x * __builtin_fmaf(c1, x2, c0);
    return 1.0f - __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(w) + 1.0f);
}
__device__ __forceinline__ float gelu_tanh_f(float x) { return x * gelu_sigmoid_f(x, x * x); }
// d/dx [x s(x)] = s + x s (1 - s) * 2 du/dx,  du/dx = k0 (1 + 3 k1 x^2)
__device__ __forceinline__ float gelu_tanh_grad_f(float x) {
    const float k0 = 0.7978845608028654f, k1 = 0.044715f;
    const float x2 = x * x;
    const float sg = gelu_sigmoid_f(x, x2);
    const float du2 = __builtin_fmaf(6.0f * k0 * k1, x2, 2.0f * k0);
    return __builtin_fmaf(x * du2, sg * (1.0f - sg), sg);
}
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }

// buffer resource for bounds-checked (OOB reads return 0, OOB stores dropped) raw buffer ops
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// Bijective XCD-aware remap of a linear workgroup id (8 XCDs, round-robin dispatch): consecutive
// logical ids land on the same XCD so neighbouring tiles share that XCD's L2.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int nx = 8;
    int q = nwg / nx, r = nwg % nx;
    int xcd = orig % nx;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + orig / nx;
}
// rotary position embedding helpers (fp32 tables [S - St, 64]; pairs (2i, 2i+1) live in one lane's 8 elements)
__device__ __forceinline__ void rope_load8(const float* src, float* d) {
    f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { d[j] = a[j]; d[j + 4] = b[j]; }
}
// transpose of the rotation: applied to an incoming gradient
__device__ __forceinline__ void rope_bwd8(const float* rope_cos, const float* rope_sin, int spos, int sub, float* dy) {
    float cs[8], sn[8];
    rope_load8(rope_cos + (size_t)spos * 64 + sub * 8, cs);
    rope_load8(rope_sin + (size_t)spos * 64 + sub * 8, sn);
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const float a = dy[j], b = dy[j + 1];
        dy[j] = a * cs[j] + b * sn[j + 1];
        dy[j + 1] = b * cs[j + 1] - a * sn[j];
    }
}

// Philox4x32-10 (Salmon et al., SC'11; Random123): the counter-based generator behind every stateless dropout mask of the library
// (oracle/philox.py restates it in numpy).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// The dropout mask convention shared by vt_dropout_bf16 and the LoRA _drop kernels: element e of a logical [M, C] array (e = m * C + c) is
// kept iff word e % 4 of Philox(key = seed, counter = offset + e / 4) >= thresh, thresh = floor(p * 2^32) saturated to 2^32 - 1.
static inline unsigned vt_keep_thresh(float p) {
    const double t = (double)p * 4294967296.0;
    return t >= 4294967295.0 ? 0xffffffffu : (unsigned)t;
}
// the 4 mask words of counter ctr
__device__ __forceinline__ void keep_words4(unsigned long long ctr, unsigned long long seed, unsigned* rnd) {
    philox4x32_10((unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), rnd);
}
// 8 consecutive bf16 (4 dwords) whose first element has counter ctr: dropped elements become +0
__device__ __forceinline__ u32x4 keep_mask8(u32x4 v, unsigned long long ctr, unsigned long long seed, unsigned thresh) {
    unsigned rnd[8];
    keep_words4(ctr, seed, rnd);
    keep_words4(ctr + 1, seed, rnd + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] &= (rnd[2 * i] >= thresh ? 0x0000ffffu : 0u) | (rnd[2 * i + 1] >= thresh ? 0xffff0000u : 0u);
    return v;
}
// counter offset of adapter site s: 2^36 counters = 2^38 elements per site
__device__ __forceinline__ unsigned long long lora_site_offset(int site) { return (unsigned long long)site << 36; }
// The arguments that only a dropped LoRA rank-side kernel has.  Each of those kernels is a template whose trailing argument pack is one
// LoraDrop or empty: the undropped instantiation then has no such kernel argument at all (an empty struct would still take a byte and
// move the hidden arguments behind it) and `if constexpr` leaves none of the mask code in it.
struct LoraDrop {
    unsigned thresh;
    float inv_keep;          // 1 / (1 - p)
    unsigned long long seed;
    int site0;               // adapter j of a call is site site0 + j
    // read by the kernels of lora.hip only (lora_wide.hip takes n, r, rp with or without dropout and leaves these unread):
    int n, r;                // lora_down, lora_up_add: the n adapters of r rank rows each that share the call
    long long mbase;         // skinny_tn: the launch's first row within the call (the mask's element index counts rows of the whole input)
};
__device__ __forceinline__ LoraDrop lora_drop_arg() { return LoraDrop{}; }
__device__ __forceinline__ LoraDrop lora_drop_arg(const LoraDrop& d) { return d; }
// A second trailing argument selects the dgelu form of a dropped dX correction (the backward of an adapter whose input is a GELU
// output, ff.net.2): the masked sum is multiplied by gelu'(U[m,k]) before it is added.  U: the saved pre-activation, row stride ldu.
struct LoraDgelu {
    const bf16_t* U;
    int ldu;
};
__device__ __forceinline__ LoraDrop lora_drop_arg(const LoraDrop& d, const LoraDgelu&) { return d; }
__device__ __forceinline__ LoraDgelu lora_dgelu_arg() { return LoraDgelu{nullptr, 0}; }
__device__ __forceinline__ LoraDgelu lora_dgelu_arg(const LoraDrop&) { return LoraDgelu{nullptr, 0}; }
__device__ __forceinline__ LoraDgelu lora_dgelu_arg(const LoraDrop&, const LoraDgelu& g) { return g; }
static inline LoraDrop vt_lora_drop(float p, unsigned long long seed, int site0, int n = 0, int r = 0) {
    return LoraDrop{vt_keep_thresh(p), 1.0f / (1.0f - p), seed, site0, n, r, 0};
}
static inline int vt_lora_drop_bad(float p, int site0) { return !(p >= 0.f) || !(p < 1.f) || site0 < 0 || site0 > (1 << 20); }
// The origin map of a dropped wide-layout kernel (lora_wide.hip; the pack is LoraDrop, LoraOrigin [, LoraDgelu]): where the call's
// [M, K] operand sits inside the adapter's logical input [M_g, K_log], whose element index e = m_g * K_log + k_g keys the mask.  The call
// may hold a subset of the logical rows (one rank's rows under sequence parallelism) and a column range of the logical width:
//   rows     b = m / seg_local, l = m % seg_local,  m_g = b * seg_global + l + (l < n_first ? off_first : off_rest)
//   columns  k_g = k0 + k
// The identity map (seg_local = seg_global >= M, no offsets, k0 = 0, K_log = K) is what the plain _drop entry points pass.
struct LoraOrigin {
    long long seg_local, seg_global, n_first, off_first, off_rest;
    int k0, K_log;
};
static inline LoraOrigin vt_lora_origin_identity(long long M, int K) { return LoraOrigin{M > 0 ? M : 1, M > 0 ? M : 1, 0, 0, 0, 0, K}; }
__host__ __device__ __forceinline__ long long lora_origin_row(const LoraOrigin& o, long long m) {
    const long long b = m / o.seg_local, l = m - b * o.seg_local;
    return b * o.seg_global + l + (l < o.n_first ? o.off_first : o.off_rest);
}
// index of element (m, 0) of the call's operand within the logical input
__device__ __forceinline__ unsigned long long lora_origin_elem(const LoraOrigin& o, long long m) {
    return (unsigned long long)lora_origin_row(o, m) * (unsigned long long)o.K_log + (unsigned long long)o.k0;
}
// a map no kernel may be launched with: a column range off the 8-element chunks or outside the logical width, a logical width that
// splits a Philox counter between two rows, a non-positive segment, negative offsets, or an element whose counter e / 4 would reach
// the next site's 2^36
static inline int vt_lora_origin_bad(const LoraOrigin& o, long long M, int K) {
    if (o.k0 < 0 || (o.k0 % 8) || o.K_log <= 0 || (o.K_log % 4) || (long long)o.k0 + K > o.K_log) return 1;
    if (o.seg_local <= 0 || o.seg_global < 0 || o.n_first < 0 || o.n_first > o.seg_local || o.off_first < 0 || o.off_rest < 0) return 1;
    if (M <= 0) return 0;
    // the largest logical row: m_g grows with l inside each of a segment's two pieces, so the last row of each piece of the last two segments
    const long long lim = (1LL << 38) / o.K_log;        // rows whose elements all lie below 2^38 (off by < 1 row: checked exactly below)
    const long long bl = (M - 1) / o.seg_local, ll = (M - 1) - bl * o.seg_local;
    if (bl > lim || o.seg_global > lim || o.off_first > lim || o.off_rest > lim || o.seg_local > (1LL << 40)) return 1;
    if (o.seg_global && bl > lim / o.seg_global) return 1;
    long long mg = 0;
    for (int back = 0; back < 2 && bl - back >= 0; ++back) {
        const long long last = back ? o.seg_local - 1 : ll;
        const long long c0 = last < o.n_first ? last : o.n_first - 1;                  // last row of the first piece, if any
        if (c0 >= 0) { const long long v = (bl - back) * o.seg_global + c0 + o.off_first; if (v > mg) mg = v; }
        if (last >= o.n_first) { const long long v = (bl - back) * o.seg_global + last + o.off_rest; if (v > mg) mg = v; }
    }
    return (unsigned __int128)mg * (unsigned)o.K_log + (unsigned)(o.k0 + K - 1) >= ((unsigned __int128)1 << 38);
}
__device__ __forceinline__ LoraDrop lora_drop_arg(const LoraDrop& d, const LoraOrigin&) { return d; }
__device__ __forceinline__ LoraDrop lora_drop_arg(const LoraDrop& d, const LoraOrigin&, const LoraDgelu&) { return d; }
__device__ __forceinline__ LoraDgelu lora_dgelu_arg(const LoraDrop&, const LoraOrigin&) { return LoraDgelu{nullptr, 0}; }
__device__ __forceinline__ LoraDgelu lora_dgelu_arg(const LoraDrop&, const LoraOrigin&, const LoraDgelu& g) { return g; }
__device__ __forceinline__ LoraOrigin lora_origin_arg() { return LoraOrigin{1, 1, 0, 0, 0, 0, 4}; }
__device__ __forceinline__ LoraOrigin lora_origin_arg(const LoraDrop&, const LoraOrigin& o) { return o; }
__device__ __forceinline__ LoraOrigin lora_origin_arg(const LoraDrop&, const LoraOrigin& o, const LoraDgelu&) { return o; }
