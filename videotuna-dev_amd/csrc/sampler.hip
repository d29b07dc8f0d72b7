// Sampler kernels of the CogVideoX workflow (vt355.workflow.CogVideoXWorkFlow.sample):
//   vt_philox_normal   standard-normal noise from Philox4x32-10, the "noise convention" of include/vt355.h
//   vt_dpm_step        classifier-free-guidance combine + one CogVideoXDPMScheduler.step (DPM-Solver++ 2M, v-prediction) in one pass
// Replaces: diffusers' randn_tensor, noise_pred.chunk(2) / the guidance expression and CogVideoXDPMScheduler.step as the reference's
// sampling loop calls them (videotuna/models/cogvideo_hf/cogvideo_pl.py:649-661, 725-746).
#include "common.h"

#define SAMPLER_MAX_BLOCKS 2048          // grid cap of both kernels (256 threads, 4 elements per thread and sweep)

// The four normals of counter ctr under key: Box-Muller on the word pairs (0,1) and (2,3).  u1 = ((w >> 8) + 1) 2^-24 in (0, 1] and
// u2 = (w' >> 8) 2^-24 in [0, 1) are exact in fp32, so a restatement starts from the same two numbers; logf / sincosf are the precise ones.
__device__ __forceinline__ void philox_normal4(unsigned long long ctr, unsigned long long key, float* z) {
    unsigned w[4];
    philox4x32_10((unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u, (unsigned)key, (unsigned)(key >> 32), w);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = (float)((w[2 * p] >> 8) + 1u) * 5.9604644775390625e-8f;
        const float u2 = (float)(w[2 * p + 1] >> 8) * 5.9604644775390625e-8f;
        const float r = sqrtf(-2.0f * logf(u1));
        float s, c;
        sincosf(6.2831855f * u2, &s, &c);
        z[2 * p] = r * c;
        z[2 * p + 1] = r * s;
    }
}
__device__ __forceinline__ unsigned long long noise_counter(int stream_id, long long quad) {
    return ((unsigned long long)stream_id << 40) + (unsigned long long)quad;
}
static inline int noise_args_bad(long long n, int stream_id) {
    // (n - 1) / 4 must stay below 2^40 (the next stream's counters); the stream index must fit the 24 bits above them
    return n > (1ll << 42) || stream_id < 0 || stream_id >= (1 << 24);
}

template <typename T> __device__ __forceinline__ T to_out(float f);
template <> __device__ __forceinline__ float to_out<float>(float f) { return f; }
template <> __device__ __forceinline__ bf16_t to_out<bf16_t>(float f) { return f2bf(f); }

// one thread per counter (4 consecutive elements of one sample); VEC: n % 4 == 0 and an aligned base, one store per thread
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void philox_normal_kernel(T* out, long long n, int B, unsigned long long seed, int stream_id) {
    const long long quads = (n + 3) / 4, total = quads * B;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / quads, q = i - b * quads;
        float z[4];
        philox_normal4(noise_counter(stream_id, q), seed + (unsigned long long)b, z);
        T* o = out + b * n + q * 4;
        if (VEC) {
            if (sizeof(T) == 4) {
                f32x4 v = {z[0], z[1], z[2], z[3]};
                *(f32x4*)o = v;
            } else {
                u32x2 v = {pack2(z[0], z[1]), pack2(z[2], z[3])};
                *(u32x2*)o = v;
            }
        } else {
            const long long left = n - q * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < left) o[j] = to_out<T>(z[j]);
        }
    }
}

extern "C" int vt_philox_normal(void* out, int out_bf16, long long n, int B, unsigned long long seed, int stream_id, void* stream) {
    if (n <= 0 || B <= 0 || noise_args_bad(n, stream_id)) return VT_ERR_BAD_SHAPE;
    const uintptr_t a = (uintptr_t)out;
    if (a % (out_bf16 ? 2 : 4)) return VT_ERR_BAD_ALIGN;
    const bool vec = (n % 4 == 0) && (a % (out_bf16 ? 8 : 16) == 0);
    const long long total = (n + 3) / 4 * B, nb = (total + 255) / 256;
    const dim3 grid((unsigned)(nb > SAMPLER_MAX_BLOCKS ? SAMPLER_MAX_BLOCKS : nb)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (out_bf16) {
        if (vec) hipLaunchKernelGGL((philox_normal_kernel<bf16_t, true>), grid, block, 0, st, (bf16_t*)out, n, B, seed, stream_id);
        else hipLaunchKernelGGL((philox_normal_kernel<bf16_t, false>), grid, block, 0, st, (bf16_t*)out, n, B, seed, stream_id);
    } else {
        if (vec) hipLaunchKernelGGL((philox_normal_kernel<float, true>), grid, block, 0, st, (float*)out, n, B, seed, stream_id);
        else hipLaunchKernelGGL((philox_normal_kernel<float, false>), grid, block, 0, st, (float*)out, n, B, seed, stream_id);
    }
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ---------------- one DPM-Solver++ step with the guidance combine ----------------
struct DpmArgs {
    const bf16_t* v;          // [2B, per] (uncond rows, then cond rows) when guided, else [B, per]
    const bf16_t* x;          // [B, per]
    const float* x0_old;      // [B, per]; read only when second_order
    const float* noise;       // [B, per] | nullptr (drawn in the kernel); read / drawn only when m_noise != 0
    bf16_t* x_out;            // [B, per]
    float* x0_out;            // [B, per]
    long long per;
    int B, guided, second_order, stream_id;
    float g, sa, sb, m1, m2, m3, m4, m_noise;
    unsigned long long seed;
};

// The arithmetic of one element, with every fused multiply-add spelled out: the tensor-fed and the in-kernel noise path, and the
// vector and the scalar path, round alike.
__device__ __forceinline__ void dpm_element(const DpmArgs& a, float vu, float vc, float x, float x0_old, float eps, float& x_new,
                                            float& x0) {
    const float v = a.guided ? fmaf(a.g, vc - vu, vu) : vu;
    x0 = fmaf(-a.sb, v, a.sa * x);
    const float d = a.second_order ? fmaf(-a.m4, x0_old, a.m3 * x0) : x0;
    x_new = fmaf(-a.m2, d, a.m1 * x);
    if (a.m_noise != 0.0f) x_new = fmaf(a.m_noise, eps, x_new);
}

template <bool VEC>
__global__ __launch_bounds__(256) void dpm_step_kernel(DpmArgs a) {
    const long long per = a.per, half = per * a.B;
    const bool noisy = a.m_noise != 0.0f;
    if (VEC) {
        // per % 4 == 0: thread i owns the 4 elements of counter q of sample b; 8-byte bf16 and 16-byte fp32 accesses
        const long long quads = per / 4, total = quads * a.B;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const long long b = i / quads, q = i - b * quads, e = i * 4;
            float vu[4], vc[4], x[4], xo[4] = {0.f, 0.f, 0.f, 0.f}, eps[4] = {0.f, 0.f, 0.f, 0.f};
            const u32x2 pu = *(const u32x2*)(a.v + e), px = *(const u32x2*)(a.x + e);
            u32x2 pc = pu;
            if (a.guided) pc = *(const u32x2*)(a.v + half + e);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                vu[2 * j] = __uint_as_float(pu[j] << 16); vu[2 * j + 1] = __uint_as_float(pu[j] & 0xffff0000u);
                vc[2 * j] = __uint_as_float(pc[j] << 16); vc[2 * j + 1] = __uint_as_float(pc[j] & 0xffff0000u);
                x[2 * j] = __uint_as_float(px[j] << 16); x[2 * j + 1] = __uint_as_float(px[j] & 0xffff0000u);
            }
            if (a.second_order) {
                const f32x4 t = *(const f32x4*)(a.x0_old + e);
                xo[0] = t[0]; xo[1] = t[1]; xo[2] = t[2]; xo[3] = t[3];
            }
            if (noisy) {
                if (a.noise) {
                    const f32x4 t = *(const f32x4*)(a.noise + e);
                    eps[0] = t[0]; eps[1] = t[1]; eps[2] = t[2]; eps[3] = t[3];
                } else {
                    philox_normal4(noise_counter(a.stream_id, q), a.seed + (unsigned long long)b, eps);
                }
            }
            float xn[4], x0[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) dpm_element(a, vu[j], vc[j], x[j], xo[j], eps[j], xn[j], x0[j]);
            const u32x2 po = {pack2(xn[0], xn[1]), pack2(xn[2], xn[3])};
            *(u32x2*)(a.x_out + e) = po;
            const f32x4 fo = {x0[0], x0[1], x0[2], x0[3]};
            *(f32x4*)(a.x0_out + e) = fo;
        }
    } else {
        // any per >= 1, any 2- / 4-byte alignment: one element per thread; an in-kernel draw computes the element's counter and keeps one word
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < half; e += (long long)gridDim.x * 256) {
            const long long b = e / per, k = e - b * per;
            const float vu = bf2f(a.v[e]);
            const float vc = a.guided ? bf2f(a.v[half + e]) : vu;
            const float x = bf2f(a.x[e]);
            const float xo = a.second_order ? a.x0_old[e] : 0.f;
            float eps = 0.f;
            if (noisy) {
                if (a.noise) {
                    eps = a.noise[e];
                } else {
                    float z[4];
                    philox_normal4(noise_counter(a.stream_id, k >> 2), a.seed + (unsigned long long)b, z);
                    const int w = (int)(k & 3);
                    eps = w == 0 ? z[0] : w == 1 ? z[1] : w == 2 ? z[2] : z[3];
                }
            }
            float xn, x0;
            dpm_element(a, vu, vc, x, xo, eps, xn, x0);
            a.x_out[e] = f2bf(xn);
            a.x0_out[e] = x0;
        }
    }
}

extern "C" int vt_dpm_step(const void* v, const void* x, const float* x0_old, const float* noise, void* x_out, float* x0_out,
                           long long per, int B, int guided, float g, float sqrt_ab, float sqrt_1mab, float m1, float m2, float m3,
                           float m4, float m_noise, int second_order, unsigned long long seed, int stream_id, void* stream) {
    if (per <= 0 || B <= 0 || noise_args_bad(per, stream_id) || per > (1ll << 60) / B) return VT_ERR_BAD_SHAPE;
    if (!v || !x || !x_out || !x0_out || (second_order && !x0_old)) return VT_ERR_BAD_SHAPE;
    const uintptr_t av = (uintptr_t)v, ax = (uintptr_t)x, ao = (uintptr_t)x_out, a0 = (uintptr_t)x0_out;
    const uintptr_t aold = second_order ? (uintptr_t)x0_old : 0, an = (m_noise != 0.0f && noise) ? (uintptr_t)noise : 0;
    if ((av | ax | ao) % 2 || (a0 | aold | an) % 4) return VT_ERR_BAD_ALIGN;
    // the cond half of v starts per * B elements in: 8-byte aligned with the base whenever per % 4 == 0
    const bool vec = (per % 4 == 0) && (av | ax | ao) % 8 == 0 && (a0 | aold | an) % 16 == 0;
    DpmArgs a{(const bf16_t*)v, (const bf16_t*)x, second_order ? x0_old : nullptr, m_noise != 0.0f ? noise : nullptr, (bf16_t*)x_out,
              x0_out, per, B, guided ? 1 : 0, second_order ? 1 : 0, stream_id, g, sqrt_ab, sqrt_1mab, m1, m2, m3, m4, m_noise, seed};
    const long long work = vec ? per / 4 * B : per * B, nb = (work + 255) / 256;
    const dim3 grid((unsigned)(nb > SAMPLER_MAX_BLOCKS ? SAMPLER_MAX_BLOCKS : nb)), block(256);
    if (vec) hipLaunchKernelGGL(dpm_step_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(dpm_step_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
