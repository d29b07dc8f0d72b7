// Zero-padded N-d convolution over channels-last activations as an implicit GEMM on the matrix cores (gfx950), forward / input
// gradient and weight gradient: the convolutions of the VideoCrafter2 UNet (BASELINE configs[3]).
//   ResBlock.in_layers[2] / out_layers[3] / Upsample.conv / UNetModel.out[2] ... Conv2d 3x3, padding 1
//       (videotuna/models/lvdm/modules/networks/openaimodel3d.py:166-170, 193, 110-112, 647)
//   Downsample.op ............................................................ Conv2d 3x3, stride 2, padding 1 (:71-79)
//   TemporalConvBlock.conv1..4 ............................................... Conv3d (3,1,1), padding (1,0,0)  (:278-296)
// The reference runs them on NCHW / NCTHW tensors through cuDNN with `(b t) c h w <-> b c t h w` copies in between
// (openaimodel3d.py:249-253); here one channels-last buffer [N, T, H, W, C] serves all of them: a Conv2d is the kernel with
// one temporal tap, the temporal convolution the kernel with one spatial tap.
//
//   y[n,t,ho,wo,co] = bias[co] + sbias[n,co] + res[n,t,ho,wo,co]
//                     + sum_{dt,dh,dw,ci} x[n, t+dt-pt, ho*s+dh-ph, wo*s+dw-pw, ci] * wk[co, (dt,dh,dw), ci]      (zeros outside)
// GEMM view: M = output positions, N = Cout, K = taps * Cin; 128x128x64 tile, LDS-DMA staging (buffer_load ... lds), XOR swizzle
// and MFMA loop of gemm_bf16.hip / conv3d.hip; the row a lane fetches for output position m and a tap is the shifted input
// position or an always-out-of-range offset (zeros).  No im2col buffer.  sbias (fp32 [N, Cout]) is the ResBlock's
// `h + emb_out[..., None, None]` (:245) folded into the convolution that produces h.
// The INPUT gradient of a stride-1 convolution is the same kernel on dY with the flipped, transposed weight (host packs it);
// the WEIGHT gradient is conv_dw_kernel below.
#include "common.h"
#include <stdlib.h>

struct ConvNdParams {
    const bf16_t* x; const bf16_t* w; bf16_t* y;
    const bf16_t* bias;      // [Cout] or null
    const float* sbias;      // fp32 [N, sbias_ld] or null: per-sample bias (sample = m / rows_per_sample)
    const bf16_t* res;       // [M, ldr] or null
    long long ldx, ldy, ldr, x_bytes;
    int sbias_ld, rows_per_sample;
    int M, Cout, Cin, T, H, W, Ho, Wo;
    int KT, KH, KW, pt, ph, pw, stride;
};

#define CN_BM 128
#define CN_BN 128
#define CN_BK 64
#define CN_CS_LD 132
#define CN_OOB 0x80000000u
// 0 = pick per shape, 1 = always the 128 x 128 kernels, 2 = the 320-wide kernels whenever the shape allows (tests, A/B timing)
static int g_conv_tile = 0;
// cap of convnd320_kernel's persistent grid: 0 = the device's CU count, else 1 .. that count (tests: with a small cap a few thousand positions
// make workgroups walk several tiles).  The shape rule itself keeps counting with the device's CUs; the product path never sets it.
static int g_conv_slots = 0;
static int cn_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    }
    return cus;
}
extern "C" int vt_conv_set_tile(int mode) {
    if (mode < 0 || mode > 2) return VT_ERR_BAD_SHAPE;
    g_conv_tile = mode;
    return VT_OK;
}
extern "C" int vt_conv_set_slots(int slots) {
    if (slots < 0 || slots > cn_cus()) return VT_ERR_BAD_SHAPE;
    g_conv_slots = slots;
    return VT_OK;
}
__device__ __forceinline__ int dw3_key(int row) { return (row & 7) ^ (((row >> 3) & 1) << 2); }
static __device__ __forceinline__ void dw3_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ __launch_bounds__(256, 2) void convnd_cl_kernel(ConvNdParams p) {
    __shared__ __attribute__((aligned(16))) char smem[65536];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int nbm = (p.M + CN_BM - 1) / CN_BM, nbn = (p.Cout + CN_BN - 1) / CN_BN;
    const int id = xcd_remap(blockIdx.x, nbm * nbn);
    const int tile_m = id / nbn, tile_n = id % nbn;
    const int row0 = tile_m * CN_BM, col0 = tile_n * CN_BN;
    const int HWo = p.Ho * p.Wo;
    const int ldw = p.KT * p.KH * p.KW * p.Cin;

    __amdgpu_buffer_rsrc_t ra = make_rsrc(p.x, (unsigned)p.x_bytes);
    const long long w_rem = (long long)(p.Cout - col0) * ldw * 2;
    __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w + (size_t)col0 * ldw, (unsigned)(w_rem > 0x7fffffffLL ? 0x7fffffffLL : w_rem));

    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int drl = lane >> 3, dcp = lane & 7;
    const int chunk_off = (dcp ^ drl) << 4;
    int w_voff[4];
    int rt[4], rh[4], rw_[4], rn[4];     // (t, ho, wo, n) of this lane's four output rows; rt < 0: row beyond M
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 8 * (wv + 4 * j) + drl;
        w_voff[j] = row * ldw * 2 + chunk_off;
        const int m = row0 + row;
        if (m < p.M) {
            const int sp = m % HWo;
            const int nt = m / HWo;
            rt[j] = nt % p.T; rn[j] = nt / p.T;
            rh[j] = sp / p.Wo;
            rw_[j] = sp - rh[j] * p.Wo;
        } else {
            rt[j] = -1; rh[j] = 0; rw_[j] = 0; rn[j] = 0;
        }
    }
    const int kpt = p.Cin / CN_BK;
    const int ntaps = p.KT * p.KH * p.KW;
    unsigned a_voff[4];
    auto set_tap = [&](int tap) {
        const int dw = tap % p.KW, dh = (tap / p.KW) % p.KH, dt = tap / (p.KW * p.KH);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int tt = rt[j] + dt - p.pt;
            const int hh = rh[j] * p.stride + dh - p.ph, ww = rw_[j] * p.stride + dw - p.pw;
            const bool ok = rt[j] >= 0 && tt >= 0 && tt < p.T && hh >= 0 && hh < p.H && ww >= 0 && ww < p.W;
            const long long r = (((long long)rn[j] * p.T + tt) * p.H + hh) * p.W + ww;
            a_voff[j] = ok ? (unsigned)(r * p.ldx * 2 + chunk_off) : CN_OOB;
        }
    };
    int d_tap = 0, d_kc = 0;
    auto dma = [&](int buf) {
        if (d_kc == 0) set_tap(d_tap);
        const int a_soff = d_kc * CN_BK * 2;
        const int w_soff = (d_tap * p.Cin + d_kc * CN_BK) * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            char* dst = smem + buf * 32768 + (wv + 4 * j) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)dst, 16, (int)a_voff[j], a_soff, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(dst + 16384), 16, w_voff[j], w_soff, 0, 0);
        }
        if (++d_kc == kpt) { d_kc = 0; ++d_tap; }
    };

    f32x4 acc[4][4];   // [tn][tm]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = ntaps * kpt;
    dma(0);
    __syncthreads();
    const int frow = lane & 15, fq = lane >> 4, fx = lane & 7;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) dma(buf ^ 1);
        const char* As = smem + buf * 32768;
        const char* Ws = As + 16384;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int coff = (((ks * 4 + fq) ^ fx) << 4);
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = *(const bf16x8*)(As + (wm * 64 + t * 16 + frow) * 128 + coff);
                wf[t] = *(const bf16x8*)(Ws + (wn * 64 + t * 16 + frow) * 128 + coff);
            }
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm)
                    acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tn], af[tm], acc[tn][tm], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---------------- epilogue: two 64-row halves through LDS; bias + per-sample bias + residual; bf16 store ----------------
    float* Cs = (float*)smem;
    const int er = tid >> 5, ec = (tid & 31) * 4;
    const int n = col0 + ec;
    float bias4[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias != nullptr && n < p.Cout) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bias4[j] = bf2f(p.bias[n + j]);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (wm == half) {
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm)
                    *(f32x4*)(Cs + (tm * 16 + frow) * CN_CS_LD + wn * 64 + tn * 16 + fq * 4) = acc[tn][tm];
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 8; ++pass) {
            const int ml = pass * 8 + er;
            const int m = row0 + half * 64 + ml;
            if (m < p.M && n < p.Cout) {
                f32x4 v = *(const f32x4*)(Cs + ml * CN_CS_LD + ec);
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = v[j] + bias4[j];
                if (p.sbias != nullptr) {
                    const f32x4 sb = *(const f32x4*)(p.sbias + (size_t)(m / p.rows_per_sample) * p.sbias_ld + n);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] += sb[j];
                }
                if (p.res != nullptr) {
                    const u32x2 r2 = *(const u32x2*)(p.res + (size_t)m * p.ldr + n);
                    o[0] += __uint_as_float(r2[0] << 16); o[1] += __uint_as_float(r2[0] & 0xffff0000u);
                    o[2] += __uint_as_float(r2[1] << 16); o[3] += __uint_as_float(r2[1] & 0xffff0000u);
                }
                u32x2 c2;
                c2[0] = pack2(o[0], o[1]);
                c2[1] = pack2(o[2], o[3]);
                *(u32x2*)(p.y + (size_t)m * p.ldy + n) = c2;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Forward / input gradient, 128 x 320 tile (r03): Cout % 320 == 0 and enough tiles to fill the chip (the UNet's two outer levels).
// convnd_cl_kernel keeps ONE 32 KiB K-tile in flight per workgroup and re-gathers the x rows for each of the three 128-column tiles of a
// 320-wide output (the third one 5/8 empty): at 163 840 positions it runs at ~650 TFLOP/s, bound by the latency of its own loads.  Same
// cure as conv_dw320_kernel: all of a 320-channel block per workgroup (x gathered once), K-tiles of 32 channels of one tap = 64-byte rows,
// a ring of five 28 KiB stages [128 x rows | 320 weight rows] filled by four LOADER waves (7 buffer_load ... lds each per K-tile, counted
// vmcnt), eight MULTIPLIER waves (2 x 4: 64 positions x 80 channels = 4 x 5 MFMA 16x16x32 tiles, fragments by ds_read_b128).
// 64-byte rows: physical 16-byte chunk = logical ^ key(row), key = (-(row >> 2)) & 3 -- the 16 lanes ds_read_b128 serves together
// ({0-3, 12-15, 20-27}, ...) are rows 0-3 / 12-15 of one k-chunk and rows 4-11 of the next: this key spreads them over all 64 banks.
#define CN3_NS 5
#define CN3_STAGE 28672
__device__ __forceinline__ int cn3_key(int row) { return (-(row >> 2)) & 3; }

__global__ __launch_bounds__(768, 1) void convnd320_kernel(ConvNdParams p) {
    __shared__ __attribute__((aligned(16))) char smem[CN3_NS * CN3_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbm = (p.M + 127) / 128, nbn = p.Cout / 320;
    const int ntiles = nbm * nbn;
    // PERSISTENT: workgroup `slot` walks tiles slot, slot + gridDim.x, ...; the loaders run ahead across tile boundaries, so the ring is
    // already refilled while the multipliers write a tile out (a K loop is only 30 .. 180 K-tiles long here: with one workgroup per CU
    // and an epilogue behind a drained ring, the first version gained 4 % over the 128 x 128 kernel)
    const int slot = xcd_remap(blockIdx.x, gridDim.x);
    if (slot >= ntiles) return;
    const int my_tiles = (ntiles - slot + (int)gridDim.x - 1) / (int)gridDim.x;
    const int ldw = p.KT * p.KH * p.KW * p.Cin;
    const int kpt = p.Cin / 32;                                   // K-tiles per tap
    const int ntaps = p.KT * p.KH * p.KW;
    const int nk = ntaps * kpt;
    const int total = my_tiles * nk;

    if (wave >= 8) {
        // =================================== loader waves ===================================
        const int lw = wave - 8;
        const int r16 = lane >> 2;
        const int lc = (lane & 3) ^ cn3_key(r16);                  // logical 16-byte chunk (8 channels of the K-tile's 32)
        __amdgpu_buffer_rsrc_t ra = make_rsrc(p.x, (unsigned)p.x_bytes);
        const int HWo = p.Ho * p.Wo;
        int rt[2], rh[2], rw_[2], rn[2];
        int w_voff[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) w_voff[j] = (16 * (lw + 4 * j) + r16) * ldw * 2 + lc * 16;
        int tile = slot;
        const bf16_t* wbase = p.w;
        unsigned w_bytes = 0;
        auto set_tile = [&]() {
            const int row0 = (tile / nbn) * 128, col0 = (tile % nbn) * 320;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int m = row0 + 16 * (lw + 4 * j) + r16;
                if (m < p.M) {
                    const int sp = m % HWo, nt = m / HWo;
                    rt[j] = nt % p.T; rn[j] = nt / p.T;
                    rh[j] = sp / p.Wo; rw_[j] = sp - rh[j] * p.Wo;
                } else {
                    rt[j] = -1; rh[j] = 0; rw_[j] = 0; rn[j] = 0;
                }
            }
            const long long w_rem = (long long)(p.Cout - col0) * ldw * 2;
            wbase = p.w + (size_t)col0 * ldw;
            w_bytes = (unsigned)(w_rem > 0x7fffffffLL ? 0x7fffffffLL : w_rem);
        };
        unsigned a_voff[2] = {CN_OOB, CN_OOB};
        auto set_tap = [&](int tap) {
            const int dw = tap % p.KW, dh = (tap / p.KW) % p.KH, dt = tap / (p.KW * p.KH);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int tt = rt[j] + dt - p.pt;
                const int hh = rh[j] * p.stride + dh - p.ph, ww = rw_[j] * p.stride + dw - p.pw;
                const bool ok = rt[j] >= 0 && tt >= 0 && tt < p.T && hh >= 0 && hh < p.H && ww >= 0 && ww < p.W;
                const long long r = (((long long)rn[j] * p.T + tt) * p.H + hh) * p.W + ww;
                a_voff[j] = ok ? (unsigned)(r * p.ldx * 2 + lc * 16) : CN_OOB;
            }
        };
        int d_tap = 0, d_kc = 0;
        set_tile();
        auto issue = [&](int g) {                                  // K-tile g of this workgroup's stream -> stage g % NS
            if (d_kc == 0) set_tap(d_tap);
            __amdgpu_buffer_rsrc_t rw = make_rsrc(wbase, w_bytes);
            char* st = smem + (g % CN3_NS) * CN3_STAGE + lw * 1024;
            const int a_soff = d_kc * 64;
            const int w_soff = (d_tap * p.Cin + d_kc * 32) * 2;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                unsigned off = a_voff[j];
                asm volatile("" : "+v"(off));                      // one load per piece under the full EXEC mask (the vmcnt ladder counts 7 per K-tile)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)(st + j * 4096), 16, (int)off, a_soff, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 5; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(st + 8192 + j * 4096), 16, w_voff[j], w_soff, 0, 0);
            if (++d_kc == kpt) {
                d_kc = 0;
                if (++d_tap == ntaps) {                            // the next K-tile opens the workgroup's next output tile
                    d_tap = 0;
                    tile += gridDim.x;
                    if (tile < ntiles) set_tile();
                }
            }
        };
        int issued = 0;
        for (; issued < CN3_NS - 1 && issued < total; ++issued) issue(issued);
        for (int g = 0; g < total; ++g) {
            const int younger = issued - g - 1;
            if (younger >= 3) asm volatile("s_waitcnt vmcnt(21)" ::: "memory");
            else if (younger == 2) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
            else if (younger == 1) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            dw3_barrier();                                         // (A) stage g % NS is ready / stage (g-1) % NS has been consumed
            if (issued < total) { issue(issued); ++issued; }
        }
        return;
    }

    // =================================== multiplier waves ===================================
    const int wm = wave & 1, wn = wave >> 1;                       // 2 x 4 waves: positions 64 wm .., channels 80 wn ..
    const int frow = lane & 15, fq = lane >> 4;
    const int rd_off = frow * 64 + ((fq ^ cn3_key(frow)) << 4);
    int g = 0;
    for (int tile = slot; tile < ntiles; tile += gridDim.x) {
        const int row0 = (tile / nbn) * 128, col0 = (tile % nbn) * 320;
        f32x4 acc[5][4];   // [tn][tm]: D[n][m], the lane holds position m = lane & 15 and the four consecutive channels n = 4 (lane >> 4) + r
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < nk; ++kt, ++g) {
            dw3_barrier();                                         // (A)
            const char* As = smem + (g % CN3_NS) * CN3_STAGE + (wm * 64) * 64 + rd_off;
            const char* Ws = smem + (g % CN3_NS) * CN3_STAGE + 8192 + (wn * 80) * 64 + rd_off;
            bf16x8 af[4], wf[5];
#pragma unroll
            for (int t = 0; t < 4; ++t) af[t] = *(const bf16x8*)(As + t * 1024);
#pragma unroll
            for (int t = 0; t < 5; ++t) wf[t] = *(const bf16x8*)(Ws + t * 1024);
#pragma unroll
            for (int tn = 0; tn < 5; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm)
                    acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tn], af[tm], acc[tn][tm], 0, 0, 0);
        }
        // ---- epilogue straight from the registers (no LDS, no barrier: the loaders are already filling the ring for the next tile): a lane
        // owns four consecutive channels of a position = one 8-byte store; the five channel tiles of a wave make 160 contiguous bytes per row
#pragma unroll
        for (int tn = 0; tn < 5; ++tn) {
            const int n = col0 + wn * 80 + tn * 16 + fq * 4;
            float b4[4] = {0.f, 0.f, 0.f, 0.f};
            if (p.bias != nullptr) {
#pragma unroll
                for (int j = 0; j < 4; ++j) b4[j] = bf2f(p.bias[n + j]);          // a parameter view: only 2-byte aligned
            }
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) {
                const int m = row0 + wm * 64 + tm * 16 + frow;
                if (m < p.M) {
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = acc[tn][tm][j] + b4[j];
                    if (p.sbias != nullptr) {
                        const f32x4 sb = *(const f32x4*)(p.sbias + (size_t)(m / p.rows_per_sample) * p.sbias_ld + n);
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[j] += sb[j];
                    }
                    if (p.res != nullptr) {
                        const u32x2 r2 = *(const u32x2*)(p.res + (size_t)m * p.ldr + n);
                        o[0] += __uint_as_float(r2[0] << 16); o[1] += __uint_as_float(r2[0] & 0xffff0000u);
                        o[2] += __uint_as_float(r2[1] << 16); o[3] += __uint_as_float(r2[1] & 0xffff0000u);
                    }
                    u32x2 c2;
                    c2[0] = pack2(o[0], o[1]);
                    c2[1] = pack2(o[2], o[3]);
                    *(u32x2*)(p.y + (size_t)m * p.ldy + n) = c2;
                }
            }
        }
    }
}

// Byte extent of a buffer descriptor over `rows` rows of stride `ld` elements of which the first `cols` are read: it ends with the LAST row's
// logical columns, not at rows * ld -- an operand may be a column slice of a wider buffer (one half of a skip concatenation, or its gradient)
// whose base is not the allocation's base, and rows * ld counted from there runs past the end of the allocation.
static long long cn_extent_bytes(long long rows, long long ld, long long cols) { return ((rows - 1) * ld + cols) * 2; }

// Test hook (tests/test_unet_kernels_gpu.py): the byte extents vt_conv_cl / vt_conv_dw_cl put into their descriptors for this geometry, so a
// test can assert extent <= bytes between the slice's base and the end of its allocation BEFORE launching anything.
extern "C" int vt_conv_desc_extents(long long ldx, long long lddy, int N, int T, int H, int W, int Cin, int Cout, int KH, int KW, int ph, int pw,
                                    int stride, long long* fwd_x_bytes, long long* dw_x_bytes, long long* dw_dy_bytes) {
    if (N <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH < 1 || KW < 1 || stride < 1) return VT_ERR_BAD_SHAPE;
    const int Ho = (H + 2 * ph - KH) / stride + 1, Wo = (W + 2 * pw - KW) / stride + 1;
    if (Ho <= 0 || Wo <= 0) return VT_ERR_BAD_SHAPE;
    const long long rows_in = (long long)N * T * H * W, rows_out = (long long)N * T * Ho * Wo;
    if (fwd_x_bytes) *fwd_x_bytes = cn_extent_bytes(rows_in, ldx, Cin);
    if (dw_x_bytes) *dw_x_bytes = cn_extent_bytes(rows_in, ldx, (Cin + 7) / 8 * 8);
    if (dw_dy_bytes) *dw_dy_bytes = cn_extent_bytes(rows_out, lddy, (Cout + 7) / 8 * 8);
    return VT_OK;
}

// What vt_conv_cl does with a geometry: the plan vt_conv_plan reports and vt_conv_cl follows.
struct ConvNdPlan {
    int kernel;            // 1 = convnd_cl_kernel (128 x 128 tiles, one per workgroup), 2 = convnd320_kernel (128 x 320 tiles, persistent)
    int grid;              // workgroups
    int tiles;             // output tiles of that kernel
    int tiles_per_wg;      // the most tiles one workgroup walks
    int Ho, Wo;
    long long rows_out, x_bytes;
};
static int cn_plan(long long ldx, long long ldy, int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw,
                   int stride, ConvNdPlan* pl) {
    if (N <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin % CN_BK) || (Cout % 4)) return VT_ERR_BAD_SHAPE;
    if (KT < 1 || KH < 1 || KW < 1 || stride < 1 || pt < 0 || ph < 0 || pw < 0 || 2 * pt != KT - 1) return VT_ERR_BAD_SHAPE;   // no temporal stride / shrink
    const int Ho = (H + 2 * ph - KH) / stride + 1, Wo = (W + 2 * pw - KW) / stride + 1;
    if (Ho <= 0 || Wo <= 0) return VT_ERR_BAD_SHAPE;
    if ((ldx % 8) || (ldy % 4) || ldx < Cin || ldy < Cout) return VT_ERR_BAD_SHAPE;
    const long long rows_in = (long long)N * T * H * W, rows_out = (long long)N * T * Ho * Wo;
    const long long xb = cn_extent_bytes(rows_in, ldx, Cin);    // ends with the last row's Cin columns (x may be a column slice of a wider buffer)
    if (xb >= 0x7fffffffLL || rows_out >= 0x7fffffffLL || (long long)KT * KH * KW * Cin * 2 * CN_BN >= 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
    pl->Ho = Ho; pl->Wo = Wo; pl->rows_out = rows_out; pl->x_bytes = xb;
    const int nbm = (int)((rows_out + CN_BM - 1) / CN_BM), nbn = (Cout + CN_BN - 1) / CN_BN;
    static int cn3_env = -1;                 // VT355_CONV320=0: always the 128 x 128 kernel (A/B)
    if (cn3_env < 0) { const char* e = getenv("VT355_CONV320"); cn3_env = e ? atoi(e) : 1; }
    // Cout = 320 (and 960): 2.5 (7.5) tiles of 128 -- there the 128 x 320 kernel wins 15 .. 25 % (profiles/r03_conv_kbench.txt); at 640 / 1280 the
    // 128 x 128 kernel has no ragged tile, runs two workgroups per CU and is 4 .. 25 % faster
    if (cn3_env && g_conv_tile != 1 && (Cout % 320) == 0 && ((Cout % 128) != 0 || g_conv_tile == 2)) {
        const int cus3 = cn_cus();
        // one workgroup per CU and pass (140 KiB of LDS): only when whole passes are >= 80 % full
        const long long t3 = (long long)nbm * (Cout / 320), passes = (t3 + cus3 - 1) / cus3;
        if (g_conv_tile == 2 || (t3 >= cus3 && (double)t3 >= 0.8 * (double)(passes * cus3))) {
            const int cap = g_conv_slots ? g_conv_slots : cus3;
            pl->kernel = 2; pl->tiles = (int)t3; pl->grid = (int)(t3 < cap ? t3 : cap);
            pl->tiles_per_wg = (int)((t3 + pl->grid - 1) / pl->grid);
            return VT_OK;
        }
    }
    pl->kernel = 1; pl->tiles = pl->grid = nbm * nbn; pl->tiles_per_wg = 1;
    return VT_OK;
}

// host-only query (tests): kernel, grid, tiles and the most tiles per workgroup of the launch vt_conv_cl would make for this geometry under the
// current vt_conv_set_tile / vt_conv_set_slots setting.  Each output pointer may be NULL.
extern "C" int vt_conv_plan(long long ldx, long long ldy, int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw,
                            int stride, int* kernel, int* grid, int* tiles, int* tiles_per_wg) {
    ConvNdPlan pl;
    const int rc = cn_plan(ldx, ldy, N, T, H, W, Cin, Cout, KT, KH, KW, pt, ph, pw, stride, &pl);
    if (rc != VT_OK) return rc;
    if (kernel) *kernel = pl.kernel;
    if (grid) *grid = pl.grid;
    if (tiles) *tiles = pl.tiles;
    if (tiles_per_wg) *tiles_per_wg = pl.tiles_per_wg;
    return VT_OK;
}

// x: bf16 [N,T,H,W,Cin] (position stride ldx), wk: bf16 [Cout, KT*KH*KW*Cin] tap-major (dt,dh,dw,ci); y: bf16
// [N,T,Ho,Wo,Cout] with Ho = (H + 2 ph - KH) / stride + 1 (same for W); bias bf16 [Cout] | null; sbias fp32 [N, sbias_ld] | null;
// res bf16 like y | null.  Cin % 64 == 0, Cout % 4 == 0, the whole x must span < 2 GiB.
extern "C" int vt_conv_cl(const void* x, long long ldx, const void* wk, const void* bias, const float* sbias, int sbias_ld,
                          const void* res, long long ldr, void* y, long long ldy,
                          int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw, int stride,
                          void* stream) {
    ConvNdPlan pl;
    const int rc = cn_plan(ldx, ldy, N, T, H, W, Cin, Cout, KT, KH, KW, pt, ph, pw, stride, &pl);
    if (rc != VT_OK) return rc;
    if (res != nullptr && ((ldr % 4) || ldr < Cout)) return VT_ERR_BAD_SHAPE;
    if (sbias != nullptr && ((sbias_ld % 4) || sbias_ld < Cout)) return VT_ERR_BAD_SHAPE;
    if ((((uintptr_t)x) | ((uintptr_t)wk) | ((uintptr_t)y) | ((uintptr_t)res) | ((uintptr_t)sbias)) & 15) return VT_ERR_BAD_ALIGN;
    const int Ho = pl.Ho, Wo = pl.Wo;
    ConvNdParams p;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)wk; p.y = (bf16_t*)y; p.bias = (const bf16_t*)bias; p.sbias = sbias;
    p.res = (const bf16_t*)res; p.ldx = ldx; p.ldy = ldy; p.ldr = ldr; p.x_bytes = pl.x_bytes; p.sbias_ld = sbias_ld;
    p.rows_per_sample = T * Ho * Wo;
    p.M = (int)pl.rows_out; p.Cout = Cout; p.Cin = Cin; p.T = T; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo;
    p.KT = KT; p.KH = KH; p.KW = KW; p.pt = pt; p.ph = ph; p.pw = pw; p.stride = stride;
    if (pl.kernel == 2) hipLaunchKernelGGL(convnd320_kernel, dim3((unsigned)pl.grid), dim3(768), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(convnd_cl_kernel, dim3((unsigned)pl.grid), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Weight gradient:  dW[co, tap, ci] (+)= sum_m dY[m, co] * x[shift(m, tap), ci]      (fp32, laid out like wk: [Cout, taps*Cin])
// The reduction runs over the output positions m -- the slow index of both operands -- so, as in gemm_nt_bf16.hip, tiles are staged
// row-major ([64 positions][128 channels], LDS-DMA, source-side swizzle) and both MFMA fragments come from transposed LDS reads
// (ds_read_b64_tr_b16); the x rows of a K-tile are GATHERED: row m of the tile is the input position that the lane's tap pairs
// with output position m, or zeros.  P = Cout and Q = taps * Cin need not be tile multiples: the columns past them hold whatever lies
// next in memory (or zeros), feed only accumulators that are never stored.  The position axis is split over blockIdx.y (fp32 atomics) until the
// grid fills the chip.  With one tap and no shift this is also the weight gradient of an nn.Linear whose dimensions are not
// multiples of 128 (C = 320).
struct ConvDwParams {
    const bf16_t* dy; const bf16_t* x; float* dw;
    float* dbias;            // conv_dw320_kernel: += column sums of dy (the bias gradient), or null
    long long lddy, ldx, dy_bytes, x_bytes;
    int M, Cout, Cin, T, H, W, Ho, Wo, KT, KH, KW, pt, ph, pw, stride;
    int m_chunk, splits, accumulate;
    // exact division of a 31-bit row index by Ho*Wo, Wo and T as multiply + shift (Granlund-Montgomery): the gather decodes four rows per
    // lane and K-tile, and hardware integer division (~40 VALU instructions each, 6 per row) cost more than the K-tile's MFMAs
    unsigned long long mg_hwo, mg_wo, mg_t;
    int sh_hwo, sh_wo, sh_t;
};
__device__ __forceinline__ int cn_fastdiv(int n, unsigned long long magic, int shift) { return (int)(((unsigned long long)(unsigned)n * magic) >> shift); }
static void cn_magic(int d, unsigned long long* magic, int* shift) {
    int l = 0;
    while ((1LL << l) < d) ++l;
    *shift = 31 + l;
    *magic = ((1ULL << *shift) + (unsigned long long)d - 1) / (unsigned long long)d;
}
typedef __attribute__((ext_vector_type(8))) short short8cn;
__device__ __forceinline__ int cn_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ bf16x8 cn_tr_pair(const char* p0, const char* p1) {
    short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(p0));
    short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(p1));
    short8cn v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v8);
}

__global__ __launch_bounds__(256, 2) void conv_dw_kernel(ConvDwParams p) {
    __shared__ __attribute__((aligned(16))) char smem[65536];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave & 1, wq = wave >> 1;
    const int ntaps = p.KT * p.KH * p.KW;
    const int QF = ntaps * p.Cin;                    // the (tap, ci) axis flattened: a 128-column tile may straddle taps -- every lane
                                                     // fetches ONE 8-channel chunk of one tap, so the gather is per lane anyway -- and only
                                                     // the very last tile of the axis is ragged (Cin = 320: 23 tiles instead of 9 x 3)
    const int nbp = (p.Cout + 127) / 128, nbq = (QF + 127) / 128;
    const int id = xcd_remap(blockIdx.x, nbp * nbq);
    const int tile_p = id % nbp, tile_q = id / nbp;
    const int p0 = tile_p * 128, q0 = tile_q * 128;
    const int HWo = p.Ho * p.Wo;

    const int m_lo = (int)blockIdx.y * p.m_chunk;
    const int m_cnt = min(p.M - m_lo, p.m_chunk);
    if (m_cnt <= 0) return;
    __amdgpu_buffer_rsrc_t ra = make_rsrc(p.dy, (unsigned)p.dy_bytes);
    __amdgpu_buffer_rsrc_t rb = make_rsrc(p.x, (unsigned)p.x_bytes);

    // lane l lands at (row l>>4 of its 4-row block, physical chunk l&15) and fetches logical chunk (l&15) ^ swz(row): its column, hence
    // its tap and input-channel offset, are fixed for the whole kernel (per j: the row inside the K-tile changes the swizzle)
    const int drl = lane >> 4, dcp = lane & 15;
    int a_col[4], b_ci[4], b_dt[4], b_dh[4], b_dw[4], b_roff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 4 * (wave + 4 * j) + drl;
        const int ch = dcp ^ cn_swz(row);
        a_col[j] = (p0 + ch * 8) * 2;
        const int qc = q0 + ch * 8;
        if (qc < QF) {
            const int tap = qc / p.Cin;
            b_ci[j] = (qc - tap * p.Cin) * 2;
            b_dw[j] = tap % p.KW - p.pw; b_dh[j] = (tap / p.KW) % p.KH - p.ph; b_dt[j] = tap / (p.KW * p.KH) - p.pt;
        } else {
            b_ci[j] = -1; b_dw[j] = 0; b_dh[j] = 0; b_dt[j] = 0;
        }
        b_roff[j] = (b_dt[j] * p.H + b_dh[j]) * p.W + b_dw[j];
    }
    // The position decode of a K-tile's 64 rows (three divisions each) is done ONCE, by the first wave, two K-tiles ahead, into a
    // small LDS table: {row index of the centre tap, t, h*stride, w*stride}; every lane then only adds its tap's
    // constants and tests the bounds (r02: the per-lane decode of four rows cost as much issue time as the K-tile's MFMAs).
    __shared__ int4 rowtab[2][64];
    auto fill = [&](int kt) {
        if (tid < 64) {
            const int ml = kt * 64 + tid;
            int4 e = {0, 0x40000000, 0, 0};                     // t far out of range for every tap
            if (ml < m_cnt) {
                const int m = m_lo + ml;
                const int nt = cn_fastdiv(m, p.mg_hwo, p.sh_hwo), sp = m - nt * HWo;
                const int n = cn_fastdiv(nt, p.mg_t, p.sh_t), t = nt - n * p.T;
                const int ho = cn_fastdiv(sp, p.mg_wo, p.sh_wo), wo = sp - ho * p.Wo;
                e.x = ((n * p.T + t) * p.H + ho * p.stride) * p.W + wo * p.stride;
                e.y = t; e.z = ho * p.stride; e.w = wo * p.stride;
            }
            rowtab[kt & 1][tid] = e;
        }
    };
    const unsigned ldx2 = (unsigned)(p.ldx * 2);
    auto dma = [&](int kt, int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 4 * (wave + 4 * j) + drl;
            const int ml = kt * 64 + row;
            const int4 e = rowtab[kt & 1][row];
            unsigned a_off = CN_OOB, b_off = CN_OOB;
            if (ml < m_cnt) a_off = (unsigned)((long long)(m_lo + ml) * p.lddy * 2 + a_col[j]);
            const int tt = e.y + b_dt[j], hh = e.z + b_dh[j], ww = e.w + b_dw[j];
            if (b_ci[j] >= 0 && (unsigned)tt < (unsigned)p.T && (unsigned)hh < (unsigned)p.H && (unsigned)ww < (unsigned)p.W)
                b_off = (unsigned)(e.x + b_roff[j]) * ldx2 + (unsigned)b_ci[j];
            char* dst = smem + buf * 32768 + (wave + 4 * j) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)dst, 16, (int)a_off, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (__attribute__((address_space(3))) void*)(dst + 16384), 16, (int)b_off, 0, 0, 0);
        }
    };
    const int g = lane >> 4, ql = (lane & 15) >> 2, pl = lane & 3;
    auto tr_addr = [&](const char* img, int slab_col0, int ks, int sec, int t) {
        const int row = ks * 32 + 8 * g + ql + 4 * sec;
        const int col = slab_col0 + t * 16 + 4 * pl;
        return img + row * 256 + (((col >> 3) ^ cn_swz(row)) << 4) + (col & 7) * 2;
    };
    f32x4 acc[4][4];     // [tp][tq]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nk = (m_cnt + 63) / 64;
    fill(0); fill(1);
    __syncthreads();
    dma(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) dma(kt + 1, buf ^ 1);
        if (kt + 2 < nk) fill(kt + 2);                   // slot kt & 1: read by dma(kt, .) one iteration ago, behind a barrier
        const char* As = smem + buf * 32768;
        const char* Bs = As + 16384;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[4], bfr[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = cn_tr_pair(tr_addr(As, wp * 64, ks, 0, t), tr_addr(As, wp * 64, ks, 1, t));
                bfr[t] = cn_tr_pair(tr_addr(Bs, wq * 64, ks, 0, t), tr_addr(Bs, wq * 64, ks, 1, t));
            }
#pragma unroll
            for (int tp = 0; tp < 4; ++tp)
#pragma unroll
                for (int tq = 0; tq < 4; ++tq)
                    acc[tp][tq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[tp], bfr[tq], acc[tp][tq], 0, 0, 0);
        }
        __syncthreads();
    }
    const int fr = lane & 15;
#pragma unroll
    for (int tp = 0; tp < 4; ++tp)
#pragma unroll
        for (int tq = 0; tq < 4; ++tq)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int pr = p0 + wp * 64 + tp * 16 + 4 * g + rg;
                const int qc = q0 + wq * 64 + tq * 16 + fr;
                if (pr < p.Cout && qc < QF) {
                    float* c = p.dw + (size_t)pr * QF + qc;
                    const float v = acc[tp][tq][rg];
                    if (p.splits > 1 || p.accumulate) atomicAdd(c, v);
                    else *c = v;
                }
            }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Weight gradient, 320-row tile (r03): Cout % 320 == 0 -- every channel count of the VideoCrafter2 UNet (320 / 640 / 1280).
// Why: conv_dw_kernel's 128 x 128 tile reads 32 KiB of operands per 2.1 MFLOP (64 flop/B) with ONE K-tile in flight per workgroup: at the
// UNet's first level (163 840 positions, P = 320 of 384 tile rows used) it moved 5.8 TB/s of L2 / fabric reads for 296 useful TFLOP/s, and
// its LDS (fragment reads + DMA writes, 1500 cycles per 1024 MFMA cycles) was busier than its matrix pipe.  Here:
//   tile 320 (all of a Cout block, no ragged third tile) x 128 columns of the (tap, ci) axis: 91 flop/B;
//   K-tile = 32 positions, a ring of DW3_NS = 5 stages of 28 KiB = [5 dY slabs | 2 x slabs] x [32 rows][128 B], four K-tiles in flight;
//   four LOADER waves (one 8-row block each: they decode their row's position once per K-tile, then 5 + 2 buffer_load ... lds) and eight
//   MULTIPLIER waves (4 x 2: 80 x 64 outputs each = 5 x 4 MFMA 16x16x32 tiles, fragments by ds_read_b64_tr_b16), as gemm_pc_bf16.hip:
//   counted vmcnt in the loaders only, one raw barrier per K-tile;
//   swizzle key(row) = (row & 7) ^ (((row >> 3) & 1) << 2) on the 16-byte chunk index: the two 16-lane groups of a half-wave read rows r..r+3
//   and r+8..r+11 -- with the plain (row & 7) key they meet on the same banks.
// One-dimensional grid of tiles x splits workgroups; the xcd remap keeps the q-tiles of one position range (same dY rows, overlapping x
// rows) on one XCD's L2.
#define DW3_NS 5
#define DW3_STAGE 28672
#define DW3_P 320
#define DW3_Q 128

__global__ __launch_bounds__(768, 1) void conv_dw320_kernel(ConvDwParams p) {
    __shared__ __attribute__((aligned(16))) char smem[DW3_NS * DW3_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntaps = p.KT * p.KH * p.KW;
    const int QF = ntaps * p.Cin;
    const int nbp = p.Cout / DW3_P, nbq = (QF + DW3_Q - 1) / DW3_Q;
    const int tiles = nbp * nbq;
    const int lin = xcd_remap(blockIdx.x, tiles * p.splits);
    const int split = lin / tiles, tile = lin - split * tiles;
    const int tile_p = tile % nbp, tile_q = tile / nbp;
    const int p0 = tile_p * DW3_P, q0 = tile_q * DW3_Q;
    const int m_lo = split * p.m_chunk;
    const int m_cnt = min(p.M - m_lo, p.m_chunk);
    if (m_cnt <= 0) return;
    const int nk = (m_cnt + 31) / 32;

    if (wave >= 8) {
        // =================================== loader waves ===================================
        const int lw = wave - 8;                                   // rows 8 lw .. 8 lw + 7 of every K-tile
        const int rloc = 8 * lw + (lane >> 3);
        const int lc = (lane & 7) ^ dw3_key(rloc);                 // the logical 16-byte chunk this lane fetches (of every slab)
        __amdgpu_buffer_rsrc_t ra = make_rsrc(p.dy, (unsigned)p.dy_bytes);
        __amdgpu_buffer_rsrc_t rb = make_rsrc(p.x, (unsigned)p.x_bytes);
        const int HWo = p.Ho * p.Wo;
        const unsigned lddy2 = (unsigned)(p.lddy * 2), ldx2 = (unsigned)(p.ldx * 2);
        const unsigned a_col = (unsigned)((p0 + lc * 8) * 2);      // + slab * 128 bytes
        int b_ci[2], b_dt[2], b_dh[2], b_dw[2], b_roff[2];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            const int qc = q0 + sb * 64 + lc * 8;
            if (qc < QF) {
                const int tap = qc / p.Cin;
                b_ci[sb] = (qc - tap * p.Cin) * 2;
                b_dw[sb] = tap % p.KW - p.pw; b_dh[sb] = (tap / p.KW) % p.KH - p.ph; b_dt[sb] = tap / (p.KW * p.KH) - p.pt;
            } else {
                b_ci[sb] = -1; b_dw[sb] = 0; b_dh[sb] = 0; b_dt[sb] = 0;
            }
            b_roff[sb] = (b_dt[sb] * p.H + b_dh[sb]) * p.W + b_dw[sb];
        }
        auto issue = [&](int g) {                                  // K-tile g -> stage g % NS
            char* st = smem + (g % DW3_NS) * DW3_STAGE + lw * 1024;
            const int ml = g * 32 + rloc;
            const bool live = ml < m_cnt;
            const int m = m_lo + ml;
            unsigned a_off = live ? (unsigned)m * lddy2 + a_col : CN_OOB;
            asm volatile("" : "+v"(a_off));
#pragma unroll
            for (int sl = 0; sl < 5; ++sl)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)(st + sl * 4096), 16, (int)a_off, sl * 128, 0, 0);   // slab column offset as the SCALAR offset: an immediate would also move the LDS address
            const int nt = cn_fastdiv(m, p.mg_hwo, p.sh_hwo), sp = m - nt * HWo;
            const int n = cn_fastdiv(nt, p.mg_t, p.sh_t), t = nt - n * p.T;
            const int ho = cn_fastdiv(sp, p.mg_wo, p.sh_wo), wo = sp - ho * p.Wo;
            const int hs = ho * p.stride, ws = wo * p.stride;
            const int rbase = ((n * p.T + t) * p.H + hs) * p.W + ws;
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
                const int tt = t + b_dt[sb], hh = hs + b_dh[sb], ww = ws + b_dw[sb];
                const bool ok = live && b_ci[sb] >= 0 && (unsigned)tt < (unsigned)p.T && (unsigned)hh < (unsigned)p.H && (unsigned)ww < (unsigned)p.W;
                unsigned b_off = ok ? (unsigned)(rbase + b_roff[sb]) * ldx2 + (unsigned)b_ci[sb] : CN_OOB;
                asm volatile("" : "+v"(b_off));          // ONE load per slab under the full EXEC mask: the vmcnt ladder below counts 7 per K-tile
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (__attribute__((address_space(3))) void*)(st + (5 + sb) * 4096), 16, (int)b_off, 0, 0, 0);
            }
        };
        int issued = 0;
        for (; issued < DW3_NS - 1 && issued < nk; ++issued) issue(issued);
        for (int g = 0; g < nk; ++g) {
            // K-tile g must have landed before the barrier that hands it over; the younger ones stay in flight (7 operations per K-tile)
            const int younger = issued - g - 1;
            if (younger >= 3) asm volatile("s_waitcnt vmcnt(21)" ::: "memory");
            else if (younger == 2) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
            else if (younger == 1) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            dw3_barrier();                                         // (A) stage g % NS is ready / stage (g-1) % NS has been consumed
            if (issued < nk) { issue(issued); ++issued; }          // into stage (g + NS - 1) % NS = (g - 1) % NS
        }
        return;
    }

    // =================================== multiplier waves ===================================
    const int wp = wave & 3, wq = wave >> 2;                       // 4 x 2 waves: rows 80 wp .., columns 64 wq ..
    const int kg = lane >> 4, tq_ = (lane & 15) >> 2, tp_ = lane & 3;
    // transposed-read addresses inside a slab: row = 8 kg + 4 sec + tq_, columns c16 + 4 tp_ .. + 3 of a 16-column sub-tile
    int a_addr[5][2], b_addr[4][2];
#pragma unroll
    for (int sec = 0; sec < 2; ++sec) {
        const int row = 8 * kg + 4 * sec + tq_;
        const int key = dw3_key(row);
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int col = wp * 80 + t * 16 + 4 * tp_;            // 0 .. 319
            a_addr[t][sec] = (col >> 6) * 4096 + row * 128 + (((((col & 63) >> 3)) ^ key) << 4) + (col & 7) * 2;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = t * 16 + 4 * tp_;                      // inside x slab wq
            b_addr[t][sec] = (5 + wq) * 4096 + row * 128 + ((((col >> 3)) ^ key) << 4) + (col & 7) * 2;
        }
    }
    f32x4 acc[5][4];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // bias gradient = column sums of dY, which every q-tile of a (channel block, position range) streams anyway: the dY fragments of sub-tile t
    // (16 channels) are summed by the wq = 0 waves of q-tile t % nsub (nsub = min(q-tiles, 5)): a fifth of the work each, no extra pass over dY
    const int nsub = nbq < 5 ? nbq : 5;
    const bool bias_wave = p.dbias != nullptr && wq == 0 && tile_q < nsub;
    float bsum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < nk; ++g) {
        dw3_barrier();                                             // (A) the loaders have landed stage g % NS
        const char* st = smem + (g % DW3_NS) * DW3_STAGE;
        bf16x8 af[5], bfr[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) bfr[t] = cn_tr_pair(st + b_addr[t][0], st + b_addr[t][1]);
#pragma unroll
        for (int t = 0; t < 5; ++t) af[t] = cn_tr_pair(st + a_addr[t][0], st + a_addr[t][1]);
        if (bias_wave) {
#pragma unroll
            for (int t = 0; t < 5; ++t)
                if (t % nsub == tile_q) {
                    const u32x4 w4 = __builtin_bit_cast(u32x4, af[t]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) bsum[t] += __uint_as_float(w4[e] << 16) + __uint_as_float(w4[e] & 0xffff0000u);
                }
        }
#pragma unroll
        for (int tp = 0; tp < 5; ++tp)
#pragma unroll
            for (int tq = 0; tq < 4; ++tq)
                acc[tp][tq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[tp], bfr[tq], acc[tp][tq], 0, 0, 0);
    }
    const int fr = lane & 15, g4 = lane >> 4;
    if (bias_wave) {                                               // the lane holds column (lane & 15) of rows 8 kg .. 8 kg + 7: fold the four row groups
#pragma unroll
        for (int t = 0; t < 5; ++t)
            if (t % nsub == tile_q) {
                float v = bsum[t];
                v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
                if (lane < 16) atomicAdd(p.dbias + p0 + wp * 80 + t * 16 + lane, v);
            }
    }
#pragma unroll
    for (int tp = 0; tp < 5; ++tp)
#pragma unroll
        for (int tq = 0; tq < 4; ++tq)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int pr = p0 + wp * 80 + tp * 16 + 4 * g4 + rg;
                const int qc = q0 + wq * 64 + tq * 16 + fr;
                if (qc < QF) {
                    float* c = p.dw + (size_t)pr * QF + qc;
                    const float v = acc[tp][tq][rg];
                    if (p.splits > 1 || p.accumulate) atomicAdd(c, v);
                    else *c = v;
                }
            }
}

// dy: bf16 [N,T,Ho,Wo,Cout] (position stride lddy), x: bf16 [N,T,H,W,Cin] (ldx), dw: fp32 [Cout, taps*Cin].  accumulate != 0: dw +=
// (gradient accumulation over micro-batches); otherwise dw is overwritten.  Cin % 8 == 0, ldx % 8 == 0, lddy % 8 == 0 (16-byte rows; Cout itself
// is free: 4 output channels live in an 8-wide buffer), both tensors < 2 GiB -- except the one-tap (Linear) case, which is chunked over rows.
extern "C" int vt_group_colsum(const void* X, int ldx, const void* Y, int ldy, const float* mean, const float* rstd, float* out1, float* out2,
                               long long M, int D, int S, int St, int grouped, long long o_bstride, long long o_segstride, void* stream);      // reduce.hip
// dbias: fp32 [Cout] += column sums of dy (the convolution's / Linear's bias gradient), or NULL.  The 320-row kernel folds them into its own
// pass over dy; otherwise vt_group_colsum runs next to the weight-gradient kernel (same result, one more pass over dy).
extern "C" int vt_conv_dw_bias_cl(const void* dy, long long lddy, const void* x, long long ldx, float* dw, float* dbias,
                                  int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw, int stride,
                                  int accumulate, void* stream);
extern "C" int vt_conv_dw_cl(const void* dy, long long lddy, const void* x, long long ldx, float* dw,
                             int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw, int stride,
                             int accumulate, void* stream) {
    return vt_conv_dw_bias_cl(dy, lddy, x, ldx, dw, nullptr, N, T, H, W, Cin, Cout, KT, KH, KW, pt, ph, pw, stride, accumulate, stream);
}
// What vt_conv_dw_bias_cl does with a geometry: the plan vt_conv_dw_plan reports and vt_conv_dw_bias_cl follows.
struct ConvDwPlan {
    int kernel;            // 1 = conv_dw_kernel (128 x 128 tiles, grid tiles x splits), 2 = conv_dw320_kernel (320 x 128 tiles, grid tiles * splits)
    int tiles, splits, m_chunk;
    int dbias_fused;       // 1: the kernel adds the bias gradient itself, 0: vt_group_colsum does
    long long row_step;    // > 0: a Linear over more rows than one descriptor spans, run in row chunks of this many; the rest describes the first
    int Ho, Wo;
    long long rows_out, x_bytes, dy_bytes;
};
static int cn_dw_plan(long long lddy, long long ldx, int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw,
                      int stride, ConvDwPlan* pl) {
    if (N <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return VT_ERR_BAD_SHAPE;
    if (KT < 1 || KH < 1 || KW < 1 || stride < 1 || pt < 0 || ph < 0 || pw < 0 || 2 * pt != KT - 1) return VT_ERR_BAD_SHAPE;
    const int Ho = (H + 2 * ph - KH) / stride + 1, Wo = (W + 2 * pw - KW) / stride + 1;
    if (Ho <= 0 || Wo <= 0 || (ldx % 8) || (lddy % 8) || ldx < Cin || lddy < Cout || (Cin % 8)) return VT_ERR_BAD_SHAPE;    // a 16-byte chunk must stay inside one tap
    const long long rows_in = (long long)N * T * H * W, rows_out = (long long)N * T * Ho * Wo;
    // The descriptors end with the LOGICAL end of the last row (its Cin / Cout columns, rounded up to a 16-byte chunk), not at
    // rows * ld: when dy or x is a column slice of a wider buffer (the gradient of one half of a skip concatenation), rows * ld counted
    // from the slice's base runs past the end of the allocation, and a ragged column tile of the last rows would read there -- an
    // unmapped page when the allocation ends a segment (memory access fault seen at the full 320x512 size).  Past the descriptor: zeros.
    const long long xb = cn_extent_bytes(rows_in, ldx, (Cin + 7) / 8 * 8), yb = cn_extent_bytes(rows_out, lddy, (Cout + 7) / 8 * 8);
    if (xb >= 0x7fffff00LL || yb >= 0x7fffff00LL) {
        // A Linear's weight gradient (one tap: rows are independent terms of the sum) over more rows than one descriptor spans -- the 720p x
        // 129-frame sequence has 119 312 rows of up to 21 504 columns, 5 GB: row chunks of < 2 GiB each, accumulated into dw in turn.
        if (KT * KH * KW != 1 || stride != 1 || pt || ph || pw) return VT_ERR_BAD_SHAPE;
        const long long ldmax = lddy > ldx ? lddy : ldx;
        const long long step = (0x7fffff00LL / (ldmax * 2) - 1) / 256 * 256;
        if (step < 256) return VT_ERR_BAD_SHAPE;
        const int rc = cn_dw_plan(lddy, ldx, 1, 1, 1, (int)(rows_in < step ? rows_in : step), Cin, Cout, 1, 1, 1, 0, 0, 0, 1, pl);
        if (rc != VT_OK || pl->row_step) return VT_ERR_BAD_SHAPE;
        pl->row_step = step;
        return VT_OK;
    }
    pl->row_step = 0; pl->Ho = Ho; pl->Wo = Wo; pl->rows_out = rows_out; pl->x_bytes = xb; pl->dy_bytes = yb;
    const int taps = KT * KH * KW;
    const int cus = cn_cus();
    static int dw3_env = -1;                 // VT355_CONV_DW320=0: always the 128 x 128 kernel (A/B)
    if (dw3_env < 0) { const char* e = getenv("VT355_CONV_DW320"); dw3_env = e ? atoi(e) : 1; }
    if (dw3_env && g_conv_tile != 1 && (Cout % DW3_P) == 0 && (rows_out >= 2048 || g_conv_tile == 2)) {
        const long long t3 = (long long)(Cout / DW3_P) * ((taps * Cin + DW3_Q - 1) / DW3_Q);
        // one workgroup per CU and pass (140 KiB of LDS): the fewest position splits that fill >= 90 % of whole passes (every split adds
        // P x QF fp32 atomics), at least 8 K-tiles each
        const long long maxs = rows_out / 256 > 0 ? rows_out / 256 : 1;
        long long best_s = 1; double best_e = 0.0;
        for (long long sct = 1; sct <= maxs && t3 * sct <= 4LL * cus; ++sct) {
            const long long wgs = t3 * sct, passes = (wgs + cus - 1) / cus;
            const double e = (double)wgs / (double)(passes * cus);
            if (e > best_e + 1e-9) { best_e = e; best_s = sct; }
            if (e >= 0.9) { best_s = sct; break; }
        }
        int chunk3 = (int)((rows_out + best_s - 1) / best_s);
        chunk3 = (chunk3 + 31) / 32 * 32;
        pl->kernel = 2; pl->tiles = (int)t3; pl->m_chunk = chunk3; pl->splits = (int)((rows_out + chunk3 - 1) / chunk3); pl->dbias_fused = 1;
        return VT_OK;
    }
    const int tiles = ((Cout + 127) / 128) * ((taps * Cin + 127) / 128);
    long long want = (2LL * cus + (long long)tiles - 1) / (long long)tiles;                       // ~2 workgroups per CU
    long long maxs = (rows_out + 511) / 512;                                                       // >= 8 K-tiles per workgroup
    int splits = (int)(want < 1 ? 1 : (want > maxs ? maxs : want));
    if (splits < 1) splits = 1;
    int chunk = (int)((rows_out + splits - 1) / splits);
    chunk = (chunk + 63) / 64 * 64;
    pl->kernel = 1; pl->tiles = tiles; pl->m_chunk = chunk; pl->splits = (int)((rows_out + chunk - 1) / chunk); pl->dbias_fused = 0;
    return VT_OK;
}

// host-only query (tests): kernel, tiles, position splits and rows per split of the launch vt_conv_dw_bias_cl would make for this geometry under
// the current vt_conv_set_tile setting, whether the kernel folds the bias gradient in (1) or vt_group_colsum computes it (0), and row_step > 0
// when the call is run in row chunks of that many (the other values then describe the first chunk).  Each output pointer may be NULL.
extern "C" int vt_conv_dw_plan(long long lddy, long long ldx, int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph,
                               int pw, int stride, int* kernel, int* tiles, int* splits, int* m_chunk, int* dbias_fused, long long* row_step) {
    ConvDwPlan pl;
    const int rc = cn_dw_plan(lddy, ldx, N, T, H, W, Cin, Cout, KT, KH, KW, pt, ph, pw, stride, &pl);
    if (rc != VT_OK) return rc;
    if (kernel) *kernel = pl.kernel;
    if (tiles) *tiles = pl.tiles;
    if (splits) *splits = pl.splits;
    if (m_chunk) *m_chunk = pl.m_chunk;
    if (dbias_fused) *dbias_fused = pl.dbias_fused;
    if (row_step) *row_step = pl.row_step;
    return VT_OK;
}

extern "C" int vt_conv_dw_bias_cl(const void* dy, long long lddy, const void* x, long long ldx, float* dw, float* dbias,
                                  int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw, int stride,
                                  int accumulate, void* stream) {
    ConvDwPlan pl;
    const int prc = cn_dw_plan(lddy, ldx, N, T, H, W, Cin, Cout, KT, KH, KW, pt, ph, pw, stride, &pl);
    if (prc != VT_OK) return prc;
    if ((((uintptr_t)x) | ((uintptr_t)dy)) & 15 || (((uintptr_t)dw) & 3)) return VT_ERR_BAD_ALIGN;
    if (pl.row_step) {
        const long long rows_in = (long long)N * T * H * W, step = pl.row_step;
        for (long long r0 = 0; r0 < rows_in; r0 += step) {
            const long long n = rows_in - r0 < step ? rows_in - r0 : step;
            const int rc = vt_conv_dw_bias_cl((const bf16_t*)dy + r0 * lddy, lddy, (const bf16_t*)x + r0 * ldx, ldx, dw, dbias, 1, 1, 1, (int)n, Cin, Cout,
                                              1, 1, 1, 0, 0, 0, 1, (accumulate || r0 > 0) ? 1 : 0, stream);
            if (rc != VT_OK) return rc;
        }
        return VT_OK;
    }
    const int Ho = pl.Ho, Wo = pl.Wo;
    ConvDwParams p;
    p.dy = (const bf16_t*)dy; p.x = (const bf16_t*)x; p.dw = dw; p.dbias = dbias; p.lddy = lddy; p.ldx = ldx; p.dy_bytes = pl.dy_bytes; p.x_bytes = pl.x_bytes;
    p.M = (int)pl.rows_out; p.Cout = Cout; p.Cin = Cin; p.T = T; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo;
    p.KT = KT; p.KH = KH; p.KW = KW; p.pt = pt; p.ph = ph; p.pw = pw; p.stride = stride; p.accumulate = accumulate;
    p.m_chunk = pl.m_chunk; p.splits = pl.splits;
    cn_magic(Ho * Wo, &p.mg_hwo, &p.sh_hwo); cn_magic(Wo, &p.mg_wo, &p.sh_wo); cn_magic(T, &p.mg_t, &p.sh_t);
    const int taps = KT * KH * KW;
    hipStream_t st = (hipStream_t)stream;
    if (!pl.dbias_fused && dbias != nullptr) {
        if ((((uintptr_t)dbias) & 3) || lddy > 0x7fffffffLL) return VT_ERR_BAD_SHAPE;
        const int rc = vt_group_colsum(dy, (int)lddy, nullptr, 0, nullptr, nullptr, dbias, nullptr, pl.rows_out, Cout, 1, 0, 0, 0, 0, stream);
        if (rc != VT_OK) return rc;
    }
    if (pl.splits > 1 && !accumulate) {
        if (hipMemsetAsync(dw, 0, (size_t)Cout * taps * Cin * 4, st) != hipSuccess) return VT_ERR_LAUNCH;
    }
    if (pl.kernel == 2) hipLaunchKernelGGL(conv_dw320_kernel, dim3((unsigned)((long long)pl.tiles * pl.splits)), dim3(768), 0, st, p);
    else hipLaunchKernelGGL(conv_dw_kernel, dim3(pl.tiles, pl.splits), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH;
}
