/* vt355 -- C ABI of the MI355X-native CogVideoX finetune hot path (libvt355.so, gfx950 only).
 *
 * The reference (VideoVerses/VideoTuna-dev, pure Python) has NO FFI boundary on this path: the
 * denoiser is chosen by `target:` reflection (videotuna/utils/common_utils.py:90-109) and every op is
 * a torch / diffusers / peft call.  This header is the boundary the engine introduces *below* that
 * Python plug-in point; each entry point names the reference call it replaces.  INTEGRATION.md shows
 * the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (workspace too);
 *   - bf16 tensors are raw uint16 storage (`void*`), row-major, innermost stride 1, leading dimensions
 *     (`ld*`, in elements) given explicitly; 16-byte aligned base pointers unless noted;
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*); no hidden syncs,
 *     no allocation, no host reads of device data -> safe under hipGraph capture;
 *   - return 0 on success, a negative VT_ERR_* otherwise; no C++ exception crosses the ABI;
 *   - compute entry points keep no state between calls and are safe from autograd's backward thread (one process per
 *     GPU, as PL's DDPStrategy runs the reference).  Five process-global TUNING knobs exist for tests and A/B timing only --
 *     vt_gemm_set_tile, vt_gemm_set_big_loop, vt_conv_set_tile, vt_conv_set_slots, vt_conv3d_set_kernel, vt_attn_bwd_set_chain (and the VT_* environment variables read once at first use);
 *     they select between kernels that give the same results, the product path never calls them.
 *   - deviation from SURVEY 8(b)'s sketch of this ABI (vt_tensor descriptors, vt_<op>_params structs,
 *     vt_workspace_bytes_<op>, vt_last_error): arguments are flat pointers + leading dimensions (one ctypes call, no struct
 *     marshalling), workspaces are sized by vt_<op>_ws_bytes / vt_<op>_workspace_bytes where an op needs one, errors are the
 *     return code + vt_error_string(code) (no thread-local last-error state).  Listed in DESIGN.md 4.
 */
#ifndef VT355_H
#define VT355_H
#ifdef __cplusplus
extern "C" {
#endif

#define VT_OK 0
#define VT_ERR_BAD_SHAPE (-1)
#define VT_ERR_BAD_ALIGN (-2)
#define VT_ERR_LAUNCH (-3)
#define VT_ERR_UNSUPPORTED (-4)

int vt_version(void);                 /* ABI version, currently 2 (r02: vt_adamw guard, vt_temporal_pool_cl keep_first, UNet entry points) */
const char* vt_arch(void);            /* "gfx950" */
const char* vt_error_string(int code);

/* GEMM epilogues */
#define VT_EPI_BIAS 0        /* C = A W^T + bias                                   (nn.Linear)                */
#define VT_EPI_BIAS_GELU 1   /* C2 = u = A W^T + bias ; C = gelu_tanh(u)           (FeedForward net.0)         */
#define VT_EPI_GATED_RES 2   /* C = R + gate[b,seg] * (A W^T + bias); C2 (optional) = A W^T + bias   (h += gate * to_out / ff.net.2;
                                                                                    gate == NULL -> C = R + ...;
                                                                                    r_mod > 0 -> R row = m % r_mod) */
#define VT_EPI_DGELU 3       /* C = (A W^T) * gelu_tanh'(U)                        (backward through net.0 act) */

/* C[M,N] = A[M,K] * W[N,K]^T, bf16 operands, fp32 accumulate.  K % 64 == 0, N % 4 == 0.
 * A, W and an fp32 C 16-byte aligned; a bf16 C and C2 / R / U 8-byte aligned with leading dimensions that are multiples of 4 (the
 * 256x256 kernel moves them 16 bytes at a time where they are 16-byte aligned with leading dimensions that are multiples of 8).
 * Replaces: every torch.nn.Linear of diffusers CogVideoXBlock / CogVideoXPatchEmbed / TimestepEmbedding /
 * CogVideoXLayerNormZero.linear / proj_out, called by the reference via
 * videotuna/models/cogvideo_hf/cogvideo_pl.py:865-871; rows m belong to sample b = m / S and are text
 * rows when (m % S) < St (diffusers concatenates [text, video]). */
int vt_gemm_bf16(const void* A, int lda, const void* W, int ldw, void* C, int ldc,
                 int M, int N, int K, const void* bias, int epilogue, int out_fp32,
                 const void* R, int ldr, int r_mod,
                 const float* gate_txt, const float* gate_vid, int gate_bstride, int S, int St,
                 void* C2, int ldc2, const void* U, int ldu, void* stream);
/* tile selection of vt_gemm_bf16: 0 = by shape (default), 1 = always the 128x128 kernel, 2 = always the 256x256 kernel,
 * 3 = always the 256x128 producer/consumer kernel */
int vt_gemm_set_tile(int mode);
/* which kernel vt_gemm_bf16 runs for an (M, N, K) problem under the current tile mode: 1 = 128x128, 2 = 256x256, 3 = 256x128
 * producer/consumer, 4 = the producer/consumer kernel's 128-row instantiation; < 0 on a bad shape */
int vt_gemm_bf16_kernel(int M, int N, int K);
/* vt_gemm_bf16 with the tiling named by the caller: tile 0 = by shape (exactly vt_gemm_bf16), 1 / 2 / 3 = that kernel, as under
 * vt_gemm_set_tile.  A non-zero global mode of vt_gemm_set_tile wins over the argument.  Same validation as vt_gemm_bf16;
 * VT_ERR_BAD_SHAPE for a tile outside 0..3.  The kernels are bit-identical, so the argument only moves time. */
int vt_gemm_bf16_tile(const void* A, int lda, const void* W, int ldw, void* C, int ldc,
                      int M, int N, int K, const void* bias, int epilogue, int out_fp32,
                      const void* R, int ldr, int r_mod,
                      const float* gate_txt, const float* gate_vid, int gate_bstride, int S, int St,
                      void* C2, int ldc2, const void* U, int ldu, int tile, void* stream);
/* the tile argument a CogVideoX block passes for its ff.net.2 forward and ff.net.0.proj input-gradient products (N = 1920 / 1984 with
 * a long K, which vt_gemm_bf16's shape rule leaves on the producer / consumer kernel): 2 where the 256x256 kernel was measured ahead
 * (csrc/gemm_bf16.hip has the rule and the rows), 0 = no opinion for every other shape; < 0 on a bad shape */
int vt_gemm_bf16_block_tile(int M, int N, int K);
/* K-loop of the 256x256 kernel: 0 = by shape (default), 1 = always the two-phase loop, 2 = always the eight-phase loop (operand
 * loads in flight across barriers); bit-identical results, tests and A/B timing only */
int vt_gemm_set_big_loop(int mode);
/* epilogue path of the last 256x256-kernel launch: 1 = 16-byte accesses, 0 = the 8-byte path (an operand of the epilogue was not
 * 16-byte aligned, or N % 8 != 0), -1 = no launch yet (tests) */
int vt_gemm_big_last_wide(void);
/* convolution tile choice: 0 = per shape (default), 1 = always the 128 x 128 kernels, 2 = the 320-wide loader / multiplier kernels whenever
 * Cout % 320 == 0 (tests and A/B timing; csrc/convnd.hip) */
int vt_conv_set_tile(int mode);
/* cap of the persistent grid of the 128 x 320 forward convolution kernel, process-global (tests; csrc/convnd.hip): 0 = the device's CU count
 * (default), else 1 .. that count, so that a few thousand positions make workgroups walk several tiles.  The shape rule of vt_conv_cl keeps
 * counting with the device's CUs.  Anything else: VT_ERR_BAD_SHAPE, nothing changes. */
int vt_conv_set_slots(int slots);

/* Weight-gradient GEMM: C[P,Q] (+)= alpha * sum_m A[m,P] * B[m,Q]  (A = dY [M,lda], B = X [M,ldb] bf16, C fp32).
 * P % 128 == 0, Q % 128 == 0.  Replaces: autograd's dW = dY^T X of every nn.Linear (full fine-tuning, config 3). */
int vt_gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int P, int Q,
                    float alpha, int accumulate, void* stream);
/* The same product with the result un-padded on the way out: row p lands in row (p / row_group) * row_keep + p % row_group when
 * p % row_group < row_keep and is dropped otherwise (row_group == 0: rows as they are; P % row_group == 0); likewise columns.  C is
 * [P / row_group * row_keep, >= Q / col_group * col_keep].  Replaces: autograd's dW of OpenSora's attention projections
 * (opensora/models/layers/blocks.py:129-175, 301-347), whose 72-wide heads run padded to 80 here. */
int vt_gemm_nt_bf16_unpad(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int P, int Q,
                          float alpha, int accumulate, int row_group, int row_keep, int col_group, int col_keep, void* stream);

/* out1[g,d] += sum_m X[m,d];  out2[g,d] += sum_m X[m,d]*Yn[m,d]  (Yn = Y, or (Y-mean[m])*rstd[m] with row stats);
 * grouped: the sums of (sample b, seg 0 text / 1 video) go to out + b*o_bstride + seg*o_segstride + d.
 * Bias / adaLN / LayerNorm parameter gradients. */
int vt_group_colsum(const void* X, int ldx, const void* Y, int ldy, const float* mean, const float* rstd,
                    float* out1, float* out2, long long M, int D, int S, int St, int grouped,
                    long long o_bstride, long long o_segstride, void* stream);

/* dgamma/dbeta [2][2][64] (q: gamma,beta; k: gamma,beta) of the per-head LayerNorm, accumulated */
int vt_qk_ln_param_grads(const float* dq_hat, int lddq, const void* dk_hat, int lddk, const void* qkv, int ld,
                         const float* mean, const float* rstd, float* out_2x2x64, long long M, int H,
                         const float* rope_cos, const float* rope_sin, int S, int St, void* stream);
/* LayerNorm / adaLN parameter gradients from grouped sums G1 = sum dy, G2 = sum dy*xhat (see csrc/reduce.hip) */
int vt_ln_param_combine(const float* G1, const float* G2, int G, int D, const void* gamma, const void* beta,
                        const float* scale_txt, const float* scale_vid, int bstride, float* dgamma, float* dbeta,
                        float* dshift_txt, float* dshift_vid, float* dscale_txt, float* dscale_vid, int dbstride,
                        int grouped, void* stream);
/* Linear backward for <= 8 rows: dW += dy^T x, db += sum dy, dx += dy W  (time-embedding / adaLN MLPs) */
int vt_small_linear_bwd(const float* dy, int ldy, const void* x, int ldx, const void* W, float* dW, float* db,
                        float* dx, int lddx, int Bn, int N, int K, void* stream);
int vt_silu_bwd(const float* dy, const void* x, float* dx, long long n, void* stream);

/* Flash attention forward, head_dim 64, non-causal.  Element (b,s,h,d) of q lives at
 * q + b*q_bs + s*q_rs + h*64 + d (same for k, v, o) so a fused QKV projection is consumed in place.
 * lse2[b,h,s] = log2(sum_j exp(scale * q.k_j)) (fp32), kept for the backward.
 * q_prescaled != 0: q was already multiplied by softmax_scale*log2(e) (vt_qk_layernorm_fwd's q_scale), so the
 * kernels use exp2 of the raw scores; dq is still the gradient wrt the UNscaled q_hat, dk wrt k_hat.
 * (forward only) q_prescaled == 2: the same on the 16x16x32-MFMA variant of the kernel (identical contract; not the default).
 * Replaces: F.scaled_dot_product_attention in diffusers CogVideoXAttnProcessor2_0 (cogvideo_pl.py:865-871). */
int vt_attn_fwd_hd64(const void* q, const void* k, const void* v, void* o, float* lse2,
                     int B, int H, int S,
                     long long q_rs, long long k_rs, long long v_rs, long long o_rs,
                     long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                     float softmax_scale, int q_prescaled, void* stream);

/* The same forward with an additive score bias: softmax(q k^T * softmax_scale + bias) v.  bias_t is fp32, TRANSPOSED,
 * [H][S keys][S queries] (bias_t[h][key][q]), shared by every sample; lse2 as above (bias included).
 * Replaces: T5Attention's softmax(scores + position_bias) in transformers' T5EncoderModel, the frozen text encoder the
 * reference calls at cogvideo_pl.py:254-286 / lvdm/modules/encoders/condition.py:81-95 (no scaling there: pass 1.0). */
int vt_attn_fwd_bias_hd64(const void* q, const void* k, const void* v, const float* bias_t, void* o, float* lse2,
                          int B, int H, int S,
                          long long q_rs, long long k_rs, long long v_rs, long long o_rs,
                          long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                          float softmax_scale, void* stream);
/* Split-K C_f32[M,N] = A[M,K] W[N,K]^T for a few hundred rows against a large weight (the T5 encoder at 2 x 226 tokens): the K range
 * is cut into `splits` pieces (a divisor of K/64; <= 0: chosen so that tiles x splits fills the CUs) whose partial tiles are added
 * into C with fp32 atomics; C is zeroed by the call.  vt_residual_cast_bf16: out = bf16(acc (+ R)), the finishing pass.
 * Replaces: the `o` / `wo` nn.Linear of transformers' T5Attention / T5DenseGatedActDense + the residual add of T5LayerSelfAttention /
 * T5LayerFF (modeling_t5.py), reached from cogvideo_pl.py:254-286. */
int vt_gemm_splitk_f32(const void* A, int lda, const void* W, int ldw, float* C, int ldc, int M, int N, int K, int splits, void* stream);
int vt_residual_cast_bf16(const float* acc, long long lda, const void* R, long long ldr, void* out, long long ldo, long long M, int N,
                          void* stream);
/* GroupNorm (+ SiLU) over channels-last activations: x, y bf16 [N, P, C] (P = T*H*W positions, position stride ldx / ldy), G groups
 * of C/G channels, statistics over (P x C/G) in fp32, y = silu?((x - mean) * rstd * gamma + beta).  ws: fp32 scratch of
 * vt_groupnorm_ws_bytes(N, C) bytes.  First kernel of the next scope rows: replaces `Normalize` -> `nonlinearity` in
 * the CogVideoX VAE's ResNet blocks (cogvideo_sat/vae_modules/cp_enc_dec.py:436-459, 681-777; diffusers AutoencoderKLCogVideoX
 * behind cogvideo_pl.py:792-813) and GroupNorm32 -> SiLU in the VideoCrafter2 UNet (lvdm/modules/networks/openaimodel3d.py:229-255),
 * on one channels-last layout instead of the reference's NCHW <-> NCTHW permutes. */
long long vt_groupnorm_ws_bytes(int N, int C);
int vt_groupnorm_silu_cl(const void* x, long long ldx, const void* gamma, const void* beta, void* y, long long ldy,
                         int N, long long P, int C, int G, float eps, int silu, float* ws, long long ws_bytes, void* stream);
/* Causal 3x3x3 convolution on channels-last video activations as an implicit GEMM (no im2col buffer):
 *   y[n,t,h,w,co] = bias[co] + sum_{dt,dh,dw} sum_ci x[n, max(t+dt-2,0), h+dh-1, w+dw-1, ci] * wk[co, (dt,dh,dw), ci]
 * zero padding in h / w, the first frame replicated in front of t.  x: bf16 [N,T,H,W,Cin] (position stride ldx), wk: bf16
 * [Cout, 27*Cin] = torch's Conv3d weight permuted to [Cout,3,3,3,Cin], bias bf16 [Cout] or NULL, y: bf16 [N,T,H,W,Cout].
 * Cin % 64 == 0, Cout % 4 == 0.  Replaces: ContextParallelCausalConv3d (cogvideo_sat/vae_modules/cp_enc_dec.py:356-433) /
 * diffusers CogVideoXCausalConv3d in the VAE encoder the reference runs at cogvideo_pl.py:792-813. */
int vt_causal_conv3d_cl(const void* x, long long ldx, const void* wk, const void* bias, const void* res, long long ldr,
                        void* y, long long ldy, int N, int T, int H, int W, int Cin, int Cout, void* stream);
/* res (optional, bf16 [N,T,H,W,Cout], position stride ldr) is added to the result: the skip of the ResNet block (x + h,
 * cp_enc_dec.py:776).  vt_downsample_conv2d_cl: the VAE's spatial downsample (DownSample3D.forward, cp_enc_dec.py:660-666): per
 * frame, a zero line / column appended at the bottom / right, 3x3 convolution with stride 2; wk bf16 [Cout, 9*Cin] = Conv2d weight
 * permuted to [Cout,3,3,Cin]; y bf16 [N,T,H/2,W/2,Cout]. */
int vt_downsample_conv2d_cl(const void* x, long long ldx, const void* wk, const void* bias, void* y, long long ldy,
                            int N, int T, int H, int W, int Cin, int Cout, void* stream);
/* vt_downsample_conv2d_cl with a residual (bf16 [N,T,H/2,W/2,Cout], position stride ldr) added to the result: the EPI_GATED_RES
 * instantiations of the stride-2 kernels, which no layer of the VAE uses (tests) */
int vt_downsample_conv2d_res_cl(const void* x, long long ldx, const void* wk, const void* bias, const void* res, long long ldr,
                                void* y, long long ldy, int N, int T, int H, int W, int Cin, int Cout, void* stream);
/* Kernel choice of vt_causal_conv3d_cl / vt_downsample_conv2d_cl, process-global (tests and A/B timing; csrc/conv3d.hip).
 * mode: 0 = by shape (default), 1 = always the 128-row kernel, 2 = the 256-row producer / consumer kernel wherever its span check allows;
 * the environment variable VT_CONV_KERNEL, read once, is its initial value.  slots: cap of the persistent grid, 0 = the device's own
 * (CUs rounded down to a multiple of 8), else a multiple of 8 from 8 up to that value.  Anything else: VT_ERR_BAD_SHAPE, nothing changes. */
int vt_conv3d_set_kernel(int mode, int slots);
/* host-only query, no launch: what the launch for this geometry would be under the current setting.  kt = 3, stride = 1: vt_causal_conv3d_cl;
 * kt = 1, stride = 2: vt_downsample_conv2d_cl.  kernel: 1 = 128-row tiles (one per workgroup), 2 = producer / consumer (256-row tiles,
 * persistent); grid: workgroups; tiles: output tiles of that kernel; tiles_per_wg: the most tiles one workgroup walks.  Each output
 * pointer may be NULL.  Computed by the helper the launch itself follows. */
int vt_conv3d_plan(long long ldx, int N, int T, int H, int W, int Cin, int Cout, int kt, int stride,
                   int* kernel, int* grid, int* tiles, int* tiles_per_wg);
/* The encoder's first convolution (RGB): x bf16 [N,T,H,W,8] (8 channels per position, unused ones zero), wk bf16 [Cout, 32*8] =
 * the Conv3d weight as (tap, channel) with taps 27..31 and channels >= Cin zero; 8 taps per K-tile instead of one. */
int vt_causal_conv3d_in8_cl(const void* x, const void* wk, const void* bias, void* y, long long ldy,
                            int N, int T, int H, int W, int Cout, void* stream);
/* Temporal compression of the VAE's DownSample3D (cp_enc_dec.py:640-667).  keep_first != 0 (its rank-0 / fake_cp branch, :645-657, and
 * diffusers' CogVideoXDownsample3D for an ODD frame count): frame 0 kept, frames 1.. averaged in consecutive pairs (a trailing odd
 * frame is dropped): x bf16 [N,T,HW,C] -> y bf16 [N, 1 + (T-1)/2, HW, C].  keep_first == 0 (its other branch, :658-667, and diffusers
 * for an EVEN frame count): avg_pool1d(2, 2) over all frames, y bf16 [N, T/2, HW, C].  Channels-last. */
int vt_temporal_pool_cl(const void* x, long long ldx, void* y, long long ldy, int N, int T, long long HW, int C, int keep_first,
                        void* stream);
/* SpatialNorm3D (+ SiLU) of the VAE decoder: y = silu?( ((x - mean) * rstd * gamma + beta) * mod_y[n,tz,hz,wz,c] + mod_b[n,tz,hz,wz,c] ).
 * x, y: bf16 [N,T,H,W,C] channels-last (position stride ldx / ldy); mod: bf16 [N,Tz,Hz,Wz,2C] contiguous = (conv_y(zq) | conv_b(zq)) at
 * LATENT resolution (1x1x1 convolutions commute with nearest interpolation: one GEMM over the latent's positions, no upsampled zq is
 * stored); hz = h / (H/Hz), wz = w / (W/Wz); T > 1: tz = 0 for t = 0, else 1 + (t-1) / ((T-1)/(Tz-1)); T == 1: tz = 0; the ratios must
 * be powers of two.  Statistics and ws as vt_groupnorm_silu_cl; 64-bit offsets (x / y may exceed 4 GiB).
 * Replaces: SpatialNorm3D.forward (cogvideo_sat/vae_modules/cp_enc_dec.py:462-539: two F.interpolate, two 1x1x1 convolutions over the
 * upsampled latent, GroupNorm, multiply, add) + nonlinearity (:753, :766, :1064) of ContextParallelDecoder3D. */
int vt_spatialnorm_silu_cl(const void* x, long long ldx, const void* gamma, const void* beta, const void* mod, void* y, long long ldy,
                           int N, int T, int H, int W, int C, int Tz, int Hz, int Wz, int G, float eps, int silu, float* ws,
                           long long ws_bytes, void* stream);
/* Upsample3D.forward in one implicit-GEMM launch: nearest 2x in h / w (tup != 0 and T > 1: also in t with frame 0 kept single,
 * To = 1 + 2 (T-1), output frame t reads input frame 0 for t = 0, else 1 + (t-1)/2; otherwise To = T), then the per-frame 3x3 Conv2d:
 *   y[n,t,h,w,co] = bias[co] + sum_{dh,dw,ci} x[n, ts(t), (h+dh-1)>>1, (w+dw-1)>>1, ci] * wk[co,(dh,dw),ci]
 * zero where h+dh-1 / w+dw-1 leaves [0,2H) / [0,2W).  x: bf16 [N,T,H,W,Cin], wk: bf16 [Cout, 9*Cin], y: bf16 [N,To,2H,2W,Cout].
 * Cin % 64 == 0, Cout % 4 == 0; descriptors rebased per tile, 64-bit stores: any size of x and y.  The upsampled tensor is never stored.
 * Replaces: Upsample3D.forward (cogvideo_sat/vae_modules/cp_enc_dec.py:560-622: F.interpolate per 32-channel split, torch.cat, Conv2d). */
int vt_upsample_conv2d_cl(const void* x, long long ldx, const void* wk, const void* bias, void* y, long long ldy,
                          int N, int T, int H, int W, int Cin, int Cout, int tup, void* stream);
/* T5LayerNorm: y[m,:] = x[m,:] * rsqrt(mean(x[m,:]^2) + eps) * w  (bf16 rows of D, fp32 statistics; no mean, no bias) */
int vt_rmsnorm_bf16(const void* x, long long ldx, const void* w, void* y, long long ldy, long long M, int D, float eps,
                    void* stream);
/* T5DenseGatedActDense activation: y[m,f] = gelu_tanh(u[m,f]) * u[m,F+f]  (u = x [Wi0;Wi1]^T from one fused GEMM) */
int vt_gated_gelu_bf16(const void* u, long long ldu, void* y, long long ldy, long long M, int F, void* stream);

/* Flash attention backward.  delta_ws: [B*H*S] fp32 workspace; dq_f32: fp32 [.., H*64] accumulation buffer
 * that the CALLER ZEROES beforehand (dQ is summed across key blocks with fp32 atomics); dk, dv bf16.
 * chain_ws / chain_ws_bytes: optional scratch (256-byte aligned, >= vt_attn_bwd_chain_ws_bytes(B,H,S) bytes, contents
 * of bytes >= 256 don't matter) that lets runs of consecutive key blocks hand their running dQ tile to each other so that
 * only one block per run issues atomics (csrc/attn_bwd.hip); NULL: every key block adds atomically.  ((int*)chain_ws)[8] is
 * the error word of THIS launch: non-zero if a hand-off wait timed out (dQ is then invalid).  ((int*)chain_ws)[16] is
 * STICKY: it counts time-outs over all launches and is never cleared by the library -- the caller zeroes bytes [64, 256)
 * once when it allocates the workspace and hands &((int*)chain_ws)[16] to vt_adamw as `guard`, so that an optimizer step
 * whose gradients came from an invalid launch is refused on the device.
 * Replaces: autograd of the SDPA call above (loss.backward() under PL). */
int vt_attn_bwd_hd64(const void* q, const void* k, const void* v, const void* o, const void* dout,
                     const float* lse2, float* delta_ws, float* dq_f32, void* dk, void* dv,
                     int B, int H, int S,
                     long long q_rs, long long k_rs, long long v_rs, long long o_rs, long long do_rs,
                     long long dq_rs, long long dk_rs, long long dv_rs,
                     long long q_bs, long long k_bs, long long v_bs, long long o_bs, long long do_bs,
                     long long dq_bs, long long dk_bs, long long dv_bs,
                     float softmax_scale, int q_prescaled, void* chain_ws, long long chain_ws_bytes, void* stream);
long long vt_attn_bwd_chain_ws_bytes(int B, int H, int S);
/* tuning / test knob: chain_len 1 = atomics only, 0 = default (3, or VT_BWD_CHAIN); slots 0 = one workgroup per CU,
 * else a smaller persistent grid (multiple of 8) so that small problems run several generations */
int vt_attn_bwd_set_chain(int chain_len, int slots);
/* host-only query, no launch: the plan vt_attn_bwd_hd64 follows for this problem under the current knobs.  have_ws != 0: the caller hands
 * a chain workspace.  chain_len: 1 = every key block adds its dQ atomically, L > 1 = runs of up to L key blocks hand their dQ tiles on;
 * grid: workgroups of the persistent launch; generations: key blocks a workgroup sweeps at most.  Each output pointer may be NULL. */
int vt_attn_bwd_chain_plan(int B, int H, int S, int have_ws, int* chain_len, int* grid, int* generations);

/* y = LayerNorm(x; gamma, beta, eps) * (1 + scale[b,seg]) + shift[b,seg]; gamma/beta may be NULL (no
 * affine), the four modulation pointers may be NULL (plain LayerNorm).  mean/rstd [M] fp32 optional.
 * Replaces: diffusers CogVideoXLayerNormZero.norm + modulate, norm_final, AdaLayerNorm (SURVEY 8(a) a3,a6). */
int vt_ln_modulate_fwd(const void* x, int ldx, void* y, int ldy, const void* gamma, const void* beta,
                       const float* shift_txt, const float* scale_txt, const float* shift_vid,
                       const float* scale_vid, int mod_bstride, float* mean, float* rstd,
                       int M, int D, int S, int St, float eps, void* stream);
/* dx = dres + d/dx[ LN-modulate ](dy)  (dres may be NULL) */
int vt_ln_modulate_bwd(const void* dy, int lddy, const void* x, int ldx, const float* mean, const float* rstd,
                       const void* gamma, const float* scale_txt, const float* scale_vid, int mod_bstride,
                       const void* dres, int lddres, void* dx, int lddx,
                       int M, int D, int S, int St, void* stream);

/* per-head LayerNorm(64, affine) of the q and k thirds of a fused [M, 3*H*64] projection; writes
 * [M, 2*H*64] (q_hat | k_hat) and the statistics [M, 2H].  Replaces attn.norm_q / attn.norm_k.
 * rope_cos/rope_sin (fp32 [S-St, 64], or both NULL): rotary position embedding of the video rows (row m is sequence
 * position m % S; positions >= St rotate), i.e. diffusers' apply_rotary_emb(use_real=True, unbind_dim=-1) that
 * CogVideoXAttnProcessor2_0 runs on q[:, :, text_len:] / k[:, :, text_len:] with the image_rotary_emb tables built at
 * cogvideo_pl.py:442-473 (CogVideoX-5B recipes).  The backward entry points apply the transposed rotation to the
 * incoming gradients before the LayerNorm backward / parameter-gradient sums. */
int vt_qk_layernorm_fwd(const void* qkv, int ld, void* out, int ldo, const void* gq, const void* bq,
                        const void* gk, const void* bk, float* mean, float* rstd,
                        long long M, int H, float eps, float q_scale,
                        const float* rope_cos, const float* rope_sin, int S, int St, void* stream);
int vt_qk_layernorm_bwd(const float* dq_hat, int lddq, const void* dk_hat, int lddk, const void* qkv, int ld,
                        const float* mean, const float* rstd, const void* gq, const void* gk,
                        void* dqkv, int ldd, long long M, int H,
                        const float* rope_cos, const float* rope_sin, int S, int St, void* stream);

/* y[m,:] = x[m,:] * gate[b(m), seg(m)]  (backward of the gated residual) */
int vt_gate_mul(const void* x, int ldx, void* y, int ldy, const float* g_txt, const float* g_vid, int bstride,
                long long M, int D, int S, int St, void* stream);
int vt_silu_bf16(const void* x, void* y, long long n, void* stream);
int vt_cast_f32_bf16(const float* x, void* y, long long n, void* stream);
/* sinusoid(t) [B,D] bf16, cos half first when flip_sin_to_cos (diffusers Timesteps; cf. diffusion_utils.py:9-33) */
int vt_timestep_embedding(const long long* t, void* out, int B, int D, int flip_sin_to_cos, float freq_shift,
                          void* stream);
/* [B,F,C,H,W] bf16 <-> tokens [B*F*(H/P)*(W/P), ldt] with columns (c p q) */
int vt_patchify(const void* img, void* tok, int B, int F, int C, int H, int W, int P, int ldt, void* stream);
int vt_unpatchify(const void* tok, void* img, int B, int F, int C, int H, int W, int P, int ldt, void* stream);

/* scheduler.add_noise (cogvideo_pl.py:864): noisy = sqrt_ab[b]*x0 + sqrt_1mab[b]*noise  (fp32 in, bf16 out) */
int vt_add_noise(const float* x0, const float* noise, const float* sqrt_ab, const float* sqrt_1mab, void* noisy,
                 long long per_sample, int B, void* stream);
/* Sampler (csrc/sampler.hip; CogVideoXWorkFlow.sample, cogvideo_pl.py:476-772).
 *
 * Noise convention (vt355.workflow.sample without a torch generator; a statement of record):
 *   element  e = index inside one sample's logical array of n elements (row-major over the sample's shape); sample b of B
 *   key      seed + b (mod 2^64): sample b under `seed` is sample 0 under `seed + b`
 *   counter  (stream << 40) + e / 4, as (lo, hi, 0, 0); stream 0 = the initial latents, stream i + 1 = the noise of denoising step i.
 *            n <= 2^42 (e / 4 stays below 2^40) and 0 <= stream < 2^24, else VT_ERR_BAD_SHAPE
 *   normal   words (w0, w1, w2, w3) of Philox4x32-10(key, counter) give elements 4 (e / 4) + {0, 1, 2, 3} by Box-Muller on the pairs
 *            (w0, w1) and (w2, w3): u1 = ((w >> 8) + 1) 2^-24 in (0, 1], u2 = (w' >> 8) 2^-24 in [0, 1), both exact in fp32,
 *            rad = sqrt(-2 ln u1), z_even = rad cos(2 pi u2), z_odd = rad sin(2 pi u2) with the precise logf / sincosf
 *            (tests/sampler_ref.py restates it in fp64 on oracle/philox.py)
 * vt_philox_normal: out[b * n + e] for b < B, e < n, fp32 (4-byte aligned) or bf16 (out_bf16 != 0, 2-byte aligned, one rounding of the
 *   fp32 value).  Not torch's generator: it neither reads nor advances one.  Replaces: diffusers randn_tensor (cogvideo_pl.py:651-661).
 * vt_dpm_step: guidance combine + CogVideoXDPMScheduler.step (cogvideo_pl.py:725-746) over B samples of `per` elements, all in fp32:
 *     v  = guided ? v[b] + g (v[B + b] - v[b]) : v[b]        v bf16 [2B, per] (uncond rows, then cond rows) or [B, per]
 *     x0 = sqrt_ab x - sqrt_1mab v                            x bf16 [B, per];  x0_out fp32 [B, per]
 *     d  = second_order ? m3 x0 - m4 x0_old : x0              x0_old fp32 [B, per], NOT read when second_order == 0 (may be NULL)
 *     x' = m1 x - m2 d + m_noise eps                          x_out bf16 [B, per]
 *   eps = noise[b, e] (fp32 [B, per]) or, noise == NULL, the value vt_philox_normal(seed, stream) gives that element, bit for bit;
 *   m_noise == 0: noise is neither read nor drawn.  The coefficients are host scalars (vt355.scheduler computes them in fp64).
 *   Any per >= 1: bf16 pointers 2-byte, fp32 pointers 4-byte aligned (else VT_ERR_BAD_ALIGN); the 8- / 16-byte path is taken only when
 *   per % 4 == 0 and every pointer read or written allows it.  x_out may be x. */
int vt_philox_normal(void* out, int out_bf16, long long n, int B, unsigned long long seed, int stream_id, void* stream);
int vt_dpm_step(const void* v, const void* x, const float* x0_old, const float* noise, void* x_out, float* x0_out,
                long long per, int B, int guided, float g, float sqrt_ab, float sqrt_1mab, float m1, float m2, float m3,
                float m4, float m_noise, int second_order, unsigned long long seed, int stream_id, void* stream);
/* cogvideo_pl.py:872-886: x0_hat = sqrt_ab*noisy - sqrt_1mab*v ; loss = mean_b mean_i w_b (x0_hat-x0)^2 ;
 * optionally d loss / d v * grad_scale (bf16).  partials_ws: >= 512 floats. */
int vt_diffusion_loss(const void* vpred, const void* noisy, const float* x0, const float* sqrt_ab,
                      const float* sqrt_1mab, const float* weights, float* loss, float* partials_ws,
                      void* dvpred, long long per_sample, int B, float grad_scale, void* stream);

/* d loss / d v = grad_out[0] * 2 w_b (x0_hat - x0) (-sqrt_1mab) / (per_sample*B); grad_out is a DEVICE scalar */
int vt_diffusion_loss_bwd(const void* vpred, const void* noisy, const float* x0, const float* sqrt_ab,
                          const float* sqrt_1mab, const float* weights, const float* grad_out, void* dvpred,
                          long long per_sample, int B, void* stream);

/* torch.optim.AdamW step (cogvideo_pl.py:774-779) over one flat fp32 buffer; g is multiplied by grad_scale
 * first; p_bf16 (optional) receives the bf16 compute copy. step is 1-based.  guard (optional, device int): when *guard != 0
 * at execution time the whole update is skipped (p, m, v untouched) -- the sticky error word of vt_attn_bwd_hd64. */
int vt_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, float lr, float beta1,
             float beta2, float eps, float weight_decay, int step, float grad_scale, const int* guard, void* stream);

/* Gradient clipping without a host round trip and without rewriting the gradients (Lightning's gradient_clip_val).
 * vt_grad_sqnorm: read-only sweep over n fp32 values at any 4-byte aligned g; a FIXED grid of vt_grad_sqnorm_partials() (= 2048)
 *   workgroups x 256 threads, workgroup b stores the sum of g^2 over its share to partials[slot * 2048 + b] (every workgroup
 *   stores, zeros included).  No atomics: bit-identical from run to run.  Per thread one fp32 accumulator per 16-byte lane takes at
 *   most ceil(ceil(n / 4) / (2048 * 256)) + 1 sequential additions, then 10 fp32 tree levels (4 lanes, 64-wide wave, 4 waves).
 * vt_clip_finalize: sums partials[0 .. nslots * 2048) in double in a fixed order and stores record[0] = total_norm =
 *   grad_scale * sqrt(sum), record[1] = clip_coef = min(1, max_norm / (total_norm + 1e-6))  (torch.nn.utils.clip_grad_norm_,
 *   norm_type 2, error_if_nonfinite False: a NaN norm gives a NaN coefficient).
 * vt_adamw_clip: vt_adamw on the gradient g * grad_scale * *clip_coef_dev (clip_coef_dev != NULL: the 'norm' algorithm) or
 *   clamp(g * grad_scale, -clip_value, +clip_value) (clip_value > 0: the 'value' algorithm); neither: exactly vt_adamw; both:
 *   VT_ERR_UNSUPPORTED. */
int vt_grad_sqnorm_partials(void);
int vt_grad_sqnorm(const float* g, long long n, float* partials, int slot, void* stream);
int vt_clip_finalize(const float* partials, int nslots, float grad_scale, float max_norm, float* record, void* stream);
int vt_adamw_clip(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, float grad_scale, const int* guard,
                  const float* clip_coef_dev, float clip_value, void* stream);

/* LoRA (peft LoraLayer, cogvideo_pl.py:143-149) */
int vt_lora_down(const void* X, int ldx, const void* A, int lda, int R, void* T, int ldt, long long M, int K,
                 int zero_cols, void* stream);                   /* T[M,16] = X A^T ; T[:,16:16+zero_cols] = 0 */
int vt_skinny_tn(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp,
                 long long osr, float alpha, long long M, int P, float* workspace, void* stream);
                                                                 /* out[p*osp+r*osr] += alpha*sum_m Big[m,p]*Small[m,r];
                                                                    workspace: NULL (atomics) or vt_skinny_tn_workspace_bytes(P)
                                                                    bytes (two-stage, reproducible, no contended atomics) */
long long vt_skinny_tn_workspace_bytes(int P);
int vt_lora_up_add(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int R, long long M, int K,
                   void* stream);                                /* dX += dT A                          */
int vt_lora_pack_b(const float* Bcat, void* Wext, int ldw, int n_adapters, int d_out, int r, float scale, void* stream);
int vt_lora_pack_bt(const float* Bcat, void* WText, int ldwt, int n_adapters, int d_out, int r, float scale, void* stream);

/* LoRA, ranks 17..128 ("wide" layout): adapter j of a fused projection owns the K-extension columns [j*rp, j*rp + r), rp = r rounded
 * up to a multiple of 16, the extension is ext columns wide; all products on bf16 MFMA with fp32 sums */
int vt_lora_down_wide(const void* X, int ldx, const void* A, int lda, int n_adapters, int r, int rp, int ext, void* T, int ldt,
                      long long M, int K, void* stream);         /* T[m, j*rp+i] = sum_k X[m,k] A[j*r+i, k]; 0 elsewhere in [0, ext) */
int vt_lora_tn_wide(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp, long long osr,
                    float alpha, long long M, int P, void* stream);
                                                                 /* out[p*osp+i*osr] += alpha*sum_m Big[m,p]*Small[m,i], R <= 128
                                                                    (fp32 atomics across the row slices) */
int vt_lora_up_add_wide(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r, int rp,
                        long long M, int K, void* stream);       /* dX[m,k] += sum_j sum_i dT[m, j*rp+i] A[j*r+i, k] */
int vt_lora_pack_b_wide(const float* Bcat, void* Wext, int ldw, int n_adapters, int d_out, int r, int rp, int ext, float scale,
                        void* stream);
int vt_lora_pack_bt_wide(const float* Bcat, void* WText, int ldwt, int n_adapters, int d_out, int r, int rp, int ext, float scale,
                         void* stream);

/* LoRA dropout (peft lora_dropout > 0: y = W x + b + (alpha/r) B A drop(x), one nn.Dropout per adapted Linear): _drop siblings of the
 * six rank-side kernels.  No mask is stored; each kernel recomputes it.  Adapter j of a call is adapter site site0 + j (the engine
 * numbers the sites 4 * layer + {0,1,2,3} for to_q, to_k, to_v, to_out.0); element (m, k) of the logical [M, K] adapter input (K, not
 * ldx) is e = m * K + k and is kept iff word e % 4 of Philox4x32-10(key = seed, counter = (site << 36) + e / 4) >= floor(p * 2^32):
 * vt_dropout_bf16's convention with offset = site << 36.  The n_adapters adapters of a call (R = n_adapters * r rank columns in the
 * narrow kernels) read the same X under n_adapters different masks.  1 / (1 - p) multiplies the fp32 sums.  0 <= p < 1, else
 * VT_ERR_BAD_SHAPE.  The masks are Philox, not torch's generator: statistically, not bit-wise, peft's. */
int vt_lora_down_drop(const void* X, int ldx, const void* A, int lda, int R, int n_adapters, void* T, int ldt, long long M, int K,
                      int zero_cols, float p, unsigned long long seed, int site0, void* stream);
                                                                 /* T[m, j r + i] = 1/(1-p) sum_k keep_j(m,k) X[m,k] A[j r + i, k] */
int vt_skinny_tn_drop(const void* Big, int ldb, const void* Small, int lds_, int R, int n_adapters, float* out, long long osp,
                      long long osr, float alpha, long long M, int P, float* workspace, float p, unsigned long long seed, int site0,
                      void* stream);                             /* out[p*osp+i*osr] += alpha/(1-p) sum_m keep_{i / r}(m,p) Big[m,p] Small[m,i];
                                                                    Big is the logical [M, P] adapter input; n_adapters 1 or 3 */
int vt_lora_up_add_drop(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int R, int n_adapters, long long M, int K,
                        float p, unsigned long long seed, int site0, void* stream);
                                                                 /* dX[m,k] += 1/(1-p) sum_j keep_j(m,k) sum_i dT[m, j r + i] A[j r + i, k] */
int vt_lora_down_wide_drop_fits(int n_adapters, int rp);         /* 1 if vt_lora_down_wide_drop takes n_adapters adapters in one call
                                                                    (one masked X block per adapter must fit 64 KB of LDS) */
int vt_lora_down_wide_drop(const void* X, int ldx, const void* A, int lda, int n_adapters, int r, int rp, int ext, void* T, int ldt,
                           long long M, int K, float p, unsigned long long seed, int site0, void* stream);
int vt_lora_tn_wide_drop(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp, long long osr,
                         float alpha, long long M, int P, float p, unsigned long long seed, int site, void* stream);   /* one adapter */
int vt_lora_up_add_wide_drop(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r, int rp,
                             long long M, int K, float p, unsigned long long seed, int site0, void* stream);
/* the dgelu form of the two dropped dX corrections (an adapter whose input is gelu(U): ff.net.2 of the CogVideoX block):
   dX[m,k] += gelu'(U[m,k]) / (1-p) * sum_j keep_j(m,k) sum_i dT[m, .] A[., k]; U bf16 [M, K] with row stride ldu; gelu' is the EPI_DGELU
   epilogue's function and multiplies the fp32 sum before the add */
int vt_lora_up_add_dgelu_drop(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int R, int n_adapters, const void* U,
                              int ldu, long long M, int K, float p, unsigned long long seed, int site0, void* stream);
int vt_lora_up_add_wide_dgelu_drop(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r, int rp,
                                   const void* U, int ldu, long long M, int K, float p, unsigned long long seed, int site0, void* stream);

/* The wide _drop products with an ORIGIN MAP (_at): the call's operand is a piece -- some rows, a column range -- of the adapter's
 * logical input [M_g, K_log], and the mask is keyed by the element's place in THAT array, e = m_g * K_log + k_g:
 *   rows     b = m / seg_local, l = m % seg_local,  m_g = b * seg_global + l + (l < n_first ? off_first : off_rest)
 *   columns  k_g = k0 + k
 * (seg_local = seg_global >= M, n_first = off_first = off_rest = k0 = 0, K_log = K is the identity: the plain _drop entry point, which is
 * the same kernel and returns the same bits.)  VT_ERR_BAD_SHAPE before any launch when k0 % 8 != 0, k0 + K > K_log, K_log % 4 != 0,
 * seg_local <= 0, n_first > seg_local, an offset (or seg_global, n_first) is negative, or the largest e / 4 reaches 2^36 (the next
 * site's counters).  Everything else is the sibling's.
 *
 * HunyuanVideo mask convention (vt355.hunyuan, lora_dropout > 0; a statement of record):
 *   site     adapter site s = the 0-based position of the adapter among the lora_A entries of model.lora.shapes (the q, k, v adapters of
 *            a fused projection are consecutive sites, as the multi-adapter kernels number them: site0 + j)
 *   keep     element (m_g, k) of an adapter's logical input [M_g, K] (K = D, 4 D or 5 D), e = m_g * K + k, is kept iff word e % 4 of
 *            Philox4x32-10(key = seed, counter = (s << 36) + e / 4) >= floor(p * 2^32): vt_dropout_bf16's rule;
 *            oracle/philox.py: dropout_keep_mask(M_g, K, p, seed, offset = s << 36) is the same mask
 *   rows     m_g is the row in the UNSHARDED run's row space of that Linear's input: double-block sites b * Li + l over the image
 *            rows; single-block sites b * (Li + Lt) + l, image rows first, then text rows.  Under Ulysses sequence parallelism a
 *            rank's rows are its contiguous 1/P of the image rows followed by the replicated text rows; the origin map puts them
 *            back (seg_local = Li / P [+ Lt], seg_global = Li [+ Lt], n_first = Li / P, off_first = rank * Li / P, off_rest =
 *            Li - Li / P), so a P-rank run draws the unsharded run's masks.  All ranks of a group use one seed.
 *   columns  linear2's input gradient is produced in two column ranges of its [M, 5 D] input: k0 = 0 (attention half, K = D) and
 *            k0 = D (MLP half, K = 4 D, the dgelu form), both with K_log = 5 D. */
int vt_lora_down_wide_drop_at(const void* X, int ldx, const void* A, int lda, int n_adapters, int r, int rp, int ext, void* T, int ldt,
                              long long M, int K, float p, unsigned long long seed, int site0, long long seg_local, long long seg_global,
                              long long n_first, long long off_first, long long off_rest, int k0, int K_log, void* stream);
int vt_lora_tn_wide_drop_at(const void* Big, int ldb, const void* Small, int lds_, int R, float* out, long long osp, long long osr,
                            float alpha, long long M, int P, float p, unsigned long long seed, int site, long long seg_local,
                            long long seg_global, long long n_first, long long off_first, long long off_rest, int k0, int K_log,
                            void* stream);                       /* Big = columns k0 .. k0 + P of the logical input; one adapter */
int vt_lora_up_add_wide_drop_at(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r, int rp,
                                long long M, int K, float p, unsigned long long seed, int site0, long long seg_local,
                                long long seg_global, long long n_first, long long off_first, long long off_rest, int k0, int K_log,
                                void* stream);                   /* dX, A = columns k0 .. k0 + K of the logical input / of the adapters */
int vt_lora_up_add_wide_dgelu_drop_at(void* dX, int ldx, const void* dT, int ldt, const void* A, int lda, int n_adapters, int r, int rp,
                                      const void* U, int ldu, long long M, int K, float p, unsigned long long seed, int site0,
                                      long long seg_local, long long seg_global, long long n_first, long long off_first,
                                      long long off_rest, int k0, int K_log, void* stream);   /* U = the same columns of the pre-activation */

/* DoRA (peft 0.12 LoraConfig(use_dora=True), DoraLinearLayer without dropout): y = b + c (x) (W x + s B A x), c_j = m_j / norm_j,
 * norm_j = ||W_j + s (B A)_j||_2 detached.  c is folded into the packed operands once per adapter version (csrc/dora.hip).
 * vt_dora_norm: out[j] = norm_j (mag == NULL) or mag[j] / norm_j, j < n_adapters * d_out; W bf16 [n_adapters d_out, K] (row stride ldw),
 *   A bf16 [n_adapters r, K] (lda), B bf16 [n_adapters d_out, r] contiguous -- adapter a owns rows [a d_out, (a+1) d_out) of W and B and
 *   rows [a r, (a+1) r) of A.  fp32 sums in an order fixed by (K, r); B A is never written to memory.  1 <= r <= 128, n_adapters <= 3,
 *   d_out % 8 == 0, K % 8 == 0, W and A 16-byte aligned.
 * vt_dora_scale: dst[j, k] = bf16(c[by_col ? k : j] * src[j, k]) for rows x cols (cols % 8 == 0), one round-to-nearest-even of the fp32
 *   product; src == dst allowed.  vt_dora_transpose_scale: dst[k, j] = bf16(c[j] * src[j, k]), src [rows, cols], both multiples of 8.
 * vt_dora_db_add: G[j, i] += c[j] * S[j, i] over [N, r] fp32.  vt_dora_dm: dm[j] += (sum_gy[j] - bias[j] * sum_g[j]) / mag[j], the
 *   magnitude gradient from vt_group_colsum(X = g, Y = y)'s two sums; bias bf16 [N] | NULL. */
int vt_dora_norm(const void* W, int ldw, const void* A, int lda, const void* B, int n_adapters, int d_out, int r, int K, float scale,
                 const float* mag, float* out, void* stream);
int vt_dora_scale(const void* src, long long lds_, void* dst, long long ldd, const float* c, int rows, int cols, int by_col, void* stream);
int vt_dora_transpose_scale(const void* src, long long src_ld, void* dst, long long dst_ld, const float* c, int rows, int cols,
                            void* stream);
int vt_dora_db_add(float* G, const float* S, const float* c, int N, int r, void* stream);
int vt_dora_dm(const float* sum_g, const float* sum_gy, const void* bias, const float* mag, float* dm, int N, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * VideoCrafter2 UNet path (BASELINE configs[3]): lvdm UNetModel.forward and its backward
 * (videotuna/models/lvdm/modules/networks/openaimodel3d.py:650-694) on ONE channels-last layout [B, T, H, W, C].
 * ------------------------------------------------------------------------------------------------------------------------------ */

/* Zero-padded convolution as an implicit GEMM:  y[n,t,ho,wo,co] = bias[co] + sbias[n,co] + res[...] + sum_{dt,dh,dw,ci}
 * x[n, t+dt-pt, ho*stride+dh-ph, wo*stride+dw-pw, ci] * wk[co, (dt,dh,dw), ci].  x bf16 [N,T,H,W,Cin] (position stride ldx), wk bf16
 * [Cout, KT*KH*KW*Cin] = the torch weight permuted to [Cout, KT, KH, KW, Cin]; y bf16 [N,T,Ho,Wo,Cout]; bias bf16 [Cout] | NULL;
 * sbias fp32 [N, sbias_ld] | NULL (per-sample bias: ResBlock's `h + emb_out[..., None, None]`, openaimodel3d.py:245); res bf16 like
 * y | NULL.  2*pt == KT-1 (no temporal stride), Cin % 64 == 0, Cout % 4 == 0, x spans < 2 GiB.
 * Replaces: Conv2d 3x3 of ResBlock / Upsample / out (openaimodel3d.py:166-170, 193, 110-112, 647), Downsample.op (stride 2, :71-79),
 * Conv3d (3,1,1) of TemporalConvBlock (:278-296); with the flipped, transposed weight it is also their input gradient. */
int vt_conv_cl(const void* x, long long ldx, const void* wk, const void* bias, const float* sbias, int sbias_ld,
               const void* res, long long ldr, void* y, long long ldy,
               int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw, int stride, void* stream);
/* host-only query, no launch: what vt_conv_cl's launch for this geometry would be under the current vt_conv_set_tile / vt_conv_set_slots
 * setting.  kernel: 1 = 128 x 128 tiles (one per workgroup), 2 = 128 x 320 tiles, persistent; grid: workgroups; tiles: output tiles of that
 * kernel; tiles_per_wg: the most tiles one workgroup walks.  Each output pointer may be NULL.  Computed by the helper the launch follows. */
int vt_conv_plan(long long ldx, long long ldy, int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw,
                 int stride, int* kernel, int* grid, int* tiles, int* tiles_per_wg);
/* Weight gradient of the same convolution: dw[co, tap, ci] (+)= sum_m dy[m, co] * x[shift(m, tap), ci]; dw fp32 [Cout, taps*Cin],
 * overwritten or (accumulate != 0) added to.  One tap, no padding: the weight gradient of an nn.Linear of any (multiple-of-8) size.
 * Replaces: autograd's conv / linear weight gradients under loss.backward(). */
int vt_conv_dw_cl(const void* dy, long long lddy, const void* x, long long ldx, float* dw,
                  int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw, int stride,
                  int accumulate, void* stream);
/* vt_conv_dw_cl + the bias gradient: dbias fp32 [Cout] += column sums of dy (NULL: none).  For Cout % 320 == 0 the sums come out of the
 * weight-gradient kernel's own pass over dy; otherwise they are a second pass (vt_group_colsum) -- same result either way. */
int vt_conv_dw_bias_cl(const void* dy, long long lddy, const void* x, long long ldx, float* dw, float* dbias,
                       int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw, int stride,
                       int accumulate, void* stream);
/* host-only query, no launch: what vt_conv_dw_bias_cl's launch for this geometry would be under the current vt_conv_set_tile setting.
 * kernel: 1 = 128 x 128 tiles (grid tiles x splits), 2 = 320-row tiles (grid tiles * splits); splits position ranges of m_chunk rows each
 * (the last may be shorter; more than one: fp32 atomics onto a zeroed or accumulated dw); dbias_fused: 1 = the kernel adds the bias
 * gradient itself, 0 = vt_group_colsum does; row_step > 0: a Linear over more rows than one descriptor spans, run in row chunks of that
 * many, the other values describing the first chunk.  Each output pointer may be NULL.  Computed by the helper the launch follows. */
int vt_conv_dw_plan(long long lddy, long long ldx, int N, int T, int H, int W, int Cin, int Cout, int KT, int KH, int KW, int pt, int ph, int pw,
                    int stride, int* kernel, int* tiles, int* splits, int* m_chunk, int* dbias_fused, long long* row_step);
/* dst[b][c][r] = src[b][r][c] for nb bf16 matrices of rows x cols (multiples of 8), matrix b at src + b*src_boff / dst + b*dst_boff elements
 * (either offset may be negative): W^T of a Linear (torch: w.t().contiguous()) and, per tap, the flipped / channel-swapped weight of a
 * convolution's input-gradient convolution (replaces pack_conv_weight_dx's flip + permute + contiguous; lvdm/modules/networks/
 * openaimodel3d.py convolutions under autograd). */
int vt_transpose_bf16(const void* src, long long src_ld, long long src_boff, void* dst, long long dst_ld, long long dst_boff, int rows, int cols,
                      int nb, void* stream);
/* Many such transposes in one launch: table = device int64 [njobs][8] rows {src, dst, src_ld, dst_ld, rows, cols, first_block, tiles_x}
 * (64 x 64 tiles; first_block = running sum of the jobs' tile counts; rows, cols, leading dimensions multiples of 8, 16-byte aligned
 * pointers), total_blocks = the sum.  Replaces: the same per-step W^T / input-gradient-weight copies as vt_transpose_bf16, for ALL
 * weights of a model at once (autograd's saved `weight.t()` views of every nn.Linear / conv under full fine-tuning). */
int vt_transpose_multi_bf16(const void* table, int njobs, long long total_blocks, void* stream);
/* Test hook: the byte extents vt_conv_cl (fwd_x_bytes) and vt_conv_dw_cl (dw_x_bytes, dw_dy_bytes) give their buffer descriptors for this
 * geometry.  An operand may be a column slice of a wider buffer (one half of a skip concatenation h = cat([h, hs.pop()], dim=1),
 * openaimodel3d.py:686-690, or its gradient): the descriptors must end with the last row's logical columns, never at rows * ld, which
 * counted from a slice base lies past the allocation.  A test asserts extent <= bytes from the slice base to the allocation end. */
int vt_conv_desc_extents(long long ldx, long long lddy, int N, int T, int H, int W, int Cin, int Cout, int KH, int KW, int ph, int pw,
                         int stride, long long* fwd_x_bytes, long long* dw_x_bytes, long long* dw_dy_bytes);
/* Backward of vt_groupnorm_silu_cl.  ws_fwd: the workspace the forward call left (mean | rstd | a | b per (n, c)); ws_bwd: scratch of
 * vt_groupnorm_ws_bytes(N, C) bytes; dgamma / dbeta fp32 [C] ACCUMULATED (NULL: skipped); dx overwritten, or added to when
 * accumulate != 0.  Replaces: autograd of GroupNormSpecific / nn.GroupNorm (+ SiLU) (lvdm/modules/utils.py:192-203). */
int vt_groupnorm_silu_bwd_cl(const void* dy, long long lddy, const void* x, long long ldx, const void* gamma,
                             const float* ws_fwd, float* ws_bwd, long long ws_bytes, void* dx, long long lddx,
                             float* dgamma, float* dbeta, int N, long long P, int C, int G, int silu, int accumulate, void* stream);
/* GEGLU (lvdm/modules/attention.py:522-529): h [M, 2F] = (a | gate) from the projection; y = a * gelu(gate) (erf GELU) */
int vt_geglu_fwd(const void* h, long long ldh, void* y, long long ldy, long long M, int F, void* stream);
int vt_geglu_bwd(const void* dy, long long lddy, const void* h, long long ldh, void* dh, long long lddh, long long M, int F, void* stream);
/* out[m,:] = a[m,:] + b[m,:] (bf16 rows; gradient accumulation where a tensor feeds two consumers) */
int vt_add_rows_bf16(const void* a, long long lda, const void* b, long long ldb, void* out, long long ldo, long long M, int C, void* stream);
/* nn.Dropout(p) in training mode on bf16 rows: y = keep ? x / (1 - p) : 0, keep(m, c) = Philox4x32-10(key seed, counter offset + e / 4)[e % 4]
 * >= p * 2^32 with e = m * C + c -- a pure function of (seed, offset, element), so the backward pass is the same call on the gradient and no
 * mask is kept.  mask_out: uint8 [M, C] keep flags or NULL (parity tests hand the mask to the oracle).  C % 8 == 0.
 * Replaces: the three nn.Dropout(0.1) of TemporalConvBlock (openaimodel3d.py:278-296) under model.train(). */
int vt_dropout_bf16(const void* x, long long ldx, void* y, long long ldy, long long M, int C, float p, unsigned long long seed,
                    unsigned long long offset, void* mask_out, void* stream);
/* Row maps on [.., C] bf16 rows, out (+)= src[map]: mode 0: [nb, d1, d2, C] -> [nb, d2, d1, C] (the `b c t h w <-> (b h w) t c`
 * rearranges of TemporalTransformer.forward, attention.py:476-481, 509-516); 1: nearest x2 upsample [nb, d1, d2] -> [nb, 2 d1, 2 d2]
 * (Upsample.forward, openaimodel3d.py:112-120); 2: zero insertion, same shapes (input gradient of the stride-2 Downsample.op);
 * 3: 2x2 block sum [nb, 2 d1, 2 d2] -> [nb, d1, d2] (backward of 1). */
int vt_row_map_bf16(const void* src, long long lds, void* out, long long ldo, int mode, long long nb, int d1, int d2, int C,
                    int accumulate, void* stream);
/* q_sample (videotuna/schedulers/ddpm.py:216-222) with the dynamic rescaling of lvdm/ddpm3d.py:740-741:
 * x_t = sqrt_ab[b] * scale[b] * x0 + sqrt_1mab[b] * noise (fp32 in, bf16 out; scale NULL = 1) */
int vt_q_sample(const float* x0, const float* noise, const float* sqrt_ab, const float* sqrt_1mab, const float* scale, void* xt,
                long long per_sample, int B, void* stream);
/* eps-prediction loss of LVDMFlow.p_losses (lvdm/ddpm3d.py:787-847, logvar == 0): loss[0] = mean (pred - target)^2;
 * dpred (bf16 | NULL) = d loss / d pred * grad_scale */
int vt_mse_loss(const void* pred, const float* target, float* loss, void* dpred, long long total, float grad_scale, void* stream);

/* Attention against <= 128 resident keys, head_dim 64 (csrc/attn_small.hip).  Element (item b, row s, head h, d) at
 * base + b*bs + s*rs + h*64 + d.  mask_block == 0: NB items of Sq queries x Sk keys -- the text cross-attention attn2 of
 * SpatialTransformer's BasicTransformerBlock (lvdm/modules/attention.py:101-181; item = sample, the T*H*W positions of a sample share
 * its 77 text keys).  mask_block = T (32 % T == 0): q, k, v, o are ONE row space of Sq rows = consecutive sequences of T rows, a row
 * attends to its own sequence -- both attentions of TemporalTransformer (attention.py:395-519) on pixel-major rows; NB = 1, Sk = Sq,
 * batch strides ignored.  lse2: fp32 [NB, H, Sq].  Backward: dq bf16 like q; mask_block > 0: dk, dv bf16 in the k / v row space;
 * mask_block == 0: dk32, dv32 fp32 [NB, Sk, dk_rs] accumulators ZEROED BY THE CALLER. */
int vt_attn_small_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, int NB, int H, int Sq, int Sk,
                      long long q_rs, long long q_bs, long long k_rs, long long k_bs, long long v_rs, long long v_bs,
                      long long o_rs, long long o_bs, float softmax_scale, int mask_block, void* stream);
int vt_attn_small_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2,
                      void* dq, void* dk, void* dv, float* dk32, float* dv32, int NB, int H, int Sq, int Sk,
                      long long q_rs, long long q_bs, long long k_rs, long long k_bs, long long v_rs, long long v_bs,
                      long long o_rs, long long o_bs, long long do_rs, long long do_bs, long long dq_rs, long long dq_bs,
                      long long dk_rs, long long dv_rs, float softmax_scale, int mask_block, void* stream);

/* Packed temporal self-attention with learned relative-position tables, head_dim 64 (csrc/attn_relpos.hip): both attentions of
 * TemporalTransformer under use_relative_position (lvdm/modules/attention.py:19-42, 126-149; the VideoCrafter1 / LVDM layout).
 * Row space as vt_attn_small_* with mask_block = T: q, k, v, o are R rows = R / T consecutive sequences of T rows (32 % T == 0), element
 * (row s, head h, d) at base + s*rs + h*64 + d.  rel_k, rel_v: bf16 [2P+1, 64], shared by all heads.  With idx(i, j) =
 * clamp(j - i, -P, P) + P: S[i,j] = scale (q_i.k_j + q_i.rel_k[idx]), p = softmax_j S, o_i = sum_j p[i,j] (v_j + rel_v[idx]).
 * lse2: fp32 [H, R], base-2 log-sum-exp of the total scaled score.  Backward: dq, dk, dv bf16 in the row space, written whole;
 * d_rel_k, d_rel_v fp32 [2P+1, 64], the gradients summed over all sequences and heads are ADDED into them (fp32 atomics on the way: not
 * bitwise reproducible from run to run); either may be NULL, with both NULL no table-gradient work is done and workspace may be NULL,
 * otherwise workspace: vt_attn_relpos_workspace_bytes() bytes (a constant; zeroed by the call).  A refused call writes nothing. */
long long vt_attn_relpos_workspace_bytes(void);
int vt_attn_relpos_fwd(const void* q, const void* k, const void* v, const void* rel_k, const void* rel_v, void* o, float* lse2,
                       int R, int H, int T, int P, long long q_rs, long long k_rs, long long v_rs, long long o_rs,
                       float softmax_scale, void* stream);
int vt_attn_relpos_bwd(const void* q, const void* k, const void* v, const void* rel_k, const void* rel_v, const void* o,
                       const void* dout, const float* lse2, void* dq, void* dk, void* dv, float* d_rel_k, float* d_rel_v,
                       void* workspace, int R, int H, int T, int P, long long q_rs, long long k_rs, long long v_rs,
                       long long o_rs, long long do_rs, long long dq_rs, long long dk_rs, long long dv_rs,
                       float softmax_scale, void* stream);

/* Dual-context cross-attention, head_dim 64 (csrc/attn_dual.hip): o = softmax(q K^T s) V + img_scale * softmax(q K_ip^T s) V_ip, two
 * separate softmaxes over the text keys of the sample (k, v [B, Sa <= 96, .]) and the image keys of the query's frame (k_ip, v_ip
 * [B * Sq / rows_per_frame, Sb <= 32, .]; rows [f*rows_per_frame, (f+1)*rows_per_frame) of sample b meet item b * Sq / rows_per_frame + f)
 * -- DynamiCrafter's CrossAttention with img_cross_attention (lvdm/modules/attention.py:45-170).  rows_per_frame divides Sq and need
 * not be a multiple of 32; rows_per_frame = Sq is one image set per sample.  Strides as vt_attn_small_*.  lse2: fp32 [2, B, H, Sq]
 * (text plane, image plane).  Backward: dq bf16 like q; dk32, dv32 fp32 [B, Sa, H*64] and dkip32, dvip32 fp32
 * [B * Sq / rows_per_frame, Sb, H*64], contiguous and fully written; the forward's o is not needed.  ws: scratch of
 * vt_attn_dual_ws_floats(...) fp32 elements (per-chunk partial sums added in a fixed order: no atomics, reproducible bits). */
long long vt_attn_dual_ws_floats(int B, int H, int Sq, int rows_per_frame, int Sa, int Sb);
int vt_attn_dual_fwd(const void* q, const void* k, const void* v, const void* k_ip, const void* v_ip, void* o, float* lse2,
                     int B, int H, int Sq, int rows_per_frame, int Sa, int Sb,
                     long long q_rs, long long q_bs, long long k_rs, long long k_bs, long long v_rs, long long v_bs,
                     long long kip_rs, long long kip_bs, long long vip_rs, long long vip_bs, long long o_rs, long long o_bs,
                     float softmax_scale, float img_scale, void* stream);
int vt_attn_dual_bwd(const void* q, const void* k, const void* v, const void* k_ip, const void* v_ip, const void* dout,
                     const float* lse2, void* dq, float* dk32, float* dv32, float* dkip32, float* dvip32, float* ws,
                     long long ws_floats, int B, int H, int Sq, int rows_per_frame, int Sa, int Sb,
                     long long q_rs, long long q_bs, long long k_rs, long long k_bs, long long v_rs, long long v_bs,
                     long long kip_rs, long long kip_bs, long long vip_rs, long long vip_bs, long long do_rs, long long do_bs,
                     long long dq_rs, long long dq_bs, float softmax_scale, float img_scale, void* stream);

/* Flash attention for head dimensions other than 64 (csrc/attn_gen.hip): head_dim 80 (OpenSora STDiT's 72, zero padded: 16 heads x 72,
 * opensora/models/layers/blocks.py:139-225 `Attention` and :472-505 `MultiHeadCrossAttention`) or 128 (HunyuanVideo,
 * hunyuan/hyvideo_t2v/modules/attenion.py:60-156).  Element (item b, row s, head h, d) at base + b*bs + s*rs + h*hstride + d.
 * kv_len: int32 [NB] valid keys per item (the BlockDiagonalMask.from_seqlens([N]*B, y_lens) text mask, blocks.py:497-500) | NULL.
 * mask_block = T > 0: packed sequences of T rows in one row space (STDiT's 16-frame temporal attention), NB = 1, Sk = Sq.
 * lse2 fp32 [NB, H, Sq].  Backward: dq bf16 like q; packed: dk, dv bf16; otherwise dk32, dv32 fp32 [NB, Sk, dk_rs] ZEROED BY THE CALLER. */
int vt_attn_gen_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, const int* kv_len, int head_dim, int hstride,
                    int NB, int H, int Sq, int Sk, long long q_rs, long long q_bs, long long k_rs, long long k_bs, long long v_rs,
                    long long v_bs, long long o_rs, long long o_bs, float softmax_scale, int mask_block, void* stream);
int vt_attn_gen_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2, const int* kv_len,
                    void* dq, void* dk, void* dv, float* dk32, float* dv32, int head_dim, int hstride, int NB, int H, int Sq, int Sk,
                    long long q_rs, long long q_bs, long long k_rs, long long k_bs, long long v_rs, long long v_bs,
                    long long o_rs, long long o_bs, long long do_rs, long long do_bs, long long dq_rs, long long dq_bs,
                    long long dk_rs, long long dv_rs, float softmax_scale, int mask_block, void* stream);

/* OpenSora v1.0 training loss, LatentDiffusion.p_losses (videotuna/models/opensora/models/iddpm3d.py:1332-1413) for the defaults EPSILON /
 * LEARNED_RANGE / MSE: out fp32 [B, 2C, ...] = (eps_hat | v);  loss = mean_b( mse_b + vb_b ) with the variational-bound term of
 * _vb_terms_bpd (:1543-1583) through OpenSoraScheduler.p_mean_variance (:444-519, whose inverted mean-type branch :497-500 is reproduced).
 * coef fp64 [B, 8] = sqrt_ac, sqrt_1mac, posterior_mean_coef1, coef2, min_log, max_log, (t == 0), 0 at the sample's timestep; the VB
 * arithmetic is fp64 as in the reference (float64 posterior tables).  loss3 fp64 [3] = loss, mse, vb; dout fp32 like out | NULL. */
int vt_opensora_loss(const float* out, const float* x0, const float* noise, const double* coef, double* loss3, float* dout,
                     long long per_channel, int C, int B, float grad_scale, void* stream);

/* FP8 (OCP E4M3) GEMM with per-tensor scales, real fp8 MFMA (csrc/gemm_fp8.hip): C (bf16) = (Aq Wq^T) * scale_a * scale_w + bias.
 * Replaces: fp8_linear_forward (videotuna/models/hunyuan/hyvideo_t2v/modules/fp8_optimization.py:55-80), which keeps E4M3 weights with a
 * per-tensor scale but de-quantises to bf16 for F.linear (weight-only emulation); north_star asks for fp8 MFMA (configs[4], a16).
 * A, W: float8_e4m3fn bytes [M, lda] / [N, ldw]; scales: device fp32 scalars; K % 128 == 0, N % 4 == 0.
 * vt_quantize_fp8: x bf16 -> e4m3 with scale = max|x| / 448 (fp8_optimization.py:58-60) written to scale[0] (given_scale != 0: scale[0] is
 * an input, e.g. the checkpoint's fp8_scale); ws: device uint32 [1] scratch. */
int vt_gemm_fp8(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* bias,
                const float* scale_a, const float* scale_w, void* stream);
int vt_quantize_fp8(const void* x, long long ldx, void* y, long long ldy, long long M, int K, float* scale, unsigned int* ws,
                    int given_scale, void* stream);

/* MX-scaled FP8 GEMM and delayed per-tensor scaling (csrc/gemm_mxfp8.hip; HunyuanVideo fp8="mfma").
 * vt_gemm_mxfp8: C = epilogue((Aq Wq^T) * scale_a * scale_w [+ At Wt^T] + bias) on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3, unit block
 * scales); epilogue EPI_BIAS / EPI_BIAS_GELU / EPI_GATED_RES with the operands of vt_gemm_bf16; optional bf16 tail At [M, Kt], Wt [N, Kt]
 * (Kt 0 or a multiple of 32 up to 384, ldat / ldwt >= Kt; above 64 columns the tail is staged through LDS); optional e4m3 copy Cq = e4m3(C / scale_out) with max |C| into amax.  K % 128 == 0, N % 4 == 0; scales on the device.
 * vt_cast_fp8_scaled: x bf16 -> e4m3 with a device scale, max |x| into amax; row m reads x row (m / L) * Lj + off + m % L (L = 0: m) and
 * is optionally copied (bf16) to cp.  vt_ln_modulate_fwd_fp8: vt_ln_modulate_fwd plus an e4m3 copy of y and its amax.
 * vt_fp8_scale_update: per site, history [n, H] <- (amax, history[:, :-1]), scale = max(history) / 448 (1 if 0), amax cleared.
 * amax slots are uint32 holding non-negative float bits.
 * Input-gradient products of that mode (HunyuanBlocks fp8_dgrad; format codes 0 = e4m3, 1 = e5m2, both OCP):
 * vt_gemm_mxfp8_dx: C = epilogue((Gq WqT^T) * scale_g * scale_w [+ At Wt^T]), Gq [M, ldg] the quantised output gradient in format fmt_g,
 * WqT [N, ldw] e4m3 bytes of the transposed weight (row / column slices through ldw); epilogue EPI_BIAS (plain), EPI_DGELU (times
 * gelu'(pre_act_in)) or EPI_GATED_RES (+ residual, no gates); Cq (EPI_DGELU only): copy of C in format fmt_out, as vt_gemm_mxfp8's.
 * vt_cast_fp8_fmt: vt_cast_fp8_scaled with the target format as an argument (e5m2 saturates at +-57344).
 * vt_gate_mul_fp8: vt_gate_mul (y bit-equal) plus q = fp8(y / scale) in format fmt and max |y| into amax.
 * vt_fp8_scale_update_fmax: vt_fp8_scale_update with scale = max(history) / fmax (448: e4m3, 57344: e5m2).
 * Measured (M 10 456): the dX products 1.4-1.9x vt_gemm_bf16 (profiles/r05_mxfp8_dx_kbench.txt); the LoRA step 614.7 -> 584.3 ms
 * (profiles/r05_hunyuan_fp8_dgrad_ab.json). */
int vt_gemm_mxfp8(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* bias,
                  const float* scale_a, const float* scale_w, int epilogue, const void* residual, int ldr,
                  const float* gate_txt, const float* gate_vid, int gate_bstride, int S, int St, void* pre_act_out, int ldc2,
                  const void* At, int ldat, const void* Wt, int ldwt, int Kt, void* Cq, int ldcq, const float* scale_out,
                  unsigned int* amax, void* stream);
int vt_cast_fp8_scaled(const void* x, long long ldx, void* y, long long ldy, void* cp, long long ldcp, long long M, int K, int L,
                       int Lj, int off, const float* scale, unsigned int* amax, void* stream);
int vt_ln_modulate_fwd_fp8(const void* x, int ldx, void* y, int ldy, const void* gamma, const void* beta,
                           const float* shift_txt, const float* scale_txt, const float* shift_vid,
                           const float* scale_vid, int mod_bstride, float* mean, float* rstd,
                           int M, int D, int S, int St, float eps, void* q, int ldq, const float* qscale, unsigned int* amax,
                           void* stream);
int vt_fp8_scale_update(unsigned int* amax, float* history, float* scale, int n, int H, void* stream);
int vt_gemm_mxfp8_dx(const void* G, int ldg, int fmt_g, const void* WT, int ldw, void* C, int ldc, int M, int N, int K,
                     const float* scale_g, const float* scale_w, int epilogue, const void* residual, int ldr,
                     const void* pre_act_in, int ldu, const void* At, int ldat, const void* Wt, int ldwt, int Kt,
                     void* Cq, int ldcq, int fmt_out, const float* scale_out, unsigned int* amax, void* stream);
int vt_cast_fp8_fmt(const void* x, long long ldx, void* y, long long ldy, void* cp, long long ldcp, long long M, int K, int L,
                    int Lj, int off, int fmt, const float* scale, unsigned int* amax, void* stream);
int vt_gate_mul_fp8(const void* x, int ldx, void* y, int ldy, const float* g_txt, const float* g_vid, int bstride, long long M,
                    int D, int S, int St, void* q, int ldq, int fmt, const float* scale, unsigned int* amax, void* stream);
int vt_fp8_scale_update_fmax(unsigned int* amax, float* history, float* scale, int n, int H, float fmax, void* stream);

/* HunyuanVideo q/k preparation, head_dim 128 (csrc/qknorm128.hip): per-head RMSNorm(eps, weight [128]) of the q and k thirds of a fused
 * [M, 3*H*128] projection, rotary embedding of the first S_rope positions of every sample (image tokens; cos / sin fp32 [S_rope, 128] | NULL),
 * and the scatter of q^ | k^ | v into the joint [image; text] sequence: out row = (m / L) * Lout + row_off + m % L.  rstd fp32 [M, 2H].
 * Replaces: img_attn_q_norm / img_attn_k_norm / apply_rotary_emb / torch.cat of MMDoubleStreamBlock.forward and q_norm / k_norm / the
 * sliced rotary of MMSingleStreamBlock.forward (videotuna/models/hunyuan/hyvideo_t2v/modules/models.py:166-196, 351-361). * Backward: dgq / dgk fp32 [128] accumulated (both NULL: the norm weights are frozen, the reduction is skipped). */
int vt_qk_rmsnorm_rope128_fwd(const void* qkv, long long ld, void* out, long long ldo, const void* gq, const void* gk, float* rstd,
                              const float* rope_cos, const float* rope_sin, long long M, int H, int L, int Lout, int row_off,
                              int S_rope, float eps, void* stream);
int vt_qk_rmsnorm_rope128_bwd(const void* dout, long long lddo, const void* qkv, long long ld, void* dqkv, long long ldd, const void* gq,
                              const void* gk, const float* rstd, const float* rope_cos, const float* rope_sin, float* dgq, float* dgk,
                              long long M, int H, int L, int Lout, int row_off, int S_rope, void* stream);

/* ---- long-sequence attention, head_dim 128 (csrc/attn128.hip) ----------------------------------------------------------------------
 * HunyuanVideo's joint [image; text] attention at 10^4 - 10^5 tokens: `attention(q, k, v, mode="flash", cu_seqlens_q, cu_seqlens_kv, ...)`,
 * videotuna/models/hunyuan/hyvideo_t2v/modules/attenion.py:60-156, called from MMDoubleStreamBlock / MMSingleStreamBlock
 * (modules/models.py:203-221, 362-378), and its autograd.  Element (b, s, head, d) of q / k / v / o / dout / dk / dv at
 * base + b*bs + s*rs + head*128 + d (bf16; the fused qkv projection is consumed in place); kv_len: int32 [B] on the device (valid rows
 * and keys of every sample, = cu_seqlens[2b+1] - cu_seqlens[2b]) or NULL; lse2: fp32 [B, H, S], log2-domain.
 * Backward: delta_ws fp32 [B*H*S] scratch.  dq_bf16 != NULL: two passes (dK / dV key-stationary; dQ query-stationary with S and dP recomputed),
 * dQ written once in bf16 with row stride dqb_rs / batch stride dqb_bs (elements), dq32 untouched.  dq_bf16 == NULL: one pass, dQ added
 * atomically (softmax_scale-scaled) to the fp32 accumulator dq32 (strides dq_rs / dq_bs), ZEROED BY THE CALLER.  dk, dv are written for every
 * row < S (zeros for keys >= kv_len[b]). */
int vt_attn128_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, const int* kv_len, int B, int H, int S,
                   long long q_rs, long long k_rs, long long v_rs, long long o_rs,
                   long long q_bs, long long k_bs, long long v_bs, long long o_bs, float softmax_scale, void* stream);
int vt_attn128_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2, const int* kv_len,
                   float* delta_ws, float* dq32, void* dq_bf16, void* dk, void* dv, int B, int H, int S,
                   long long q_rs, long long k_rs, long long v_rs, long long o_rs, long long do_rs, long long dq_rs, long long dqb_rs,
                   long long dk_rs, long long dv_rs, long long q_bs, long long k_bs, long long v_bs, long long o_bs, long long do_bs,
                   long long dq_bs, long long dqb_bs, long long dk_bs, long long dv_bs, float softmax_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
