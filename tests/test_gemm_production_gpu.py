"""The GEMMs at the shapes, operand layouts and fused epilogues the models actually run, element by element against float64.

Every row of SITES is one call site (file:function) with the views it passes: leading dimensions, the row / column offsets of weight
slices and output column slices, the epilogue and its operands.  Each vt_gemm_bf16 row runs under the default dispatch and under each
forced tiling (vt_gemm_set_tile 1 = 128x128, 2 = 256x256 persistent, 3 = 256x128 producer / consumer, persistent), and every launch is
checked for
  1. every element against a float64 reference of the same bf16 operands, within a per-element bound (see _bound below);
  2. the second output (GELU pre-activation, un-gated branch) bit-equal to the EPI_BIAS output of the same tiling;
  3. sentinel rows past M and sentinel columns around a column-slice output left untouched;
  4. a second launch bit-identical to the first (no atomics in these kernels);
  5. the default launch bit-identical to the forced tiling the dispatcher reports (vt_gemm_bf16_kernel), and over the table the defaults
     reaching every kernel the library ships.
The MX-fp8 / fp8 rows and the 320-wide UNet Linears (ops.linear_rows -> vt_conv_cl) get checks 1, 3, 4; the fp8 output copy of
vt_gemm_mxfp8 must equal the cast of the bf16 output as written, and its amax slot the exact maximum.  The references run on the device
in float64, chunked by rows; a self-check shows the comparator rejects a 1 + 2^-5 error in one 16x16 block, two swapped rows and a
neighbouring sample's gate, and that the device float64 reference agrees with numpy."""
import math
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from parity import SENT, SENT8, poisoned

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
F64 = torch.float64
U32 = 2.0 ** -24                     # unit roundoff of fp32
SIG_ERR = 2.0 ** -20                 # absolute error bound of the kernels' GELU sigmoid (see _bound)
FP8_GROUP_ERR = 2.0 ** -9            # fp8 MFMA: loss of one in-instruction product group, relative to its largest product (see _fp8_group_term)
K0, K1 = 0.7978845608028654, 0.044715
TILE = {1: (128, 128), 2: (256, 256), 3: (256, 128), 4: (128, 128)}
KNAME = {1: "128x128", 2: "256x256", 3: "pc 256x128", 4: "pc 128x128"}

# CogVideoX-2B LoRA at micro-batch 4: 4 x (226 text + 17 550 video) rows, d = 1920, K-extension EXT = 64 (engine.py); the modulation
# table holds 30 layers x 2 LayerNormZero x 6 chunks of d per sample (gate_bstride = its row stride, engine._mod)
CB, CS, CST, CD = 4, 17776, 226, 1920
CM = CB * CS
COG_BS = 30 * 12 * CD
# HunyuanVideo bench shape: B = 1, 10 200 image + 256 text rows, D = 3072, MLP 12 288 (hunyuan.py); EXT = 64
HLI, HLT, HD, HF = 10200, 256, 3072, 12288
HLJ = HLI + HLT
# STDiT-XL/2 at the bench shape: B = 4, T = 16, S = 256 -> 16 384 rows, width 1152 (stdit.py)
SB, SRPS, SSP, SD = 4, 4096, 256, 1152


def _row(site, M, N, K, *, lda=None, a_col=0, w_rows=None, w_row=0, ldc=None, c_col=0, epi="bias", bias=True, res=None, r_mod=0,
         gates=None, c2=False, kind="bf16", kt=0, q8=False):
    """gates = (B, S, St, gate_bstride); res = "rows" (a residual of M rows) or None; kind bf16 | rows | mx | fp8"""
    return dict(site=site, M=M, N=N, K=K, lda=lda or K + a_col, a_col=a_col, w_rows=w_rows or N + w_row, w_row=w_row, ldc=ldc or N + c_col,
                c_col=c_col, epi=epi, bias=bias, res=res, r_mod=r_mod, gates=gates, c2=c2, kind=kind, kt=kt, q8=q8)


SITES = {
    # ---- CogVideoX-2B LoRA, micro-batch 4 (engine.py) ----
    "cog2b_qkv": _row("engine.py:block_forward qkv", CM, 3 * CD, CD + 64),
    "cog2b_attn_out": _row("engine.py:block_forward w_o", CM, CD, CD + 64, epi="gated", res="rows", gates=(CB, CS, CST, COG_BS), c2=True),
    "cog2b_ff1": _row("engine.py:block_forward w1", CM, 4 * CD, CD, epi="gelu", c2=True),
    "cog2b_ff2": _row("engine.py:block_forward w2", CM, CD, 4 * CD, epi="gated", res="rows", gates=(CB, CS, CST, COG_BS), c2=True),
    "cog2b_w2t_dgelu": _row("engine.py:run_backward w2_t", CM, 4 * CD, CD, epi="dgelu", bias=False),
    "cog2b_w1t": _row("engine.py:run_backward w1_t", CM, CD, 4 * CD, bias=False),
    "cog2b_wot": _row("engine.py:run_backward w_o_t", CM, CD + 64, CD, bias=False),
    "cog2b_wqkvt": _row("engine.py:run_backward w_qkv_t", CM, CD + 64, 3 * CD, bias=False),
    "cog2b_wqkvt_rows": _row("engine.py:run_backward w_qkv_t[d:] -> dx1[:, d:]", CM, 64, 3 * CD, w_rows=CD + 64, w_row=CD,
                             ldc=CD + 64, c_col=CD, bias=False),
    # ---- CogVideoX-5B feed-forward pair, micro-batch 2 (d = 3072) ----
    "cog5b_ff1": _row("engine.py:block_forward w1 (5B)", 2 * CS, 4 * 3072, 3072, epi="gelu", c2=True),
    "cog5b_ff2": _row("engine.py:block_forward w2 (5B)", 2 * CS, 3072, 4 * 3072, epi="gated", res="rows", gates=(2, CS, CST, 42 * 12 * 3072),
                      c2=True),
    # ---- HunyuanVideo bf16 mode (hunyuan.py), adapted image stream: K-extended qkv / proj ----
    "hy_img_qkv": _row("hunyuan.py:lora_linear img qkv", HLI, 3 * HD, HD + 64),
    "hy_img_proj": _row("hunyuan.py:glinear img proj", HLI, HD, HD + 64, epi="gated", res="rows", gates=(1, HLI, 0, 6 * HD), c2=True),
    "hy_img_fc1": _row("hunyuan.py:mlp fc1", HLI, HF, HD, epi="gelu", c2=True),
    "hy_img_fc2": _row("hunyuan.py:mlp fc2", HLI, HD, HF, epi="gated", res="rows", gates=(1, HLI, 0, 6 * HD), c2=True),
    "hy_img_fc2_dgrad": _row("hunyuan.py:mlp bwd fc2^T", HLI, HF, HD, epi="dgelu", bias=False),
    "hy_single_lin1_mlp": _row("hunyuan.py:single_block w1[3D:] -> cat[:, D:]", HLJ, HF, HD, w_rows=3 * HD + HF, w_row=3 * HD,
                               ldc=HD + HF, c_col=HD, epi="gelu", c2=True),
    "hy_single_lin2": _row("hunyuan.py:single_block linear2", HLJ, HD, HD + HF, epi="gated", res="rows", gates=(1, HLJ, 0, 3 * HD), c2=True),
    "hy_single_wt_rows": _row("hunyuan.py:single_block bwd _wt_rows", HLJ, HD, HF, lda=HD + HF, a_col=HD, epi="gated", res="rows",
                              bias=False),
    # ---- STDiT-XL/2 (stdit.py) ----
    "stdit_proj": _row("stdit.py:plinear attn.proj", SB * SRPS, SD, SD, epi="gated", res="rows", gates=(SB, SRPS, 0, 6 * SD), c2=True),
    "stdit_fc1": _row("stdit.py:mlp fc1", SB * SRPS, 4 * SD, SD, epi="gelu", c2=True),
    "stdit_fc2": _row("stdit.py:mlp fc2", SB * SRPS, SD, 4 * SD, epi="gated", res="rows", gates=(SB, SRPS, 0, 6 * SD), c2=True),
    "stdit_x_embedder": _row("stdit.py:forward x_embedder", SB * SRPS, SD, 64, epi="gated", res="rows", r_mod=SSP),
    # ---- VideoCrafter2 UNet (unet.py) ----
    "unet_l0_geglu": _row("unet.py:linear GEGLU proj (level 0)", 163840, 2560, 320),
    "unet_l1_linear": _row("unet.py:linear (level 1)", 40960, 640, 640),
    # ---- T5-XXL encoder (t5.py), 2 prompts x 226 tokens ----
    "t5_ff_wo": _row("t5.py:forward DenseReluDense.wo", 452, 4096, 10240, epi="gated", res="rows", bias=False),
    # ---- UNet 320-wide Linears through ops.linear_rows (vt_conv_cl as a 1x1 convolution) ----
    "unet_rows_ff_out": _row("unet.py:linear ff out (rows320)", 163840, 320, 1280, epi="gated", res="rows", kind="rows"),
    "unet_rows_geglu_dx": _row("unet.py:linear bwd GEGLU proj dx (rows320)", 163840, 320, 2560, bias=False, kind="rows"),
    # ---- HunyuanVideo fp8="mfma" (hunyuan.py mx_gemm / lora_linear) on vt_gemm_mxfp8 ----
    "mx_img_qkv_tail": _row("hunyuan.py:lora_linear img qkv (bf16 tail)", HLI, 3 * HD, HD, kind="mx", kt=64),
    "mx_img_fc1": _row("hunyuan.py:mlp fc1", HLI, HF, HD, epi="gelu", c2=True, kind="mx", q8=True),
    "mx_img_fc2": _row("hunyuan.py:mlp fc2", HLI, HD, HF, epi="gated", res="rows", gates=(1, HLI, 0, 6 * HD), c2=True, kind="mx"),
    "mx_single_lin1_qkv": _row("hunyuan.py:single_block linear1 rows [0, 3D)", HLJ, 3 * HD, HD, w_rows=3 * HD + HF, kind="mx"),
    "mx_single_lin1_mlp": _row("hunyuan.py:single_block linear1 rows [3D, 3D+F) -> cat[:, D:]", HLJ, HF, HD, w_rows=3 * HD + HF,
                               w_row=3 * HD, ldc=HD + HF, c_col=HD, epi="gelu", c2=True, kind="mx", q8=True),
    "mx_single_lin2": _row("hunyuan.py:single_block linear2", HLJ, HD, HD + HF, epi="gated", res="rows", gates=(1, HLJ, 0, 3 * HD), c2=True,
                           kind="mx"),
    # ---- HunyuanVideo fp8="matmul" qkv on vt_gemm_fp8 ----
    "fp8_img_qkv": _row("hunyuan.py:linear img qkv (fp8 matmul)", HLI, 3 * HD, HD, kind="fp8"),
}
BF16_ROWS = [k for k, r in SITES.items() if r["kind"] == "bf16"]
OTHER_ROWS = [k for k, r in SITES.items() if r["kind"] != "bf16"]


# ------------------------------------------------------------------ operands
def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _spread(n, g, dev, sigma, outliers=0, big=8.0):
    """per-channel scales exp(sigma z), a few outlier channels x big"""
    s = torch.exp(sigma * torch.randn(n, generator=g, device=dev))
    if outliers:
        s[torch.randperm(n, generator=g, device=dev)[:outliers]] *= big
    return s


def _operands(r, dev, seed):
    """A [M, lda] and W [w_rows, K] storage with per-row / per-column spread and outlier input channels, scaled so that the products
    (the pre-activations) spread over about [-6, 6]; bias, residual, gates, the saved pre-activation U over [-6, 6]"""
    g = _gen(dev, seed)
    M, N, K = r["M"], r["N"], r["K"]
    ca = _spread(K, g, dev, 0.3, outliers=max(2, K // 512))
    a = torch.randn(M, r["lda"], generator=g, device=dev)
    a[:, r["a_col"]:r["a_col"] + K] *= ca
    a *= _spread(M, g, dev, 0.35)[:, None]
    w = torch.randn(r["w_rows"], K, generator=g, device=dev) * (1.6 / math.sqrt(float((ca * ca).sum())))
    w *= _spread(r["w_rows"], g, dev, 0.35)[:, None]
    o = SimpleNamespace()
    o.A, o.W = a.to(BF), w.to(BF)
    del a, w
    o.a = o.A[:, r["a_col"]:r["a_col"] + K]
    o.w = o.W[r["w_row"]:r["w_row"] + N]
    o.bias = (torch.randn(N, generator=g, device=dev) * 0.5).to(BF) if r["bias"] else None
    o.R = None
    if r["res"]:
        o.R = torch.randn(r["r_mod"] or M, N, generator=g, device=dev).to(BF)
    o.U = (torch.randn(M, N, generator=g, device=dev) * 2.5).clamp(-7, 7).to(BF) if r["epi"] == "dgelu" else None
    o.gt = o.gv = None
    if r["gates"]:
        B, S, St, bs = r["gates"]
        tab = torch.randn(B, bs, generator=g, device=dev) * 0.4 + 0.9
        tab += torch.arange(B, device=dev, dtype=torch.float32)[:, None] * 0.35          # neighbouring samples' gates differ
        o.tab = tab
        o.gv = tab[:, 2 * N:]                                                         # video gate chunk (engine._mod: chunk 2)
        o.gt = tab[:, 5 * N:] if St > 0 else o.gv                                    # text gate chunk 5; single-segment models: one gate
        if St > 0:
            tab[:, 5 * N:6 * N] -= 0.6                                                # text and video gates differ
    return o


def _gate_rows(r, o, rows):
    """[len(rows), N] float64 gate of each row: sample b = m // S, text rows (m % S) < St"""
    B, S, St, bs = r["gates"]
    N = r["N"]
    b = rows // S
    txt = (rows % S) < St
    gt = o.gt[:, :N].double()[b]
    gv = o.gv[:, :N].double()[b]
    return torch.where(txt[:, None], gt, gv)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(K0 * (x + K1 * x ** 3)))


def _gelu_grad(x):
    t = torch.tanh(K0 * (x + K1 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * K0 * (1.0 + 3.0 * K1 * x * x)


def _ulp(x):
    """one bf16 ulp of each element (8 significant bits; normal range)"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 8)


# ------------------------------------------------------------------ the float64 reference and its bound
def _acc_coeff(r):
    """first-order rounding count of the fp32 value the epilogue sees, times the fp32 unit roundoff.  Each MFMA step adds a block of
    exact products (bf16 x bf16 and e4m3 x e4m3 are exact in fp32) into the fp32 accumulator: at most log2(depth) roundings inside the
    step (a pairwise sum; 5 for the 32-deep bf16 / fp8 steps, 7 for the 128-deep MX step) and one per step along the K chain, every one
    bounded by u times the sum of |products| reaching it.  Then: the scale product sa * sw and the scaling multiply (fp8: 2), the bf16
    tail's K chain and its 5 in-step roundings (MX, Kt = 64: 2 + 5), the bias add (1).  The bound is on |fp32 - exact| <= coeff * mag with
    mag = sum_k |a_k w_k| (+ |bias|)."""
    K, kind = r["K"], r["kind"]
    if kind == "mx":
        return (K // 128 + 7 + 2 + (r["kt"] // 32 + 5 if r["kt"] else 0) + 1) * U32
    if kind == "fp8":
        return (K // 32 + 5 + 2 + 1) * U32
    return (K // 32 + 5 + 1) * U32


def _blockmax(x):
    """max |x| over each 32-column block: [rows, K] -> [rows, K / 32]"""
    return x.abs().view(x.shape[0], -1, 32).amax(-1)


def _fp8_group_term(a_blk, w_blk):
    """the fp8 MFMAs (v_mfma_scale_f32_16x16x128_f8f6f4 and v_mfma_f32_16x16x32_fp8_fp8) do NOT sum a step's products like fp32 adds:
    inside a group of 16 consecutive k the products are aligned to the group's largest one and the small ones lose bits (measured:
    test_fp8_mfma_group_loss_model -- +2^16 - 2^16 plus 14 products of 2^-14 of the maximum come out 32 instead of 56; the bf16 MFMA keeps
    them).  Model, pinned by that test: one group loses at most FP8_GROUP_ERR x its largest |product|.  Both kernels feed each 32-byte
    block of a K row to one lane group / k-step, so a 32-block holds at most two hardware groups, each with a largest product
    <= max_block |a| x max_block |w|:  error <= 2 FP8_GROUP_ERR sum_blocks max|a| max|w|  (a float64 matmul of the block maxima)."""
    return 2 * FP8_GROUP_ERR * (a_blk @ w_blk.T)


def _bound(r, ref, mag, pre, gate=None, resid=None, U=None, acc=None, pre_e=None):
    """per-element bound on |kernel - float64 reference| for the main output:
      ulp    one bf16 ulp of the reference: the final rounding is <= 1/2 ulp of the fp32 value, which may sit in the next binade up
      pre_e  = _acc_coeff * mag: the fp32 pre-activation's error (above)
      GELU   |gelu'(pre)| pre_e + pre_e^2 (|gelu''| <= 0.8 < 2) + |pre| SIG_ERR + 2 u |out|: the sigmoid is 1 - rcp(exp2(w) + 1) with the
             hardware exp2 / rcp (1 ulp each, relative 2^-23): rcp(...) carries <= 2 * 2^-23 absolute, 1 - r adds 2^-24, and the
             <= 5 u relative error of w = x (c0 + c1 x^2) (two roundings, two rounded constants) moves s by s (1 - s) ln2 |w| 5u <= 0.53 * 5u:
             < 12 * 2^-24 < SIG_ERR = 2^-20 absolute on s, times |x|; then x * s and the bf16 store
      gated  |g| pre_e + 2 u (|r| + |g pre|): the gate multiply and the residual add in fp32
      dGELU  |gelu'(U)| acc_e + |acc| (1 + |U du2|) SIG_ERR + 2 u |out|: U is exact (bf16); gelu'(U) = s + U du2 s (1 - s),
             du2 = 2 k0 (1 + 3 k1 U^2), inherits the sigmoid's absolute error times (1 + |U du2|)"""
    if pre_e is None:
        pre_e = _acc_coeff(r) * mag
    tol = _ulp(ref)
    epi = r["epi"]
    if epi == "bias":
        tol += pre_e
        if resid is not None:                       # linear_rows: (acc + bias) + r
            tol += 2 * U32 * (resid.abs() + pre.abs())
    elif epi == "gelu":
        tol += (_gelu_grad(pre).abs() + pre_e) * pre_e + pre.abs() * SIG_ERR + 2 * U32 * ref.abs()
    elif epi == "gated":
        g = 1.0 if gate is None else gate.abs()
        tol += g * pre_e + 2 * U32 * (resid.abs() + (g * pre).abs())
    elif epi == "dgelu":
        du2 = 2 * K0 * (1 + 3 * K1 * U * U)
        tol += _gelu_grad(U).abs() * pre_e + acc.abs() * (1 + (U * du2).abs()) * SIG_ERR + 2 * U32 * ref.abs()
    return tol


def _reference(r, o, r0, r1, Wd, Wa):
    """float64 reference of rows [r0, r1): (main output, its bound, pre-activation, pre-activation bound)"""
    kind = r["kind"]
    extra = 0.0
    if kind in ("mx", "fp8"):
        a = o.aq[r0:r1].double() * o.sa64
        acc = a @ Wd.T
        mag = a.abs() @ Wa.T
        extra = _fp8_group_term(_blockmax(a), o.Wblk)
        if r["kt"]:
            at = o.At[r0:r1].double()
            acc += at @ o.Wtd.T
            mag += at.abs() @ o.Wtd.abs().T
        del a
    else:
        a = o.a[r0:r1].double()
        acc = a @ Wd.T
        mag = a.abs() @ Wa.T
        del a
    pre = acc
    if o.bias is not None:
        b = o.bias.double()
        pre = acc + b
        mag += b.abs()
    rows = torch.arange(r0, r1, device=acc.device)
    epi = r["epi"]
    gate = resid = U = None
    if epi == "bias":
        ref = pre
        if o.R is not None:
            resid = o.R[r0:r1].double()
            ref = pre + resid
    elif epi == "gelu":
        ref = _gelu(pre)
    elif epi == "gated":
        resid = o.R[rows % r["r_mod"]].double() if r["r_mod"] else o.R[r0:r1].double()
        if r["gates"]:
            gate = _gate_rows(r, o, rows)
            ref = resid + gate * pre
        else:
            ref = resid + pre
    else:
        U = o.U[r0:r1].double()
        ref = acc * _gelu_grad(U)
    pre_e = _acc_coeff(r) * mag + extra
    tol = _bound(r, ref, mag, pre, gate=gate, resid=resid, U=U, acc=acc, pre_e=pre_e)
    pre_tol = _ulp(pre) + pre_e
    return ref, tol, pre, pre_tol


class _Tally:
    """bad elements / worst |err| / bound and where, of one output over all row chunks"""

    def __init__(self, name, tile):
        self.name, self.tile = name, tile
        self.bad, self.worst, self.at = 0, 0.0, None

    def add(self, out, ref, tol, r0):
        err = (out.double() - ref).abs()
        ratio = err / tol
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)   # NaN: a sentinel never overwritten
        self.bad += int((ratio > 1.0).sum())
        i = int(torch.argmax(ratio))
        w = float(ratio.view(-1)[i])
        if self.at is None or w > self.worst:
            self.worst, self.at = w, (r0 + i // ref.shape[1], i % ref.shape[1])

    def msg(self):
        m, n = self.at
        tm, tn = self.tile
        return f"{self.name}: {self.bad} elements out of bound, worst |err| / bound {self.worst:.3g} at (row {m}, col {n}), output tile ({m // tm}, {n // tn})"


def _compare(r, o, outs, dev, Wd=None, Wa=None):
    """outs: list of (tally, main output view [M, N], pre-activation output view or None).  Chunked float64 comparison of all of them."""
    M, N = r["M"], r["N"]
    chunk = max(256, (1 << 26) // max(N, r["K"]) // 256 * 256)
    for r0 in range(0, M, chunk):
        r1 = min(M, r0 + chunk)
        ref, tol, pre, pre_tol = _reference(r, o, r0, r1, Wd, Wa)
        for t_out, out, t_pre, c2 in outs:
            t_out.add(out[r0:r1], ref, tol, r0)
            if c2 is not None:
                t_pre.add(c2[r0:r1], pre, pre_tol, r0)
        del ref, tol, pre, pre_tol
    for t_out, _, t_pre, c2 in outs:
        assert t_out.bad == 0, t_out.msg()
        if c2 is not None:
            assert t_pre.bad == 0, t_pre.msg()
    return [t[0].worst for t in outs]


# ------------------------------------------------------------------ guarded output buffers
GUARD_ROWS = 3


def _guarded(M, ld, dev, dtype=BF):
    return poisoned((M + GUARD_ROWS, ld), dtype, dev)          # SENT in every bf16 element, SENT8 in every fp8 byte


def _guards_intact(buf, M, c0, c1, what):
    """rows past M untouched; columns outside [c0, c1) of the first M rows untouched (in memory the columns right of row m's slice are
    followed by the left columns of row m + 1, so a slice that ends at ldc still has sentinels on both sides)"""
    bits = buf.view(torch.int16) if buf.dtype == BF else buf.view(torch.uint8)
    s = SENT if buf.dtype == BF else SENT8
    assert bool((bits[M:] == s).all()), f"{what}: a sentinel row past M = {M} was written"
    if c0 > 0:
        assert bool((bits[:M, :c0] == s).all()), f"{what}: a sentinel column left of the output slice was written"
    if c1 < buf.shape[1]:
        assert bool((bits[:M, c1:] == s).all()), f"{what}: a sentinel column right of the output slice was written"


def _same_bits(x, y):
    return bool(torch.equal(x.contiguous().view(torch.int16), y.contiguous().view(torch.int16)))


# ------------------------------------------------------------------ vt_gemm_bf16 rows
def _launch_bf16(r, o, C, C2, epi=None):
    from vt355 import ops
    e = {"bias": ops.EPI_BIAS, "gelu": ops.EPI_BIAS_GELU, "gated": ops.EPI_GATED_RES, "dgelu": ops.EPI_DGELU}[epi or r["epi"]]
    kw = {}
    if e == ops.EPI_GATED_RES:
        kw = dict(residual=o.R, r_mod=r["r_mod"])
        if r["gates"]:
            B, S, St, bs = r["gates"]
            assert o.tab.stride(0) == bs
            kw.update(gate_txt=o.gt, gate_vid=o.gv, gate_bstride=bs, S=S, St=St)
        kw["pre_act_out"] = C2
    elif e == ops.EPI_BIAS_GELU:
        kw["pre_act_out"] = C2
    elif e == ops.EPI_DGELU:
        kw["pre_act_in"] = o.U
    ops.gemm(o.a, o.w, C, o.bias, epilogue=e, K=r["K"], N=r["N"], **kw)


def _out_views(r, dev):
    M, N = r["M"], r["N"]
    Cb = _guarded(M, r["ldc"], dev)
    C = Cb[:M, r["c_col"]:r["c_col"] + N]
    C2b = _guarded(M, N, dev) if r["c2"] else None
    return Cb, C, C2b, (C2b[:M] if C2b is not None else None)


def _log(msg):
    print(msg, flush=True)


@pytest.mark.parametrize("name", BF16_ROWS)
def test_gemm_bf16_production_site(dev, name):
    from vt355 import ops
    r = SITES[name]
    M, N, K = r["M"], r["N"], r["K"]
    o = _operands(r, dev, seed=zlib.crc32(name.encode()) & 0xFFFF)
    kept = {}
    try:
        for mode in (1, 2, 3, 0):
            ops.gemm_set_tile(mode)
            Cb, C, C2b, C2 = _out_views(r, dev)
            _launch_bf16(r, o, C, C2)
            torch.cuda.synchronize()
            what = f"{name} tile mode {mode}"
            _guards_intact(Cb, M, r["c_col"], r["c_col"] + N, what)
            if C2b is not None:
                _guards_intact(C2b, M, 0, N, what + " C2")
            # 4. a second launch is bit-identical (guards included)
            Db, D, D2b, D2 = _out_views(r, dev)
            _launch_bf16(r, o, D, D2)
            assert _same_bits(Cb, Db), f"{what}: a second launch differs"
            if C2b is not None:
                assert _same_bits(C2b, D2b), f"{what}: a second launch differs in C2"
            del Db, D, D2b, D2
            # 2. the second output is the EPI_BIAS result of the same tiling, bit for bit
            if C2 is not None:
                Eb, E, _, _ = _out_views(r, dev)
                _launch_bf16(r, o, E, None, epi="bias")
                assert _same_bits(C2, E), f"{what}: C2 differs from the EPI_BIAS output of the same tiling"
                del Eb, E
            kept[mode] = (Cb, C, C2b, C2)
        # 5. the default is bit-identical to the tiling the dispatcher reports
        ops.gemm_set_tile(0)
        kdef = ops.gemm_kernel(M, N, K)
        fmode = 3 if kdef == 4 else kdef
        assert _same_bits(kept[0][0], kept[fmode][0]), f"{name}: the default launch differs from forced tiling {fmode}"
        if kept[0][2] is not None:
            assert _same_bits(kept[0][2], kept[fmode][2]), f"{name}: the default launch's C2 differs from forced tiling {fmode}"
        del kept[0]
    finally:
        ops.gemm_set_tile(0)
    # 1. every element of every forced tiling against float64
    ks = {1: 1, 2: 2, 3: 4 if M <= 1024 else 3}
    Wd = o.w.double()
    Wa = Wd.abs()
    outs = []
    for mode, (Cb, C, C2b, C2) in kept.items():
        nm = f"{name} [{KNAME[ks[mode]]}]"
        outs.append((_Tally(nm, TILE[ks[mode]]), C, _Tally(nm + " C2", TILE[ks[mode]]), C2))
    worst = _compare(r, o, outs, dev, Wd, Wa)
    _log(f"[gemm site] {name:20s} {r['site']:48s} M={M} N={N} K={K} epi={r['epi']:5s} default={KNAME[kdef]:11s} "
         f"worst err/bound " + " ".join(f"{KNAME[ks[m]]}:{w:.3f}" for m, w in zip(kept, worst)))


def test_default_dispatch_covers_every_bf16_kernel():
    """over the table, the default dispatch reaches the 128x128 kernel, the 256x256 kernel and both producer / consumer instantiations:
    if the heuristics move, the table must follow so that every kernel the library ships stays tested at production shapes"""
    from vt355 import ops
    ops.gemm_set_tile(0)
    got = {}
    for name in BF16_ROWS:
        r = SITES[name]
        got.setdefault(ops.gemm_kernel(r["M"], r["N"], r["K"]), []).append(name)
    for k, names in sorted(got.items()):
        _log(f"[gemm dispatch] {KNAME[k]:11s}: {', '.join(names)}")
    assert set(got) == {1, 2, 3, 4}, f"the default dispatch over the table reaches only {sorted(got)}"


# ------------------------------------------------------------------ linear_rows, MX-fp8, fp8 rows
def _quant(x, amax_frac=1.0):
    """e4m3 copy of fp32 x with a per-tensor scale (amax / 448); returns (xq, scale fp32 [1])"""
    s = (x.abs().max() / 448.0 * amax_frac).reshape(1).float()
    return (x / s).clamp(-448, 448).to(F8), s


def _e4m3_cpu(x_bf16, scale):
    """satfinite(RNE(x / scale)) on the host (IEEE division)"""
    return (x_bf16.float().cpu() / scale.float().cpu()).clamp(-448.0, 448.0).to(F8)


@pytest.mark.parametrize("name", OTHER_ROWS)
def test_gemm_other_production_site(dev, name):
    from vt355 import ops
    r = SITES[name]
    M, N, K = r["M"], r["N"], r["K"]
    o = _operands(r, dev, seed=zlib.crc32(name.encode()) & 0xFFFF)
    kind = r["kind"]
    Wd = Wa = None
    if kind in ("mx", "fp8"):
        o.aq, o.sa = _quant(o.a.float())
        o.Wq, o.sw = _quant(o.W.float())
        o.wq = o.Wq[r["w_row"]:r["w_row"] + N]
        o.sa64 = float(o.sa)
        Wd = o.wq.double() * float(o.sw)
        Wa = Wd.abs()
        o.Wblk = _blockmax(Wd)
        if r["kt"]:                                  # the adapted Linear's extension columns, bf16: xe[:, D:] and wext[:, D:]
            g = _gen(dev, 99)
            xe = torch.randn(M, K + r["kt"], generator=g, device=dev).to(BF)
            wext = (torch.randn(N, K + r["kt"], generator=g, device=dev) * 0.05).to(BF)
            o.At, o.Wt = xe[:, K:], wext[:, K:]
            o.Wtd = o.Wt.double()
        else:
            o.At = o.Wt = None
        del o.A, o.W, o.a, o.w
    else:
        Wd = o.w.double()
        Wa = Wd.abs()
    cq_args = None

    def launch():
        Cb, C, C2b, C2 = _out_views(r, dev)
        Qb = None
        if kind == "rows":
            assert r["epi"] in ("bias", "gated") and r["gates"] is None
            ops.linear_rows(o.a, o.w, C, o.bias, o.R)
        elif kind == "fp8":
            ops.gemm_fp8(o.aq, o.wq, C, o.sa, o.sw, o.bias)
        else:
            e = {"bias": ops.EPI_BIAS, "gelu": ops.EPI_BIAS_GELU, "gated": ops.EPI_GATED_RES}[r["epi"]]
            kw = dict(epilogue=e, pre_act_out=C2)
            if e == ops.EPI_GATED_RES:
                B, S, St, bs = r["gates"]
                kw.update(residual=o.R, gate_txt=o.gt, gate_vid=o.gv, gate_bstride=bs, S=S, St=St)
            if r["kt"]:
                kw["tail"] = (o.At, o.Wt)
            if r["q8"]:
                Qb = _guarded(M, r["ldc"], dev, dtype=F8)
                kw["out_fp8"] = (Qb[:M, r["c_col"]:r["c_col"] + N], cq_args[0], cq_args[1])
            ops.gemm_mxfp8(o.aq, o.wq, C, o.sa, o.sw, o.bias, **kw)
        torch.cuda.synchronize()
        return Cb, C, C2b, C2, Qb

    if r["q8"]:
        cq_args = (torch.tensor([0.0123], device=dev), torch.zeros(1, device=dev))
    Cb, C, C2b, C2, Qb = launch()
    _guards_intact(Cb, M, r["c_col"], r["c_col"] + N, name)
    if C2b is not None:
        _guards_intact(C2b, M, 0, N, name + " C2")
    if r["q8"]:
        _guards_intact(Qb, M, r["c_col"], r["c_col"] + N, name + " fp8 copy")
        Cq = Qb[:M, r["c_col"]:r["c_col"] + N]
        assert torch.equal(Cq.cpu().view(torch.uint8), _e4m3_cpu(C, cq_args[0]).view(torch.uint8)), f"{name}: fp8 copy != cast of the bf16 output"
        assert cq_args[1].item() == C.float().abs().max().item(), f"{name}: amax != max |out|"
        assert (C.float().abs() > 448 * 0.0123).any()          # some values saturate
        amax1 = cq_args[1].item()
        cq_args[1].zero_()
    # 4. determinism (the fp8 copy and the amax too)
    Db, _, D2b, _, Qd = launch()
    assert _same_bits(Cb, Db), f"{name}: a second launch differs"
    if C2b is not None:
        assert _same_bits(C2b, D2b), f"{name}: a second launch differs in C2"
    if r["q8"]:
        assert torch.equal(Qb.view(torch.uint8), Qd.view(torch.uint8)) and cq_args[1].item() == amax1
    del Db, D2b, Qd
    outs = [(_Tally(name, (128, 128)), C, _Tally(name + " C2", (128, 128)), C2)]
    worst = _compare(r, o, outs, dev, Wd, Wa)
    extra = ""
    if kind == "rows":
        # ops.linear_rows' docstring: bit-identical to vt_gemm_bf16 (same products, same fp32 sums, (acc + bias) + residual)
        same = []
        try:
            for mode in (0, 1, 2, 3):
                ops.gemm_set_tile(mode)
                Gb, G, _, _ = _out_views(r, dev)
                if o.R is not None:
                    ops.gemm(o.a, o.w, G, o.bias, epilogue=ops.EPI_GATED_RES, residual=o.R)
                else:
                    ops.gemm(o.a, o.w, G, o.bias)
                same.append(_same_bits(G, C))
                del Gb, G
        finally:
            ops.gemm_set_tile(0)
        assert all(same), f"{name}: linear_rows is not bit-identical to vt_gemm_bf16 under tile modes {[m for m, s in zip((0, 1, 2, 3), same) if not s]}"
        extra = " (bit-identical to vt_gemm_bf16 under every tiling)"
    _log(f"[gemm site] {name:20s} {r['site']:48s} M={M} N={N} K={K} epi={r['epi']:5s} {kind} worst err/bound {worst[0]:.3f}{extra}")


# ------------------------------------------------------------------ the comparator rejects what it must
def _pc_tile_of(id_, M, N, bm=256, bn=128, gm=4):
    """(row0, col0) of work item id_ of the producer / consumer kernel (gemm_pc_bf16.hip gp_tile: grouped ordering)"""
    nbm, nbn = (M + bm - 1) // bm, (N + bn - 1) // bn
    in_group = gm * nbn
    first_m = (id_ // in_group) * gm
    gsz = min(nbm - first_m, gm)
    return (first_m + (id_ % in_group) % gsz) * bm, ((id_ % in_group) // gsz) * bn


def test_comparator_rejects_wrong_tiles(dev):
    """CogVideoX ff2 (71 104 x 1920 x 7680, gated, the 256x128 producer / consumer kernel): the comparator must reject
    (a) one 16x16 block of a tile that a workgroup runs as its SECOND tile, scaled by 1 + 2^-5;
    (b) two adjacent rows swapped inside one 32-row epilogue slab;
    (c) the gate of sample b + 1 applied to the last rows of sample b in the tile that straddles the boundary;
    and the device float64 reference must agree with float64 numpy on the host on 64 sampled rows."""
    from vt355 import ops
    name = "cog2b_ff2"
    r = SITES[name]
    M, N = r["M"], r["N"]
    o = _operands(r, dev, seed=zlib.crc32(name.encode()) & 0xFFFF)
    ops.gemm_set_tile(0)
    assert ops.gemm_kernel(M, N, r["K"]) == 3
    Cb, C, C2b, C2 = _out_views(r, dev)
    _launch_bf16(r, o, C, C2)
    torch.cuda.synchronize()
    Wd = o.w.double()
    Wa = Wd.abs()

    def rejects(out, r0, r1):
        ref, tol, _, _ = _reference(r, o, r0, r1, Wd, Wa)
        t = _Tally("selfcheck", TILE[3])
        t.add(out[r0:r1], ref, tol, r0)
        return t.bad

    # the unmodified output passes on the windows used below
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    slots = cus // 8 * 8 if cus >= 8 else 8
    row0, col0 = _pc_tile_of(slots + 37, M, N)
    S = r["gates"][1]
    b_row0 = (S // 256) * 256                     # the 256-row tile that holds the first boundary (rows S - 1 | S)
    assert b_row0 < S < b_row0 + 256
    assert rejects(C, row0, row0 + 256) == 0 and rejects(C, b_row0, b_row0 + 256) == 0
    # (a) one 16x16 block, 1 + 2^-5
    bad = C.clone()
    blk = bad[row0 + 48:row0 + 64, col0 + 32:col0 + 48]
    blk.copy_((blk.double() * (1 + 2.0 ** -5)).to(BF))
    assert rejects(bad, row0, row0 + 256) > 0, "a 1 + 2^-5 error in one 16x16 block passed"
    # (b) rows 5 and 6 of the third 32-row slab swapped
    bad = C.clone()
    i = row0 + 64 + 5
    bad[[i, i + 1]] = C[[i + 1, i]]
    assert rejects(bad, row0, row0 + 256) > 0, "two swapped rows passed"
    # (c) sample 1's gate on the last 8 rows of sample 0 (row S - 1 is a video row of sample 0)
    bad = C.clone()
    acc = o.a[S - 8:S].double() @ Wd.T + o.bias.double()
    B_, S_, St_, _ = r["gates"]
    wrong = o.R[S - 8:S].double() + o.gv[1, :N].double() * acc
    bad[S - 8:S] = wrong.to(BF)
    assert rejects(bad, b_row0, b_row0 + 256) > 0, "the neighbouring sample's gate passed"
    # the device float64 reference vs numpy float64 on 64 sampled rows
    g = torch.Generator().manual_seed(5)
    pick = torch.randperm(M, generator=g)[:64].sort().values
    ref_rows = []
    for m in pick.tolist():
        ref, _, _, _ = _reference(r, o, m, m + 1, Wd, Wa)
        ref_rows.append(ref[0].cpu().numpy())
    a = o.a[pick.to(dev)].double().cpu().numpy()
    w = o.w.double().cpu().numpy()
    pre = a @ w.T + o.bias.double().cpu().numpy()
    pk = pick.numpy()
    b = pk // S_
    txt = (pk % S_) < St_
    gt = o.gt[:, :N].double().cpu().numpy()[b]
    gv = o.gv[:, :N].double().cpu().numpy()[b]
    want = o.R.double().cpu().numpy()[pk] + np.where(txt[:, None], gt, gv) * pre
    got = np.stack(ref_rows)
    mag = np.abs(a) @ np.abs(w.T)
    assert np.all(np.abs(got - want) <= 1e-12 * (mag + np.abs(want) + 1.0)), np.max(np.abs(got - want))


@pytest.mark.parametrize("kind", ["mx", "fp8", "bf16"])
def test_fp8_mfma_group_loss_model(dev, kind):
    """the in-instruction product-group loss that _fp8_group_term assumes: k = 0, 1 hold +2^16 and -2^16, n of k = 2 .. 15 hold 2^j
    (every value exact in e4m3 and bf16, every partial sum exact in fp32), the other k zero.  The fp8 MFMAs may lose at most
    FP8_GROUP_ERR x 2^16 of the small products' sum (measured: 14 x 2^2 -> 32); the bf16 MFMA loses at most one fp32 unit of 2^16 per
    product.  The same products in another 16-group (k = 16 ..) than the large pair are summed exactly by all three."""
    from vt355 import ops
    M = N = 128
    K = 256
    one = torch.ones(1, device=dev)
    worst = 0.0
    for j in range(-14, 9):
        for n in (1, 7, 14):
            for lo in (2, 16):
                a = torch.zeros(M, K, device=dev)
                w = torch.zeros(N, K, device=dev)
                a[:, 0] = a[:, 1] = 256.0
                w[:, 0], w[:, 1] = 256.0, -256.0
                a[:, lo:lo + n] = 2.0 ** (j // 2)
                w[:, lo:lo + n] = 2.0 ** (j - j // 2)
                want = n * 2.0 ** j
                out = torch.zeros(M, N, dtype=BF, device=dev)
                if kind == "mx":
                    ops.gemm_mxfp8(a.to(F8), w.to(F8), out, one, one)
                elif kind == "fp8":
                    ops.gemm_fp8(a.to(F8), w.to(F8), out, one, one)
                else:
                    ops.gemm(a.to(BF), w.to(BF), out)
                got = out.double()
                assert bool((got == got[0, 0]).all())
                loss = abs(float(got[0, 0]) - want) - float(_ulp(torch.tensor(want, dtype=F64)))    # the bf16 store: < 1 ulp
                limit = FP8_GROUP_ERR * 2.0 ** 16 if kind != "bf16" else n * 2.0 ** 16 * U32 * 2
                if lo == 16:
                    limit = 0.0
                assert loss <= limit, f"{kind}: +-2^16 and {n} x 2^{j} at k = {lo}: got {float(got[0, 0])}, want {want}"
                worst = max(worst, loss / 2.0 ** 16)
    _log(f"[fp8 group model] {kind}: worst loss / largest product {worst:.3g} (model {FP8_GROUP_ERR if kind != 'bf16' else 'fp32 units'})")
