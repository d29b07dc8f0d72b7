"""Thin tensor-level wrappers over the C-ABI (include/vt355.h).

PyTorch is used here for device memory and streams only: every wrapper turns tensors into raw
pointers / leading dimensions and launches the HIP kernel on torch's current stream.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from ._lib import check, load_library

BF16 = torch.bfloat16
EPI_BIAS, EPI_BIAS_GELU, EPI_GATED_RES, EPI_DGELU = 0, 1, 2, 3


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-kernel timing with HIP events recorded on the stream the kernels are launched on ----
_PROFILE = {"on": False, "events": {}, "work": {}}
_PROFILED = ("attn_fwd", "attn_bwd", "conv", "conv_dw")


def profile_reset(on: bool):
    """on: start a fresh measurement; off: stop recording (what was collected stays readable until the next start)"""
    _PROFILE["on"] = on
    if on:
        _PROFILE["events"] = {}
        _PROFILE["work"] = {}


def profile_work():
    """name -> algorithmic work (FLOPs) summed over the timed launches (kernels that report it: the UNet convolutions)"""
    return dict(_PROFILE["work"])


def profile_collect():
    """name -> (average ms per launch, launches); call after a stream synchronize."""
    out = {}
    for name, evs in _PROFILE["events"].items():
        ts = [a.elapsed_time(b) for a, b in evs]
        out[name] = (sum(ts) / len(ts), len(ts))
    return out


class _timed:
    def __init__(self, name, work: float = 0.0):
        self.name = name
        self.work = work

    def __enter__(self):
        if _PROFILE["on"]:
            if self.work:
                _PROFILE["work"][self.name] = _PROFILE["work"].get(self.name, 0.0) + self.work
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream())

    def __exit__(self, *exc):
        if _PROFILE["on"]:
            b = torch.cuda.Event(enable_timing=True)
            b.record(torch.cuda.current_stream())
            _PROFILE["events"].setdefault(self.name, []).append((self.a, b))


def _timed_hbm(name, rows, nbytes):
    """memory-bound kernels at the benchmark's row counts: work = algorithmic HBM bytes (bench.py turns it into GB/s)"""
    return _timed(name, nbytes) if (_PROFILE["on"] and rows >= 4096) else _NOTIME


class _NoTime:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NOTIME = _NoTime()


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str, ndim: Optional[int] = None):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor (the vt355 ops have no CPU path)")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim}-d, got shape {tuple(t.shape)}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost stride must be 1")


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.dim() == 2 else t.stride(-2)


# The glue kernels take their extents from ONE operand and trust the others to be at least as large; the checks below refuse, before
# any launch, an operand smaller than what the launch will touch (a short output is written past its end otherwise).
def _rows_cols(t: torch.Tensor, rows: int, cols: int, name: str, fn: str):
    if t.shape[0] < rows or t.shape[1] < cols:
        raise ValueError(f"{fn}: {name} {tuple(t.shape)} is smaller than the [{rows}, {cols}] the launch touches")


def _numel(t: Optional[torch.Tensor], n: int, name: str, fn: str):
    if t is not None and t.numel() < n:
        raise ValueError(f"{fn}: {name} holds {t.numel()} elements, the launch touches {n}")


def _span(t: torch.Tensor) -> int:
    """elements from t's first to its last, in memory"""
    return 0 if t.numel() == 0 else 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))


def _loss_operands(fn, vpred, noisy, x0, sa, sb, w, dvpred):
    n, B = x0.numel(), x0.shape[0]
    _numel(vpred, n, "vpred", fn); _numel(noisy, n, "noisy", fn); _numel(dvpred, n, "dvpred", fn)
    _numel(sa, B, "sa", fn); _numel(sb, B, "sb", fn); _numel(w, B, "w", fn)


def _patch_rows(img, tok, P: int, fn: str):
    B, F, C, H, W = img.shape
    if P > 0 and H % P == 0 and W % P == 0 and tok.shape[0] != B * F * (H // P) * (W // P):      # the library refuses any other P
        raise ValueError(f"{fn}: tok has {tok.shape[0]} rows, img {tuple(img.shape)} at P={P} has {B * F * (H // P) * (W // P)} tokens")


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
         epilogue: int = EPI_BIAS, residual: Optional[torch.Tensor] = None, r_mod: int = 0,
         gate_txt: Optional[torch.Tensor] = None, gate_vid: Optional[torch.Tensor] = None, gate_bstride: int = 0,
         S: int = 1, St: int = 0, pre_act_out: Optional[torch.Tensor] = None,
         pre_act_in: Optional[torch.Tensor] = None, K: Optional[int] = None, N: Optional[int] = None, tile: int = 0) -> torch.Tensor:
    """out[M,N] = a[M,K] @ w[N,K]^T (+ epilogue).  a, w are 2-d (row-strided views allowed).  tile: 0 = the library chooses by shape,
    1 / 2 / 3 = that kernel as under gemm_set_tile (same bits, a caller that knows its shape; a global gemm_set_tile mode wins)."""
    _req(a, BF16, "a", 2); _req(w, BF16, "w", 2)
    M = a.shape[0]
    K = a.shape[1] if K is None else K
    N = w.shape[0] if N is None else N
    out_f32 = out.dtype == torch.float32
    if not out_f32:
        _req(out, BF16, "out", 2)
    lib = load_library()
    with _timed("gemm", 2.0 * M * N * K if (_PROFILE["on"] and M >= 4096) else 0.0) if (_PROFILE["on"] and M >= 4096) else _NOTIME:
        check(lib.vt_gemm_bf16_tile(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0),
                                    M, N, K, _p(bias), epilogue, int(out_f32),
                                    _p(residual), 0 if residual is None else residual.stride(0), r_mod,
                                    _p(gate_txt), _p(gate_vid), gate_bstride, S, St,
                                    _p(pre_act_out), 0 if pre_act_out is None else pre_act_out.stride(0),
                                    _p(pre_act_in), 0 if pre_act_in is None else pre_act_in.stride(0), tile, _stream()),
              "vt_gemm_bf16")
    return out


def gemm_nt(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, P: Optional[int] = None, Q: Optional[int] = None,
            alpha: float = 1.0, accumulate: bool = True, row_unpad=None, col_unpad=None):
    """c[P,Q] (+)= alpha * a[:, :P]^T @ b[:, :Q]  (reduction over the rows; c is fp32).  row_unpad = (group, keep): of every `group` result rows
    the first `keep` are stored, packed (c has P / group * keep rows); col_unpad likewise -- the gradient of a weight with padded heads."""
    _req(a, BF16, "a", 2); _req(b, BF16, "b", 2); _req(c, torch.float32, "c", 2)
    P = a.shape[1] if P is None else P
    Q = b.shape[1] if Q is None else Q
    if row_unpad is None and col_unpad is None:
        check(load_library().vt_gemm_nt_bf16(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
                                             a.shape[0], P, Q, alpha, int(accumulate), _stream()), "vt_gemm_nt_bf16")
        return
    rg, rk = row_unpad or (0, 0)
    cg, ck = col_unpad or (0, 0)
    rows, cols = (P // rg * rk if rg else P), (Q // cg * ck if cg else Q)
    if c.shape[0] != rows or c.shape[1] < cols:
        raise ValueError(f"gemm_nt: un-padded result is [{rows}, {cols}], c is {tuple(c.shape)}")
    check(load_library().vt_gemm_nt_bf16_unpad(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
                                               a.shape[0], P, Q, alpha, int(accumulate), rg, rk, cg, ck, _stream()), "vt_gemm_nt_bf16_unpad")


def group_colsum(x, out1, y=None, out2=None, mean=None, rstd=None, D: Optional[int] = None, S: int = 1, St: int = 0,
                 grouped: bool = False, o_bstride: Optional[int] = None, o_segstride: Optional[int] = None):
    """out1 += column sums of x; out2 += column sums of x*y (y normalised with mean/rstd when given).  grouped: the sums of
    (sample b, seg) land at out + b*o_bstride + seg*o_segstride (defaults: a dense [2B, D] array, text row first)."""
    _req(x, BF16, "x", 2)
    D = x.shape[1] if D is None else D
    ob = 2 * D if o_bstride is None else o_bstride
    osg = D if o_segstride is None else o_segstride
    check(load_library().vt_group_colsum(x.data_ptr(), x.stride(0), _p(y), 0 if y is None else y.stride(0), _p(mean), _p(rstd),
                                         _p(out1), _p(out2), x.shape[0], D, S, St, int(grouped), ob, osg, _stream()),
          "vt_group_colsum")


def _rope_args(rope, M: int):
    """rope = None or (cos, sin, S, St): fp32 [S-St, 64] tables for the video rows of every sample"""
    if rope is None:
        return None, None, 0, 0
    cos, sin, S, St = rope
    for t in (cos, sin):
        _req(t, torch.float32, "rope table", 2)
        if tuple(t.shape) != (S - St, 64) or not t.is_contiguous():
            raise ValueError(f"rope table must be contiguous [{S - St}, 64], got {tuple(t.shape)}")
    if M % S:
        raise ValueError(f"rows {M} not a multiple of the sequence length {S}")
    return cos.data_ptr(), sin.data_ptr(), S, St


def qk_ln_param_grads(dq_hat_f32, dk_hat, qkv, mean, rstd, out, H: int, rope=None):
    rc, rsn, S, St = _rope_args(rope, qkv.shape[0])
    check(load_library().vt_qk_ln_param_grads(dq_hat_f32.data_ptr(), dq_hat_f32.stride(0), dk_hat.data_ptr(), dk_hat.stride(0),
                                              qkv.data_ptr(), qkv.stride(0), mean.data_ptr(), rstd.data_ptr(), out.data_ptr(),
                                              qkv.shape[0], H, rc, rsn, S, St, _stream()), "vt_qk_ln_param_grads")


def ln_param_combine(G1, G2, D: int, gamma, beta, scales, dgamma, dbeta, dmods, grouped: bool):
    """scales: None or (scale_txt, scale_vid, bstride); dmods: None or (dshift_txt, dshift_vid, dscale_txt, dscale_vid, bstride)."""
    sc = (None, None, 0) if scales is None else scales
    dm = (None, None, None, None, 0) if dmods is None else dmods
    check(load_library().vt_ln_param_combine(G1.data_ptr(), G2.data_ptr(), G1.shape[0], D, _p(gamma), _p(beta), _p(sc[0]), _p(sc[1]),
                                             sc[2], _p(dgamma), _p(dbeta), _p(dm[0]), _p(dm[1]), _p(dm[2]), _p(dm[3]), dm[4],
                                             int(grouped), _stream()), "vt_ln_param_combine")


def small_linear_bwd(dy_f32, x, W, dW, db, dx):
    """dy [Bn,N] fp32, x [Bn,K] bf16, W [N,K] bf16; dW [N,K] / db [N] / dx [Bn,K] fp32 accumulated (any may be None)."""
    Bn, N = dy_f32.shape
    K = W.shape[1]
    check(load_library().vt_small_linear_bwd(dy_f32.data_ptr(), dy_f32.stride(0), x.data_ptr(), x.stride(0), W.data_ptr(), _p(dW),
                                             _p(db), _p(dx), 0 if dx is None else dx.stride(0), Bn, N, K, _stream()),
          "vt_small_linear_bwd")


def silu_bwd(dy_f32, x_pre, dx_f32):
    check(load_library().vt_silu_bwd(dy_f32.data_ptr(), x_pre.data_ptr(), dx_f32.data_ptr(), dy_f32.numel(), _stream()), "vt_silu_bwd")


def attn_fwd(q, k, v, o, lse2, B: int, H: int, S: int, scale: Optional[float] = None, q_prescaled: bool = False, tiles16: bool = False):
    """q,k,v,o: views whose element (b,s,h,d) is at base + b*bs + s*rs + h*64 + d; given as 3-d [B,S,>=H*64].
    tiles16 (with q_prescaled): the 16x16x32-MFMA variant of the kernel (same results; measured slower inside the training step, kept tested)"""
    if tiles16 and not q_prescaled:
        raise ValueError("the 16x16x32 forward exists for pre-scaled q only")
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        _req(t, BF16, n, 3)
    scale = 1.0 / math.sqrt(64) if scale is None else scale
    lib = load_library()
    with _timed("attn_fwd"):
      check(lib.vt_attn_fwd_hd64(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse2.data_ptr(), B, H, S,
                               q.stride(1), k.stride(1), v.stride(1), o.stride(1),
                               q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, 2 if tiles16 else int(q_prescaled), _stream()),
          "vt_attn_fwd_hd64")


def attn_fwd_bias(q, k, v, bias_t, o, lse2, B: int, H: int, S: int, scale: float = 1.0):
    """softmax(q k^T * scale + bias) v; bias_t fp32 [H, S(keys), S(queries)] contiguous, shared by all samples (T5)."""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        _req(t, BF16, n, 3)
    _req(bias_t, torch.float32, "bias_t", 3)
    if tuple(bias_t.shape) != (H, S, S) or not bias_t.is_contiguous():
        raise ValueError(f"bias_t must be contiguous [{H}, {S}, {S}], got {tuple(bias_t.shape)}")
    check(load_library().vt_attn_fwd_bias_hd64(q.data_ptr(), k.data_ptr(), v.data_ptr(), bias_t.data_ptr(), o.data_ptr(),
                                               lse2.data_ptr(), B, H, S, q.stride(1), k.stride(1), v.stride(1), o.stride(1),
                                               q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, _stream()),
          "vt_attn_fwd_bias_hd64")


def gemm_splitk(a, w, acc, splits: int = 0):
    """acc[M,N] (fp32, overwritten) = a[M,K] @ w[N,K]^T with the K range split over the chip (few rows, large weight)"""
    _req(a, BF16, "a", 2); _req(w, BF16, "w", 2); _req(acc, torch.float32, "acc", 2)
    check(load_library().vt_gemm_splitk_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), acc.data_ptr(), acc.stride(0),
                                            a.shape[0], w.shape[0], a.shape[1], splits, _stream()), "vt_gemm_splitk_f32")


def residual_cast(acc, residual, out):
    """out = bf16(acc + residual) (residual may be None)"""
    _req(acc, torch.float32, "acc", 2); _req(out, BF16, "out", 2)
    if residual is not None:
        _req(residual, BF16, "residual", 2)
    check(load_library().vt_residual_cast_bf16(acc.data_ptr(), acc.stride(0), _p(residual), 0 if residual is None else residual.stride(0),
                                               out.data_ptr(), out.stride(0), acc.shape[0], acc.shape[1], _stream()), "vt_residual_cast_bf16")


def groupnorm_silu(x, gamma, beta, y, groups: int = 32, eps: float = 1e-6, silu: bool = True, ws: Optional[torch.Tensor] = None):
    """channels-last GroupNorm (+ SiLU): x, y bf16 [N, P, C] (position stride = stride(1)); gamma / beta bf16 [C] or None"""
    _req(x, BF16, "x", 3); _req(y, BF16, "y", 3)
    N, P, C = x.shape
    if x.stride(0) != P * x.stride(1) or y.stride(0) != P * y.stride(1):
        raise ValueError("x / y: samples must be P positions apart")
    lib = load_library()
    need = int(lib.vt_groupnorm_ws_bytes(N, C))
    if ws is None:
        ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    check(lib.vt_groupnorm_silu_cl(x.data_ptr(), x.stride(1), _p(gamma), _p(beta), y.data_ptr(), y.stride(1), N, P, C, groups, eps,
                                   int(silu), ws.data_ptr(), ws.numel() * 4, _stream()), "vt_groupnorm_silu_cl")
    return y


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """torch Conv3d weight [Cout, Cin, 3, 3, 3] (or Conv2d [Cout, Cin, 3, 3]) -> [Cout, taps * Cin], tap-major with the input
    channel innermost: the layout vt_causal_conv3d_cl / vt_downsample_conv2d_cl read"""
    if w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3):
        return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1).contiguous()
    if w.dim() == 4 and tuple(w.shape[2:]) == (3, 3):
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()
    raise ValueError(f"expected a [Cout, Cin, 3, 3, 3] or [Cout, Cin, 3, 3] weight, got {tuple(w.shape)}")


pack_conv3d_weight = pack_conv_weight


def _cl_check(t, nm):
    ld = t.stride(3)
    N, T, H, W, _ = t.shape
    if t.stride(2) != W * ld or t.stride(1) != H * W * ld or t.stride(0) != T * H * W * ld:
        raise ValueError(f"{nm}: positions must be uniformly strided (channels-last, only the channel axis may be a slice)")


def causal_conv3d(x, wk, bias, y, residual=None):
    """x bf16 [N,T,H,W,Cin] channels-last, wk = pack_conv_weight(weight) bf16, bias bf16 [Cout] or None, y bf16 [N,T,H,W,Cout];
    residual (optional, like y) is added to the result"""
    _req(x, BF16, "x", 5); _req(y, BF16, "y", 5); _req(wk, BF16, "wk", 2)
    N, T, H, W, Cin = x.shape
    Cout = y.shape[4]
    if tuple(y.shape[:4]) != (N, T, H, W) or tuple(wk.shape) != (Cout, 27 * Cin) or not wk.is_contiguous():
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} wk {tuple(wk.shape)} y {tuple(y.shape)}")
    _cl_check(x, "x"); _cl_check(y, "y")
    if residual is not None:
        _req(residual, BF16, "residual", 5); _cl_check(residual, "residual")
        if tuple(residual.shape) != tuple(y.shape):
            raise ValueError("residual must have the shape of y")
    check(load_library().vt_causal_conv3d_cl(x.data_ptr(), x.stride(3), wk.data_ptr(), _p(bias), _p(residual),
                                             0 if residual is None else residual.stride(3), y.data_ptr(), y.stride(3),
                                             N, T, H, W, Cin, Cout, _stream()), "vt_causal_conv3d_cl")
    return y


def pack_conv_in8_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv3d weight [Cout, Cin <= 8, 3, 3, 3] -> [Cout, 32 * 8]: (tap, channel), taps 27..31 and channels >= Cin zero"""
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3) or w.shape[1] > 8:
        raise ValueError(f"expected a [Cout, Cin<=8, 3, 3, 3] weight, got {tuple(w.shape)}")
    out = torch.zeros(w.shape[0], 32, 8, dtype=w.dtype, device=w.device)
    out[:, :27, :w.shape[1]] = w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], 27, w.shape[1])
    return out.reshape(w.shape[0], 256)


def causal_conv3d_in8(x, wk, bias, y):
    """first convolution of the VAE encoder: x bf16 [N,T,H,W,8] contiguous (RGB in channels 0..2), wk = pack_conv_in8_weight(w)"""
    _req(x, BF16, "x", 5); _req(y, BF16, "y", 5); _req(wk, BF16, "wk", 2)
    N, T, H, W, C8 = x.shape
    Cout = y.shape[4]
    if C8 != 8 or not x.is_contiguous() or tuple(y.shape[:4]) != (N, T, H, W) or tuple(wk.shape) != (Cout, 256) or not wk.is_contiguous():
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} wk {tuple(wk.shape)} y {tuple(y.shape)}")
    _cl_check(y, "y")
    check(load_library().vt_causal_conv3d_in8_cl(x.data_ptr(), wk.data_ptr(), _p(bias), y.data_ptr(), y.stride(3), N, T, H, W, Cout,
                                                 _stream()), "vt_causal_conv3d_in8_cl")
    return y


def downsample_conv2d(x, wk, bias, y, residual=None):
    """per frame: zero line / column at the bottom / right, 3x3 conv, stride 2.  x bf16 [N,T,H,W,Cin], y bf16 [N,T,H/2,W/2,Cout];
    residual (optional, like y; no layer of the VAE has one -- the kernels' residual epilogue, for tests) is added to the result"""
    _req(x, BF16, "x", 5); _req(y, BF16, "y", 5); _req(wk, BF16, "wk", 2)
    N, T, H, W, Cin = x.shape
    Cout = y.shape[4]
    if tuple(y.shape[:4]) != (N, T, H // 2, W // 2) or tuple(wk.shape) != (Cout, 9 * Cin) or not wk.is_contiguous():
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} wk {tuple(wk.shape)} y {tuple(y.shape)}")
    _cl_check(x, "x"); _cl_check(y, "y")
    if residual is not None:
        _req(residual, BF16, "residual", 5); _cl_check(residual, "residual")
        if tuple(residual.shape) != tuple(y.shape):
            raise ValueError("residual must have the shape of y")
        check(load_library().vt_downsample_conv2d_res_cl(x.data_ptr(), x.stride(3), wk.data_ptr(), _p(bias), residual.data_ptr(),
                                                         residual.stride(3), y.data_ptr(), y.stride(3), N, T, H, W, Cin, Cout, _stream()),
              "vt_downsample_conv2d_res_cl")
        return y
    check(load_library().vt_downsample_conv2d_cl(x.data_ptr(), x.stride(3), wk.data_ptr(), _p(bias), y.data_ptr(), y.stride(3),
                                                 N, T, H, W, Cin, Cout, _stream()), "vt_downsample_conv2d_cl")
    return y


def conv3d_set_kernel(mode: int = 0, slots: int = 0):
    """kernel of causal_conv3d / downsample_conv2d: 0 = by shape, 1 = always the 128-row kernel, 2 = the 256-row producer / consumer kernel
    wherever its span check allows; slots: cap of its persistent grid, 0 = the device's own, else a multiple of 8 (tests, A/B timing)"""
    check(load_library().vt_conv3d_set_kernel(mode, slots), "vt_conv3d_set_kernel")


def conv3d_plan(N: int, T: int, H: int, W: int, Cin: int, Cout: int, kt: int = 3, stride: int = 1, ldx: int = 0):
    """(kernel, grid, tiles, tiles_per_wg) of the launch causal_conv3d (kt 3, stride 1) / downsample_conv2d (kt 1, stride 2) would make for
    this geometry under the current conv3d_set_kernel setting; no launch.  kernel: 1 = 128-row tiles, 2 = producer / consumer (256-row
    tiles, persistent).  ldx: position stride of x, 0 = Cin"""
    import ctypes as C
    k, grid, tiles, per = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    check(load_library().vt_conv3d_plan(ldx or Cin, N, T, H, W, Cin, Cout, kt, stride, C.byref(k), C.byref(grid), C.byref(tiles), C.byref(per)),
          "vt_conv3d_plan")
    return k.value, grid.value, tiles.value, per.value


def temporal_pool_frames(T: int, keep_first: bool) -> int:
    return 1 + (T - 1) // 2 if keep_first else T // 2


def temporal_pool(x, y, keep_first: bool = True):
    """VAE DownSample3D temporal compression, x bf16 [N,T,H,W,C].  keep_first: first frame kept, the rest averaged in pairs ->
    [N, 1 + (T-1)//2, ...]; not keep_first: all frames averaged in pairs -> [N, T//2, ...] (even frame counts, diffusers' rule)"""
    _req(x, BF16, "x", 5); _req(y, BF16, "y", 5)
    N, T, H, W, C = x.shape
    To = temporal_pool_frames(T, keep_first)
    if tuple(y.shape) != (N, To, H, W, C) or To < 1:
        raise ValueError(f"y must be {(N, To, H, W, C)}, got {tuple(y.shape)}")
    _cl_check(x, "x"); _cl_check(y, "y")
    check(load_library().vt_temporal_pool_cl(x.data_ptr(), x.stride(3), y.data_ptr(), y.stride(3), N, T, H * W, C, int(keep_first),
                                             _stream()), "vt_temporal_pool_cl")
    return y


def _pow2_ratio(big: int, small: int, what: str) -> int:
    if small < 1 or big % small or (big // small) & (big // small - 1):
        raise ValueError(f"{what}: {big} / {small} is not a power-of-two ratio")
    return big // small


def spatialnorm_zq_index(T: int, Tz: int, H: int, Hz: int, W: int, Wz: int):
    """the (tz[t], hz[h], wz[w]) index vectors vt_spatialnorm_silu_cl gathers with: nearest interpolation of the latent to [T, H, W]
    with the first frame handled apart (SpatialNorm3D.forward, rank-0 / fake_cp branch).  ValueError unless every ratio is a power of two."""
    rh, rw = _pow2_ratio(H, Hz, "H / Hz"), _pow2_ratio(W, Wz, "W / Wz")
    if T > 1:
        if Tz < 2:
            raise ValueError(f"T = {T} frames need a latent of at least 2 frames, got Tz = {Tz}")
        rt = _pow2_ratio(T - 1, Tz - 1, "(T-1) / (Tz-1)")
        tz = [0] + [1 + (t - 1) // rt for t in range(1, T)]
    else:
        if Tz < 1:
            raise ValueError("Tz must be at least 1")
        tz = [0]
    return tz, [h // rh for h in range(H)], [w // rw for w in range(W)]


def upsample_src_frames(T: int, temporal: bool):
    """input frame of every output frame of vt_upsample_conv2d_cl: ts(t) = t, or with temporal upsampling (and T > 1) ts(0) = 0,
    ts(t) = 1 + (t-1)//2 over 1 + 2 (T-1) output frames (Upsample3D.forward with compress_time, first frame kept single)"""
    if temporal and T > 1:
        return [0] + [1 + (t - 1) // 2 for t in range(1, 1 + 2 * (T - 1))]
    return list(range(T))


def spatialnorm_silu(x, gamma, beta, mod, y, groups: int = 32, eps: float = 1e-6, silu: bool = True, ws: Optional[torch.Tensor] = None):
    """SpatialNorm3D (+ SiLU): x, y bf16 [N,T,H,W,C] channels-last; mod bf16 [N,Tz,Hz,Wz,2C] contiguous = (conv_y(zq) | conv_b(zq)) at
    latent resolution; y = silu?(GroupNorm(x) * mod_y[zq index] + mod_b[zq index])"""
    _req(x, BF16, "x", 5); _req(y, BF16, "y", 5); _req(mod, BF16, "mod", 5)
    N, T, H, W, C = x.shape
    Nz, Tz, Hz, Wz, C2 = mod.shape
    if tuple(y.shape) != tuple(x.shape) or Nz != N or C2 != 2 * C or not mod.is_contiguous():
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} mod {tuple(mod.shape)} y {tuple(y.shape)}")
    spatialnorm_zq_index(T, Tz, H, Hz, W, Wz)              # raises ValueError on a ratio the kernel does not take
    _cl_check(x, "x"); _cl_check(y, "y")
    lib = load_library()
    need = int(lib.vt_groupnorm_ws_bytes(N, C))
    if ws is None:
        ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    check(lib.vt_spatialnorm_silu_cl(x.data_ptr(), x.stride(3), _p(gamma), _p(beta), mod.data_ptr(), y.data_ptr(), y.stride(3),
                                     N, T, H, W, C, Tz, Hz, Wz, groups, eps, int(silu), ws.data_ptr(), ws.numel() * 4, _stream()),
          "vt_spatialnorm_silu_cl")
    return y


def upsample_conv2d(x, wk, bias, y, temporal: bool = False):
    """Upsample3D.forward fused: nearest 2x in h / w (temporal: also in t, first frame kept single), then the per-frame 3x3 convolution.
    x bf16 [N,T,H,W,Cin], wk = pack_conv_weight(Conv2d weight), y bf16 [N, len(upsample_src_frames(T, temporal)), 2H, 2W, Cout]"""
    _req(x, BF16, "x", 5); _req(y, BF16, "y", 5); _req(wk, BF16, "wk", 2)
    N, T, H, W, Cin = x.shape
    Cout = y.shape[4]
    To = len(upsample_src_frames(T, temporal))
    if tuple(y.shape[:4]) != (N, To, 2 * H, 2 * W) or tuple(wk.shape) != (Cout, 9 * Cin) or not wk.is_contiguous():
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} wk {tuple(wk.shape)} y {tuple(y.shape)} (expected {To} output frames)")
    _cl_check(x, "x"); _cl_check(y, "y")
    check(load_library().vt_upsample_conv2d_cl(x.data_ptr(), x.stride(3), wk.data_ptr(), _p(bias), y.data_ptr(), y.stride(3),
                                               N, T, H, W, Cin, Cout, int(temporal), _stream()), "vt_upsample_conv2d_cl")
    return y


def rmsnorm(x, w, y, eps: float = 1e-6):
    """T5LayerNorm: y = x * rsqrt(mean(x^2) + eps) * w (rows of a 2-d bf16 tensor)"""
    _req(x, BF16, "x", 2); _req(y, BF16, "y", 2); _req(w, BF16, "w", 1)
    check(load_library().vt_rmsnorm_bf16(x.data_ptr(), x.stride(0), w.data_ptr(), y.data_ptr(), y.stride(0), x.shape[0], x.shape[1],
                                         eps, _stream()), "vt_rmsnorm_bf16")


def gated_gelu(u, y):
    """y[:, f] = gelu_tanh(u[:, f]) * u[:, F + f] with F = y.shape[1]"""
    _req(u, BF16, "u", 2); _req(y, BF16, "y", 2)
    check(load_library().vt_gated_gelu_bf16(u.data_ptr(), u.stride(0), y.data_ptr(), y.stride(0), u.shape[0], y.shape[1], _stream()),
          "vt_gated_gelu_bf16")


def attn_bwd_chain_workspace(B: int, H: int, S: int, device) -> Optional[torch.Tensor]:
    """scratch for the dQ hand-off chains of vt_attn_bwd_hd64 (None when the library runs without chains); one buffer
    serves every attention-backward launch of a step"""
    if _SIDE_STREAMS["n"] > 0 or _CHAIN_STATE["disabled"]:
        return None          # chained workgroups spin on each other: every one of them must be resident, which nobody can
                             # promise while kernels of another stream (encoders, collectives) share the CUs
    n = int(load_library().vt_attn_bwd_chain_ws_bytes(B, H, S))
    if n <= 0:
        return None
    key = str(device)
    ws = _CHAIN_WS.get(key)
    if ws is None or ws.numel() < n:
        old = ws
        ws = _CHAIN_WS[key] = torch.empty(n, dtype=torch.uint8, device=device)
        ws[:256].zero_()                                    # the sticky words are the caller's to clear, once
        if old is not None:
            ws[64:256].copy_(old[64:256])                   # ... and must survive a re-allocation
    return ws


_CHAIN_WS = {}      # device -> workspace, reused by every launch on that device (launches of one stream are ordered)
_SIDE_STREAMS = {"n": 0}
# What happens when a dQ hand-off wait times out (the persistent workgroups of a launch were not all resident: another stream, a profiler):
# "launch" (default): the error word is read after every chained launch (one 4-byte read-back per attention backward; ~0.1 % of a
# CogVideoX step); a launch that timed out is REDONE with plain atomics (its outputs are overwritten, dQ re-zeroed), the chains stay off for the
# rest of the process, training goes on with valid gradients on every rank.  "step" (VT355_CHAIN_VERIFY=step): no read-back; the sticky count
# makes vt_adamw skip that step's update and FusedAdamW.check_errors() raise at the next step.
_CHAIN_STATE = {"disabled": False, "redone": 0, "verify": __import__("os").environ.get("VT355_CHAIN_VERIFY", "launch")}


def attn_bwd_chain_redone() -> int:
    """attention-backward launches that were redone without chains after a hand-off time-out (0 in a healthy run)"""
    return _CHAIN_STATE["redone"]


def declare_side_stream(active: bool):
    """Tell the engine that kernels of ANOTHER stream (frozen encoders one step ahead, an overlapped collective) may share the
    CUs with the backward pass from now on / no longer.  While any is declared the attention backward runs without dQ
    hand-off chains (plain atomics): the chains' inter-workgroup waits assume that all persistent workgroups are resident."""
    _SIDE_STREAMS["n"] = max(0, _SIDE_STREAMS["n"] + (1 if active else -1))


def chain_guard(device) -> Optional[torch.Tensor]:
    """int32 [1] view of the STICKY time-out counter of this device's chain workspace (None: no chained launch so far):
    what FusedAdamW hands to vt_adamw as ``guard``"""
    ws = _CHAIN_WS.get(str(device))
    return None if ws is None else ws[64:68].view(torch.int32)


def attn_bwd_chain_errors() -> int:
    """time-outs of dQ hand-off waits since the workspaces were created (sticky count; synchronises); non-zero = some
    attention backward produced an invalid dQ"""
    return sum(int(ws[64:68].view(torch.int32).item()) for ws in _CHAIN_WS.values())


def attn_bwd_chain_errors_clear():
    for ws in _CHAIN_WS.values():
        ws[64:256].zero_()


def conv_set_tile(mode: int = 0, slots: int = 0):
    """0 = per shape, 1 = always the 128 x 128 convolution kernels, 2 = the 320-wide kernels whenever Cout % 320 == 0; slots: cap of the
    128 x 320 forward kernel's persistent grid, 0 = the device's CU count, else 1 .. that count (tests, A/B timing)"""
    lib = load_library()
    check(lib.vt_conv_set_slots(slots), "vt_conv_set_slots")
    check(lib.vt_conv_set_tile(mode), "vt_conv_set_tile")


def conv_plan(N: int, T: int, H: int, W: int, Cin: int, Cout: int, kernel=(1, 3, 3), padding=(0, 1, 1), stride: int = 1, ldx: int = 0, ldy: int = 0):
    """(kernel, grid, tiles, tiles_per_wg) of the launch conv_cl would make for this geometry under the current conv_set_tile setting; no
    launch.  kernel: 1 = 128 x 128 tiles (one per workgroup), 2 = 128 x 320 tiles, persistent.  ldx / ldy: position strides, 0 = Cin / Cout"""
    import ctypes as C
    k, grid, tiles, per = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    check(load_library().vt_conv_plan(ldx or Cin, ldy or Cout, N, T, H, W, Cin, Cout, *kernel, *padding, stride, C.byref(k), C.byref(grid),
                                      C.byref(tiles), C.byref(per)), "vt_conv_plan")
    return k.value, grid.value, tiles.value, per.value


def conv_dw_plan(N: int, T: int, H: int, W: int, Cin: int, Cout: int, kernel=(1, 3, 3), padding=(0, 1, 1), stride: int = 1, ldx: int = 0, lddy: int = 0):
    """(kernel, tiles, splits, m_chunk, dbias_fused, row_step) of the launch conv_dw_cl / linear_dw (N = T = H = 1, W = rows, one tap) would
    make under the current conv_set_tile setting; no launch.  kernel: 1 = 128 x 128 tiles, 2 = 320-row tiles; splits x m_chunk cover the
    output positions; dbias_fused: 1 = the kernel adds the bias gradient, 0 = the column-sum kernel does; row_step > 0: the call runs in row
    chunks of that many and the other values describe the first"""
    import ctypes as C
    k, tiles, splits, chunk, fused, step = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
    check(load_library().vt_conv_dw_plan(lddy or Cout, ldx or Cin, N, T, H, W, Cin, Cout, *kernel, *padding, stride, C.byref(k), C.byref(tiles),
                                         C.byref(splits), C.byref(chunk), C.byref(fused), C.byref(step)), "vt_conv_dw_plan")
    return k.value, tiles.value, splits.value, chunk.value, fused.value, step.value


def gemm_set_tile(mode: int = 0):
    """tile selection of vt_gemm_bf16: 0 = by shape, 1 = always 128x128, 2 = always 256x256, 3 = 256x128 producer / consumer (tuning / test knob)"""
    check(load_library().vt_gemm_set_tile(mode), "vt_gemm_set_tile")


def gemm_set_big_loop(mode: int = 0):
    """K-loop of the 256x256 kernel: 0 = by shape, 1 = always two-phase, 2 = always eight-phase (bit-identical; tuning / test knob)"""
    check(load_library().vt_gemm_set_big_loop(mode), "vt_gemm_set_big_loop")


def gemm_big_last_wide() -> int:
    """epilogue path of the last 256x256-kernel launch: 1 = 16-byte accesses, 0 = the 8-byte path, -1 = none yet (tests)"""
    return load_library().vt_gemm_big_last_wide()


def gemm_kernel(M: int, N: int, K: int) -> int:
    """the kernel vt_gemm_bf16 runs for this shape under the current tile mode: 1 = 128x128, 2 = 256x256, 3 = 256x128 producer / consumer,
    4 = the producer / consumer kernel's 128-row instantiation"""
    k = load_library().vt_gemm_bf16_kernel(M, N, K)
    if k < 0:
        check(k, "vt_gemm_bf16_kernel")
    return k


def gemm_block_tile(M: int, N: int, K: int) -> int:
    """the `tile` a CogVideoX block passes to gemm() for its ff.net.2 forward and ff.net.0.proj input-gradient products: 2 where the 256x256
    kernel was measured ahead of the shape rule's choice, 0 = no opinion (vt_gemm_bf16_block_tile, csrc/gemm_bf16.hip)"""
    t = load_library().vt_gemm_bf16_block_tile(M, N, K)
    if t < 0:
        check(t, "vt_gemm_bf16_block_tile")
    return t


def attn_bwd_set_chain(chain_len: int = 0, slots: int = 0):
    """tuning / test knob of the dQ hand-off chains (0 = defaults); see include/vt355.h"""
    check(load_library().vt_attn_bwd_set_chain(chain_len, slots), "vt_attn_bwd_set_chain")


def attn_bwd_chain_plan(B: int, H: int, S: int, have_ws: bool = True):
    """(chain_len, grid, generations) of the launch vt_attn_bwd_hd64 would make for this problem under the current knobs; no launch.
    chain_len 1: every key block adds its dQ atomically (always so without a workspace)"""
    import ctypes as C
    L, grid, gens = C.c_int(0), C.c_int(0), C.c_int(0)
    check(load_library().vt_attn_bwd_chain_plan(B, H, S, int(have_ws), C.byref(L), C.byref(grid), C.byref(gens)), "vt_attn_bwd_chain_plan")
    return L.value, grid.value, gens.value


def attn_bwd_chain_error(chain_ws: torch.Tensor) -> int:
    """error word of the last launch that used this workspace (synchronises): non-zero = a hand-off wait timed out"""
    return int(chain_ws[32:36].view(torch.int32).item())


def attn_bwd(q, k, v, o, do, lse2, delta_ws, dq_f32, dk, dv, B: int, H: int, S: int, scale: Optional[float] = None,
             q_prescaled: bool = False, chain_ws: Optional[torch.Tensor] = None, _entry=None):
    """_entry: another build of the same entry point (tests: the forced-time-out build of libvt355_test.so)"""
    scale = 1.0 / math.sqrt(64) if scale is None else scale
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o), ("do", do), ("dk", dk), ("dv", dv)):
        _req(t, BF16, n, 3)
    _req(dq_f32, torch.float32, "dq_f32", 3)
    lib = load_library()

    def launch(ws, fn=None):
        check((fn or lib.vt_attn_bwd_hd64)(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(),
                               lse2.data_ptr(), delta_ws.data_ptr(), dq_f32.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                               B, H, S,
                               q.stride(1), k.stride(1), v.stride(1), o.stride(1), do.stride(1),
                               dq_f32.stride(1), dk.stride(1), dv.stride(1),
                               q.stride(0), k.stride(0), v.stride(0), o.stride(0), do.stride(0),
                               dq_f32.stride(0), dk.stride(0), dv.stride(0), scale, int(q_prescaled),
                               None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(),
                               _stream()),
          "vt_attn_bwd_hd64")
    with _timed("attn_bwd"):
        launch(chain_ws, _entry)
    if chain_ws is not None and _CHAIN_STATE["verify"] == "launch" and attn_bwd_chain_error(chain_ws) != 0:
        # a hand-off wait gave up (every wait is bounded): this launch's dQ is invalid.  Redo it with plain atomics -- same inputs, outputs
        # overwritten -- and keep the chains off from here on: whatever shared the CUs this time may do so again.
        import warnings
        _CHAIN_STATE["disabled"] = True
        _CHAIN_STATE["redone"] += 1
        warnings.warn("vt_attn_bwd_hd64: a dQ hand-off wait timed out (the persistent workgroups were not all resident: another stream or a "
                      "profiler shared the CUs); the launch was redone with plain atomics and the hand-off chains are switched off for the rest "
                      "of this process (VT_BWD_CHAIN=1 avoids them from the start; ops.declare_side_stream(True) announces a concurrent stream)")
        dq_f32.zero_()
        launch(None)
        chain_ws[32:36].zero_()
        chain_ws[64:68].zero_()           # the sticky count only held this repaired launch: the optimizer guard must not refuse the step


def ln_modulate_fwd(x, y, gamma, beta, mod, mean, rstd, D: int, S: int, St: int, eps: float):
    """mod: None or (shift_txt, scale_txt, shift_vid, scale_vid, bstride) fp32 views."""
    _req(x, BF16, "x", 2); _req(y, BF16, "y", 2)
    m = (None, None, None, None, 0) if mod is None else mod
    lib = load_library()
    with _timed_hbm("ln_modulate_fwd", x.shape[0], 4.0 * x.shape[0] * D):           # x read, y written, bf16
        check(lib.vt_ln_modulate_fwd(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), _p(gamma), _p(beta),
                                     _p(m[0]), _p(m[1]), _p(m[2]), _p(m[3]), m[4], _p(mean), _p(rstd),
                                     x.shape[0], D, S, St, eps, _stream()), "vt_ln_modulate_fwd")


def ln_modulate_bwd(dy, x, mean, rstd, gamma, scales, dres, dx, D: int, S: int, St: int):
    """scales: None or (scale_txt, scale_vid, bstride)."""
    _req(dy, BF16, "dy", 2); _req(x, BF16, "x", 2); _req(dx, BF16, "dx", 2)
    sc = (None, None, 0) if scales is None else scales
    lib = load_library()
    with _timed_hbm("ln_modulate_bwd", x.shape[0], (6.0 if dres is None else 8.0) * x.shape[0] * D):   # dy, x (, residual gradient) read, dx written
        check(lib.vt_ln_modulate_bwd(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), mean.data_ptr(), rstd.data_ptr(),
                                     _p(gamma), _p(sc[0]), _p(sc[1]), sc[2], _p(dres), 0 if dres is None else dres.stride(0),
                                     dx.data_ptr(), dx.stride(0), x.shape[0], D, S, St, _stream()), "vt_ln_modulate_bwd")


def qk_layernorm_fwd(qkv, out, gq, bq, gk, bk, mean, rstd, H: int, eps: float, q_scale: float = 1.0, rope=None):
    _req(qkv, BF16, "qkv", 2); _req(out, BF16, "out", 2)
    lib = load_library()
    rc, rsn, S, St = _rope_args(rope, qkv.shape[0])
    with _timed_hbm("qk_layernorm_fwd", qkv.shape[0], 8.0 * qkv.shape[0] * H * 64):   # q, k thirds read, q_hat | k_hat written
        check(lib.vt_qk_layernorm_fwd(qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), gq.data_ptr(), bq.data_ptr(),
                                      gk.data_ptr(), bk.data_ptr(), mean.data_ptr(), rstd.data_ptr(), qkv.shape[0], H, eps,
                                      q_scale, rc, rsn, S, St, _stream()), "vt_qk_layernorm_fwd")


def qk_layernorm_bwd(dq_hat_f32, dk_hat, qkv, mean, rstd, gq, gk, dqkv, H: int, rope=None):
    _req(dq_hat_f32, torch.float32, "dq_hat", 2); _req(dk_hat, BF16, "dk_hat", 2)
    lib = load_library()
    rc, rsn, S, St = _rope_args(rope, qkv.shape[0])
    with _timed_hbm("qk_layernorm_bwd", qkv.shape[0], 14.0 * qkv.shape[0] * H * 64):  # fp32 dq_hat, bf16 dk_hat, q, k read; dq, dk written
        check(lib.vt_qk_layernorm_bwd(dq_hat_f32.data_ptr(), dq_hat_f32.stride(0), dk_hat.data_ptr(), dk_hat.stride(0),
                                      qkv.data_ptr(), qkv.stride(0), mean.data_ptr(), rstd.data_ptr(), gq.data_ptr(), gk.data_ptr(),
                                      dqkv.data_ptr(), dqkv.stride(0), qkv.shape[0], H, rc, rsn, S, St, _stream()),
              "vt_qk_layernorm_bwd")


def gate_mul(x, y, g_txt, g_vid, bstride: int, D: int, S: int, St: int):
    _req(x, BF16, "x", 2); _req(y, BF16, "y", 2)
    M = x.shape[0]
    _rows_cols(x, M, D, "x", "gate_mul"); _rows_cols(y, M, D, "y", "gate_mul")
    if S > 0 and D > 0 and M > 0:
        need = ((M + S - 1) // S - 1) * bstride + D          # the last sample's gate row ends here
        for nm, g in (("g_txt", g_txt), ("g_vid", g_vid)):
            if g.dtype != torch.float32 or _span(g) < need or (g.dim() > 1 and g.shape[-1] < D):
                raise ValueError(f"gate_mul: {nm} {tuple(g.shape)} ({g.dtype}) does not hold {need} fp32 gate elements at bstride {bstride}")
    lib = load_library()
    check(lib.vt_gate_mul(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), g_txt.data_ptr(), g_vid.data_ptr(), bstride,
                          x.shape[0], D, S, St, _stream()), "vt_gate_mul")


def silu(x, y):
    _req(x, BF16, "x"); _req(y, BF16, "y")
    check(load_library().vt_silu_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "vt_silu_bf16")


def cast_f32_bf16(x, y):
    _req(x, torch.float32, "x"); _req(y, BF16, "y")
    check(load_library().vt_cast_f32_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "vt_cast_f32_bf16")


def timestep_embedding(t, out, flip: bool = True, freq_shift: float = 0.0):
    _req(t, torch.int64, "t", 1); _req(out, BF16, "out", 2)
    check(load_library().vt_timestep_embedding(t.data_ptr(), out.data_ptr(), out.shape[0], out.shape[1], int(flip),
                                               freq_shift, _stream()), "vt_timestep_embedding")


def patchify(img, tok, P: int):
    _req(img, BF16, "img", 5); _req(tok, BF16, "tok", 2)
    B, F, C, H, W = img.shape
    _patch_rows(img, tok, P, "patchify")
    check(load_library().vt_patchify(img.data_ptr(), tok.data_ptr(), B, F, C, H, W, P, tok.stride(0), _stream()), "vt_patchify")


def unpatchify(tok, img, P: int):
    _req(img, BF16, "img", 5); _req(tok, BF16, "tok", 2)
    B, F, C, H, W = img.shape
    _patch_rows(img, tok, P, "unpatchify")
    check(load_library().vt_unpatchify(tok.data_ptr(), img.data_ptr(), B, F, C, H, W, P, tok.stride(0), _stream()),
          "vt_unpatchify")


def add_noise(x0, noise, sa, sb, noisy):
    _req(x0, torch.float32, "x0"); _req(noise, torch.float32, "noise"); _req(noisy, BF16, "noisy")
    B = x0.shape[0]
    _numel(noise, x0.numel(), "noise", "add_noise"); _numel(noisy, x0.numel(), "noisy", "add_noise")
    _numel(sa, B, "sa", "add_noise"); _numel(sb, B, "sb", "add_noise")
    check(load_library().vt_add_noise(x0.data_ptr(), noise.data_ptr(), sa.data_ptr(), sb.data_ptr(), noisy.data_ptr(),
                                      x0.numel() // B, B, _stream()), "vt_add_noise")


_U64 = 0xFFFFFFFFFFFFFFFF


def philox_normal(out, seed: int, stream_id: int):
    """out [B, ...] fp32 or bf16, contiguous: standard normals under the header's noise convention (sample b: key seed + b)"""
    if out.dtype not in (torch.float32, BF16):
        raise ValueError(f"philox_normal: out must be fp32 or bf16, got {out.dtype}")
    _req(out, out.dtype, "out")
    if not out.is_contiguous() or out.dim() < 1 or out.numel() == 0:
        raise ValueError(f"philox_normal: out must be a contiguous, non-empty [B, ...] tensor, got {tuple(out.shape)}")
    B = out.shape[0]
    check(load_library().vt_philox_normal(out.data_ptr(), int(out.dtype == BF16), out.numel() // B, B, int(seed) & _U64, int(stream_id),
                                          _stream()), "vt_philox_normal")
    return out


def dpm_step(v, x, x0_old, noise, x_out, x0_out, g: Optional[float], sa: float, sb: float, m1: float, m2: float, m3: float, m4: float,
             m_noise: float, second_order: bool, seed: int = 0, stream_id: int = 0):
    """guidance combine + one CogVideoXDPMScheduler.step (vt_dpm_step).  x [B, ...] bf16; v [2B, ...] (uncond, cond) with a guidance
    scale g, or [B, ...] with g None; x0_old fp32 | None (first order); noise fp32 | None (drawn in the kernel from seed / stream_id)."""
    _req(v, BF16, "v"); _req(x, BF16, "x"); _req(x_out, BF16, "x_out"); _req(x0_out, torch.float32, "x0_out")
    B, n = x.shape[0], x.numel()
    guided = g is not None
    for name, t in (("v", v), ("x", x), ("x0_old", x0_old), ("noise", noise), ("x_out", x_out), ("x0_out", x0_out)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"dpm_step: {name} must be contiguous")
    if v.numel() != (2 * n if guided else n):
        raise ValueError(f"dpm_step: v holds {v.numel()} elements for {n} latent elements (guidance {'on' if guided else 'off'})")
    _numel(x_out, n, "x_out", "dpm_step"); _numel(x0_out, n, "x0_out", "dpm_step")
    if second_order:
        if x0_old is None:
            raise ValueError("dpm_step: a second-order step needs x0_old")
        _req(x0_old, torch.float32, "x0_old"); _numel(x0_old, n, "x0_old", "dpm_step")
    if noise is not None:
        _req(noise, torch.float32, "noise"); _numel(noise, n, "noise", "dpm_step")
    scal = [float(g) if guided else 0.0, sa, sb, m1, m2, m3 if second_order else 0.0, m4 if second_order else 0.0, m_noise]
    if not all(math.isfinite(s) for s in scal):
        raise ValueError(f"dpm_step: non-finite coefficient among (g, sa, sb, m1, m2, m3, m4, m_noise) = {scal}")
    check(load_library().vt_dpm_step(v.data_ptr(), x.data_ptr(), _p(x0_old) if second_order else None, _p(noise), x_out.data_ptr(),
                                     x0_out.data_ptr(), n // B, B, int(guided), *scal, int(bool(second_order)), int(seed) & _U64,
                                     int(stream_id), _stream()), "vt_dpm_step")


def diffusion_loss(vpred, noisy, x0, sa, sb, w, loss, partials, dvpred, grad_scale: float = 1.0):
    _req(vpred, BF16, "vpred"); _req(noisy, BF16, "noisy"); _req(x0, torch.float32, "x0")
    B = x0.shape[0]
    _loss_operands("diffusion_loss", vpred, noisy, x0, sa, sb, w, dvpred)
    _numel(loss, 1, "loss", "diffusion_loss"); _numel(partials, 512, "partials", "diffusion_loss")
    check(load_library().vt_diffusion_loss(vpred.data_ptr(), noisy.data_ptr(), x0.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                           w.data_ptr(), loss.data_ptr(), partials.data_ptr(), _p(dvpred),
                                           x0.numel() // B, B, grad_scale, _stream()), "vt_diffusion_loss")


def diffusion_loss_bwd(vpred, noisy, x0, sa, sb, w, grad_out, dvpred):
    _req(grad_out, torch.float32, "grad_out")
    B = x0.shape[0]
    _loss_operands("diffusion_loss_bwd", vpred, noisy, x0, sa, sb, w, dvpred)
    _numel(grad_out, 1, "grad_out", "diffusion_loss_bwd")
    check(load_library().vt_diffusion_loss_bwd(vpred.data_ptr(), noisy.data_ptr(), x0.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                               w.data_ptr(), grad_out.data_ptr(), dvpred.data_ptr(), x0.numel() // B, B,
                                               _stream()), "vt_diffusion_loss_bwd")


def adamw(p, g, m, v, p_bf16, lr, beta1, beta2, eps, wd, step: int, grad_scale: float = 1.0, guard: Optional[torch.Tensor] = None,
          clip_coef: Optional[torch.Tensor] = None, clip_value: float = 0.0):
    """guard: device int32 [1]; a non-zero value at execution time makes the kernel skip the whole update.
    clip_coef: device fp32 scalar written by clip_finalize (global-norm clipping); clip_value > 0: clamp(g * grad_scale, -v, +v)"""
    for n, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _req(t, torch.float32, n)
    if guard is not None:
        _req(guard, torch.int32, "guard")
    with _timed_hbm("adamw", p.numel(), (28.0 + (2.0 if p_bf16 is not None else 0.0)) * p.numel()):   # p, g, m, v read; p, m, v (+ bf16 copy) written
        if clip_coef is None and not clip_value > 0.0:
            check(load_library().vt_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(p_bf16), p.numel(),
                                          lr, beta1, beta2, eps, wd, step, grad_scale, _p(guard), _stream()), "vt_adamw")
        else:
            if clip_coef is not None:
                _req(clip_coef, torch.float32, "clip_coef")
            check(load_library().vt_adamw_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(p_bf16), p.numel(),
                                               lr, beta1, beta2, eps, wd, step, grad_scale, _p(guard), _p(clip_coef),
                                               float(clip_value), _stream()), "vt_adamw_clip")


def grad_sqnorm_partials() -> int:
    """partial sums that one grad_sqnorm launch writes (the fixed grid of the kernel)"""
    return int(load_library().vt_grad_sqnorm_partials())


def grad_sqnorm(g, partials, slot: int = 0):
    """sum of g^2 of one flat fp32 buffer (any 4-byte aligned view), as grad_sqnorm_partials() partial sums in slot ``slot`` of partials"""
    _req(g, torch.float32, "g"); _req(partials, torch.float32, "partials")
    if partials.numel() < (slot + 1) * grad_sqnorm_partials():
        raise ValueError("partials holds fewer than slot + 1 slots")
    check(load_library().vt_grad_sqnorm(g.data_ptr(), g.numel(), partials.data_ptr(), slot, _stream()), "vt_grad_sqnorm")


def clip_finalize(partials, nslots: int, grad_scale: float, max_norm: float, record):
    """record[0] = total_norm = grad_scale * sqrt(sum of the first nslots slots), record[1] = min(1, max_norm / (total_norm + 1e-6))"""
    _req(partials, torch.float32, "partials"); _req(record, torch.float32, "record")
    if partials.numel() < nslots * grad_sqnorm_partials() or record.numel() < 2:
        raise ValueError("partials / record too small")
    check(load_library().vt_clip_finalize(partials.data_ptr(), nslots, float(grad_scale), float(max_norm), record.data_ptr(),
                                          _stream()), "vt_clip_finalize")


def lora_down(x, a, R: int, t_out, K: int, zero_cols: int = 48):
    """t_out[:, :16] = x[:, :K] @ a[:R]^T (zero past R); t_out[:, 16:16+zero_cols] = 0."""
    _req(x, BF16, "x", 2); _req(a, BF16, "a", 2); _req(t_out, BF16, "t", 2)
    check(load_library().vt_lora_down(x.data_ptr(), x.stride(0), a.data_ptr(), a.stride(0), R, t_out.data_ptr(),
                                      t_out.stride(0), x.shape[0], K, zero_cols, _stream()), "vt_lora_down")


_SKINNY_WS = {}


def _skinny_ws(lib, big, P: int, use_workspace: bool):
    """the per-device workspace of the two-stage skinny_tn reduction (None: fp32 atomics), reused across calls (stream-ordered)"""
    if not use_workspace:
        return None
    need = lib.vt_skinny_tn_workspace_bytes(P) // 4
    key = big.device
    if key not in _SKINNY_WS or _SKINNY_WS[key].numel() < need:
        _SKINNY_WS[key] = torch.empty(need, dtype=torch.float32, device=big.device)
    return _SKINNY_WS[key]


def skinny_tn(big, small, R: int, out, osp: int, osr: int, alpha: float, P: int, use_workspace: bool = False):
    """out[p*osp + r*osr] += alpha * sum_m big[m,p] * small[m,r]; fp32 atomics by default; use_workspace=True selects the two-stage, bitwise-reproducible reduction (measured slightly slower)."""
    _req(big, BF16, "big", 2); _req(small, BF16, "small", 2); _req(out, torch.float32, "out")
    lib = load_library()
    ws = _skinny_ws(lib, big, P, use_workspace)
    check(lib.vt_skinny_tn(big.data_ptr(), big.stride(0), small.data_ptr(), small.stride(0), R, out.data_ptr(),
                           osp, osr, alpha, big.shape[0], P, _p(ws), _stream()), "vt_skinny_tn")


def lora_up_add(dx, dt, a, R: int, K: int):
    _req(dx, BF16, "dx", 2); _req(dt, BF16, "dt", 2); _req(a, BF16, "a", 2)
    check(load_library().vt_lora_up_add(dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), a.data_ptr(), a.stride(0),
                                        R, dx.shape[0], K, _stream()), "vt_lora_up_add")


def lora_pack_b(bcat_f32, wext, ldw: int, n_adapters: int, d_out: int, r: int, scale: float):
    check(load_library().vt_lora_pack_b(bcat_f32.data_ptr(), wext.data_ptr(), ldw, n_adapters, d_out, r, scale, _stream()),
          "vt_lora_pack_b")


def lora_pack_bt(bcat_f32, wtext, ldwt: int, n_adapters: int, d_out: int, r: int, scale: float):
    check(load_library().vt_lora_pack_bt(bcat_f32.data_ptr(), wtext.data_ptr(), ldwt, n_adapters, d_out, r, scale, _stream()),
          "vt_lora_pack_bt")


# ---- ranks 17..128: the wide K-extension layout (csrc/lora_wide.hip); adapter j owns extension columns [j*rp, j*rp + r) ----
def lora_down_wide(x, a, n_adapters: int, r: int, rp: int, ext: int, t_out, K: int):
    """t_out[:, j*rp + i] = x[:, :K] @ a[j*r + i]^T for every adapter in one pass over x; every other column of t_out[:, :ext] = 0."""
    _req(x, BF16, "x", 2); _req(a, BF16, "a", 2); _req(t_out, BF16, "t", 2)
    check(load_library().vt_lora_down_wide(x.data_ptr(), x.stride(0), a.data_ptr(), a.stride(0), n_adapters, r, rp, ext,
                                           t_out.data_ptr(), t_out.stride(0), x.shape[0], K, _stream()), "vt_lora_down_wide")


def lora_tn_wide(big, small, R: int, out, osp: int, osr: int, alpha: float, P: int):
    """out[p*osp + i*osr] += alpha * sum_m big[m,p] * small[m,i] for R <= 128 on MFMA (fp32 atomics across row slices)."""
    _req(big, BF16, "big", 2); _req(small, BF16, "small", 2); _req(out, torch.float32, "out")
    check(load_library().vt_lora_tn_wide(big.data_ptr(), big.stride(0), small.data_ptr(), small.stride(0), R, out.data_ptr(),
                                         osp, osr, alpha, big.shape[0], P, _stream()), "vt_lora_tn_wide")


def lora_up_add_wide(dx, dt, a, n_adapters: int, r: int, rp: int, K: int):
    """dx[:, :K] += sum_j dt[:, j*rp : j*rp + r] @ a[j*r : (j+1)*r] in place, all adapters in one pass over dx."""
    _req(dx, BF16, "dx", 2); _req(dt, BF16, "dt", 2); _req(a, BF16, "a", 2)
    check(load_library().vt_lora_up_add_wide(dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), a.data_ptr(), a.stride(0),
                                             n_adapters, r, rp, dx.shape[0], K, _stream()), "vt_lora_up_add_wide")


def lora_pack_b_wide(bcat_f32, wext, ldw: int, n_adapters: int, d_out: int, r: int, rp: int, ext: int, scale: float):
    check(load_library().vt_lora_pack_b_wide(bcat_f32.data_ptr(), wext.data_ptr(), ldw, n_adapters, d_out, r, rp, ext, scale,
                                             _stream()), "vt_lora_pack_b_wide")


def lora_pack_bt_wide(bcat_f32, wtext, ldwt: int, n_adapters: int, d_out: int, r: int, rp: int, ext: int, scale: float):
    check(load_library().vt_lora_pack_bt_wide(bcat_f32.data_ptr(), wtext.data_ptr(), ldwt, n_adapters, d_out, r, rp, ext, scale,
                                              _stream()), "vt_lora_pack_bt_wide")


# ---- lora_dropout > 0 (csrc/lora.hip, csrc/lora_wide.hip): the six rank-side products under recomputed Philox keep masks ----
# Adapter j of a call is adapter site site0 + j; element (m, k) of the logical [M, K] input is kept iff word e % 4 of
# Philox(seed, (site << 36) + e / 4), e = m * K + k, is >= floor(p * 2^32) (oracle/philox.py: dropout_keep_mask(M, K, p, seed, site << 36)).
_U64 = 0xFFFFFFFFFFFFFFFF


def lora_down_drop(x, a, R: int, n_adapters: int, t_out, K: int, p: float, seed: int, site0: int, zero_cols: int = 48):
    """lora_down with the n_adapters adapters of r = R / n_adapters rows each reading x under their own keep masks, times 1/(1-p)."""
    _req(x, BF16, "x", 2); _req(a, BF16, "a", 2); _req(t_out, BF16, "t", 2)
    check(load_library().vt_lora_down_drop(x.data_ptr(), x.stride(0), a.data_ptr(), a.stride(0), R, n_adapters, t_out.data_ptr(),
                                           t_out.stride(0), x.shape[0], K, zero_cols, float(p), int(seed) & _U64, site0, _stream()),
          "vt_lora_down_drop")


def skinny_tn_drop(big, small, R: int, n_adapters: int, out, osp: int, osr: int, alpha: float, P: int, p: float, seed: int, site0: int,
                   use_workspace: bool = False):
    """skinny_tn with big (the logical [M, P] adapter input) masked per group of R / n_adapters columns of small, times 1/(1-p)."""
    _req(big, BF16, "big", 2); _req(small, BF16, "small", 2); _req(out, torch.float32, "out")
    lib = load_library()
    ws = _skinny_ws(lib, big, P, use_workspace)
    check(lib.vt_skinny_tn_drop(big.data_ptr(), big.stride(0), small.data_ptr(), small.stride(0), R, n_adapters, out.data_ptr(),
                                osp, osr, alpha, big.shape[0], P, _p(ws), float(p), int(seed) & _U64, site0, _stream()),
          "vt_skinny_tn_drop")


def lora_up_add_drop(dx, dt, a, R: int, n_adapters: int, K: int, p: float, seed: int, site0: int):
    """dx[:, :K] += 1/(1-p) sum_j keep_j * (dt[:, j r:(j+1) r] @ a[j r:(j+1) r]) in place, r = R / n_adapters."""
    _req(dx, BF16, "dx", 2); _req(dt, BF16, "dt", 2); _req(a, BF16, "a", 2)
    check(load_library().vt_lora_up_add_drop(dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), a.data_ptr(), a.stride(0),
                                             R, n_adapters, dx.shape[0], K, float(p), int(seed) & _U64, site0, _stream()),
          "vt_lora_up_add_drop")


def lora_down_wide_drop_fits(n_adapters: int, rp: int) -> bool:
    """whether lora_down_wide_drop takes n_adapters adapters of padded rank rp in one call (else: one call per adapter)"""
    return bool(load_library().vt_lora_down_wide_drop_fits(n_adapters, rp))


def lora_down_wide_drop(x, a, n_adapters: int, r: int, rp: int, ext: int, t_out, K: int, p: float, seed: int, site0: int):
    _req(x, BF16, "x", 2); _req(a, BF16, "a", 2); _req(t_out, BF16, "t", 2)
    check(load_library().vt_lora_down_wide_drop(x.data_ptr(), x.stride(0), a.data_ptr(), a.stride(0), n_adapters, r, rp, ext,
                                                t_out.data_ptr(), t_out.stride(0), x.shape[0], K, float(p), int(seed) & _U64, site0,
                                                _stream()), "vt_lora_down_wide_drop")


def lora_tn_wide_drop(big, small, R: int, out, osp: int, osr: int, alpha: float, P: int, p: float, seed: int, site: int):
    _req(big, BF16, "big", 2); _req(small, BF16, "small", 2); _req(out, torch.float32, "out")
    check(load_library().vt_lora_tn_wide_drop(big.data_ptr(), big.stride(0), small.data_ptr(), small.stride(0), R, out.data_ptr(),
                                              osp, osr, alpha, big.shape[0], P, float(p), int(seed) & _U64, site, _stream()),
          "vt_lora_tn_wide_drop")


def lora_up_add_wide_drop(dx, dt, a, n_adapters: int, r: int, rp: int, K: int, p: float, seed: int, site0: int):
    _req(dx, BF16, "dx", 2); _req(dt, BF16, "dt", 2); _req(a, BF16, "a", 2)
    check(load_library().vt_lora_up_add_wide_drop(dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), a.data_ptr(), a.stride(0),
                                                  n_adapters, r, rp, dx.shape[0], K, float(p), int(seed) & _U64, site0, _stream()),
          "vt_lora_up_add_wide_drop")


def _req_preact(u, dx, K: int, dt=None, a=None, rows: int = 0, cols: int = 0):
    _req(u, BF16, "u", 2)
    if u.shape[0] != dx.shape[0] or u.shape[1] < K or dx.shape[1] < K:
        raise ValueError(f"u {tuple(u.shape)} / dx {tuple(dx.shape)}: expected {dx.shape[0]} rows of at least K = {K} columns")
    if dt is not None and (dt.shape[0] != dx.shape[0] or dt.shape[1] < cols or a.shape[0] < rows or a.shape[1] < K):
        raise ValueError(f"dt {tuple(dt.shape)} / a {tuple(a.shape)}: expected dt [{dx.shape[0]}, >= {cols}] and a [>= {rows}, >= {K}]")


def lora_up_add_dgelu_drop(dx, dt, a, R: int, n_adapters: int, u, K: int, p: float, seed: int, site0: int):
    """dx[:, :K] += gelu'(u[:, :K]) / (1-p) * sum_j keep_j * (dt[:, j r:(j+1) r] @ a[j r:(j+1) r]) in place: the dropped dX correction of
    adapters whose input is gelu(u) (ff.net.2), added to a dx that already carries the factor gelu'(u)."""
    _req(dx, BF16, "dx", 2); _req(dt, BF16, "dt", 2); _req(a, BF16, "a", 2); _req_preact(u, dx, K, dt, a, R, R)
    check(load_library().vt_lora_up_add_dgelu_drop(dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), a.data_ptr(), a.stride(0),
                                                   R, n_adapters, u.data_ptr(), u.stride(0), dx.shape[0], K, float(p), int(seed) & _U64,
                                                   site0, _stream()), "vt_lora_up_add_dgelu_drop")


def lora_up_add_wide_dgelu_drop(dx, dt, a, n_adapters: int, r: int, rp: int, u, K: int, p: float, seed: int, site0: int):
    """lora_up_add_dgelu_drop in the wide layout (adapter j = columns [j rp, j rp + r) of dt)."""
    _req(dx, BF16, "dx", 2); _req(dt, BF16, "dt", 2); _req(a, BF16, "a", 2)
    _req_preact(u, dx, K, dt, a, n_adapters * r, n_adapters * rp)
    check(load_library().vt_lora_up_add_wide_dgelu_drop(dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), a.data_ptr(),
                                                        a.stride(0), n_adapters, r, rp, u.data_ptr(), u.stride(0), dx.shape[0], K,
                                                        float(p), int(seed) & _U64, site0, _stream()),
          "vt_lora_up_add_wide_dgelu_drop")


# ---- the wide _drop products with an origin map (HunyuanVideo): the call's operand is a piece of the adapter's logical input ----
# origin = (seg_local, seg_global, n_first, off_first, off_rest, k0, K_log): row m of the call (b = m // seg_local, l = m % seg_local) is
# row m_g = b * seg_global + l + (off_first if l < n_first else off_rest) and column k is column k0 + k of the logical [M_g, K_log] input;
# the mask element is e = m_g * K_log + k0 + k.  (M, M, 0, 0, 0, 0, K) is the identity: the plain _drop call.  A bad map raises VtError
# before any launch.
def _origin(origin):
    sl, sg, nf, of, orr, k0, klog = (int(v) for v in origin)
    return sl, sg, nf, of, orr, k0, klog


def lora_down_wide_drop_at(x, a, n_adapters: int, r: int, rp: int, ext: int, t_out, K: int, p: float, seed: int, site0: int, origin):
    _req(x, BF16, "x", 2); _req(a, BF16, "a", 2); _req(t_out, BF16, "t", 2)
    check(load_library().vt_lora_down_wide_drop_at(x.data_ptr(), x.stride(0), a.data_ptr(), a.stride(0), n_adapters, r, rp, ext,
                                                   t_out.data_ptr(), t_out.stride(0), x.shape[0], K, float(p), int(seed) & _U64, site0,
                                                   *_origin(origin), _stream()), "vt_lora_down_wide_drop_at")


def lora_tn_wide_drop_at(big, small, R: int, out, osp: int, osr: int, alpha: float, P: int, p: float, seed: int, site: int, origin):
    _req(big, BF16, "big", 2); _req(small, BF16, "small", 2); _req(out, torch.float32, "out")
    check(load_library().vt_lora_tn_wide_drop_at(big.data_ptr(), big.stride(0), small.data_ptr(), small.stride(0), R, out.data_ptr(),
                                                 osp, osr, alpha, big.shape[0], P, float(p), int(seed) & _U64, site, *_origin(origin),
                                                 _stream()), "vt_lora_tn_wide_drop_at")


def lora_up_add_wide_drop_at(dx, dt, a, n_adapters: int, r: int, rp: int, K: int, p: float, seed: int, site0: int, origin):
    _req(dx, BF16, "dx", 2); _req(dt, BF16, "dt", 2); _req(a, BF16, "a", 2)
    check(load_library().vt_lora_up_add_wide_drop_at(dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), a.data_ptr(), a.stride(0),
                                                     n_adapters, r, rp, dx.shape[0], K, float(p), int(seed) & _U64, site0,
                                                     *_origin(origin), _stream()), "vt_lora_up_add_wide_drop_at")


def lora_up_add_wide_dgelu_drop_at(dx, dt, a, n_adapters: int, r: int, rp: int, u, K: int, p: float, seed: int, site0: int, origin):
    _req(dx, BF16, "dx", 2); _req(dt, BF16, "dt", 2); _req(a, BF16, "a", 2)
    _req_preact(u, dx, K, dt, a, n_adapters * r, n_adapters * rp)
    check(load_library().vt_lora_up_add_wide_dgelu_drop_at(dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), a.data_ptr(),
                                                           a.stride(0), n_adapters, r, rp, u.data_ptr(), u.stride(0), dx.shape[0], K,
                                                           float(p), int(seed) & _U64, site0, *_origin(origin), _stream()),
          "vt_lora_up_add_wide_dgelu_drop_at")


# ---- DoRA (use_dora, csrc/dora.hip): c = m / ||W + s B A|| per output feature, folded into the packed operands ----
def dora_norm(w, a, b, n_adapters: int, r: int, scale: float, out, mag=None):
    """out[j] = ||w[j] + scale * b[j] @ a||_2, or mag[j] / that norm when mag is given.  w bf16 [n d_out, K], a bf16 [n r, K], b bf16
    [n d_out, r] contiguous (adapter j: rows [j d_out, (j+1) d_out) of w and b, rows [j r, (j+1) r) of a); out, mag fp32 [n d_out]."""
    _req(w, BF16, "w", 2); _req(a, BF16, "a", 2); _req(b, BF16, "b", 2); _req(out, torch.float32, "out", 1)
    N, K = w.shape
    if mag is not None:
        _req(mag, torch.float32, "mag", 1)
    if (N % n_adapters or a.shape[0] < n_adapters * r or a.shape[1] < K or b.shape[0] != N or b.shape[1] != r or not b.is_contiguous()
            or out.numel() < N or (mag is not None and mag.numel() < N)):
        raise ValueError(f"dora_norm: w {tuple(w.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)}, out {tuple(out.shape)} do not fit "
                         f"{n_adapters} adapter(s) of rank {r}")
    check(load_library().vt_dora_norm(w.data_ptr(), w.stride(0), a.data_ptr(), a.stride(0), b.data_ptr(), n_adapters, N // n_adapters, r, K,
                                      float(scale), _p(mag), out.data_ptr(), _stream()), "vt_dora_norm")


def dora_scale(src, dst, c, by_col: bool = False):
    """dst[j, k] = bf16(c[k if by_col else j] * src[j, k]), rounded once; dst may be src (2-d row-strided views of equal shape)"""
    _req(src, BF16, "src", 2); _req(dst, BF16, "dst", 2); _req(c, torch.float32, "c", 1)
    rows, cols = src.shape
    if tuple(dst.shape) != (rows, cols) or c.numel() < (cols if by_col else rows):
        raise ValueError(f"dora_scale: src {tuple(src.shape)}, dst {tuple(dst.shape)}, c {tuple(c.shape)}")
    check(load_library().vt_dora_scale(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), c.data_ptr(), rows, cols, int(by_col),
                                       _stream()), "vt_dora_scale")


def dora_transpose_scale(src, dst, c):
    """dst[k, j] = bf16(c[j] * src[j, k]): src [N, K], dst [K, N] (row-strided views allowed), c fp32 [N]"""
    _req(src, BF16, "src", 2); _req(dst, BF16, "dst", 2); _req(c, torch.float32, "c", 1)
    rows, cols = src.shape
    if tuple(dst.shape) != (cols, rows) or c.numel() < rows:
        raise ValueError(f"dora_transpose_scale: src {tuple(src.shape)}, dst {tuple(dst.shape)}, c {tuple(c.shape)}")
    check(load_library().vt_dora_transpose_scale(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), c.data_ptr(), rows, cols,
                                                 _stream()), "vt_dora_transpose_scale")


def dora_db_add(g, s, c):
    """g[j, i] += c[j] * s[j, i]: contiguous fp32 [N, r] pair, c fp32 [N]"""
    _req(g, torch.float32, "g", 2); _req(s, torch.float32, "s", 2); _req(c, torch.float32, "c", 1)
    if tuple(g.shape) != tuple(s.shape) or not g.is_contiguous() or not s.is_contiguous() or c.numel() < g.shape[0]:
        raise ValueError(f"dora_db_add: g {tuple(g.shape)}, s {tuple(s.shape)}, c {tuple(c.shape)}")
    check(load_library().vt_dora_db_add(g.data_ptr(), s.data_ptr(), c.data_ptr(), g.shape[0], g.shape[1], _stream()), "vt_dora_db_add")


def dora_dm(sum_g, sum_gy, bias, mag, dm):
    """dm[j] += (sum_gy[j] - bias[j] * sum_g[j]) / mag[j]; fp32 vectors of one length, bias bf16 or None"""
    for n, t in (("sum_g", sum_g), ("sum_gy", sum_gy), ("mag", mag), ("dm", dm)):
        _req(t, torch.float32, n, 1)
    if bias is not None:
        _req(bias, BF16, "bias", 1)
    N = dm.numel()
    if sum_g.numel() < N or sum_gy.numel() < N or mag.numel() < N or (bias is not None and bias.numel() < N):
        raise ValueError("dora_dm: a vector is shorter than dm")
    check(load_library().vt_dora_dm(sum_g.data_ptr(), sum_gy.data_ptr(), _p(bias), mag.data_ptr(), dm.data_ptr(), N, _stream()), "vt_dora_dm")


# =====================================================================================================================
# VideoCrafter2 UNet path (include/vt355.h, second half): channels-last [N, T, H, W, C] activations
# =====================================================================================================================
def pack_conv_weight_nd(w: torch.Tensor) -> torch.Tensor:
    """torch conv weight [Cout, Cin, *k] (Conv2d [.,.,KH,KW] or Conv3d [.,.,KT,KH,KW]) -> [Cout, taps*Cin], tap-major, ci innermost"""
    if w.dim() == 4:
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()
    if w.dim() == 5:
        return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1).contiguous()
    raise ValueError(f"expected a 4-d or 5-d conv weight, got {tuple(w.shape)}")


def transpose(w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w bf16 [R, C] (row-strided view allowed) -> contiguous [C, R]: the W^T operand of a Linear's input gradient (vt_transpose_bf16)"""
    _req(w, BF16, "w", 2)
    R, C_ = w.shape
    if R % 8 or C_ % 8 or w.stride(0) % 8 or w.data_ptr() % 16 or os.environ.get("VT355_TORCH_TRANSPOSE") == "1":
        return w.t().contiguous()
    out = torch.empty(C_, R, dtype=BF16, device=w.device) if out is None else out
    check(load_library().vt_transpose_bf16(w.data_ptr(), w.stride(0), 0, out.data_ptr(), R, 0, R, C_, 1, _stream()), "vt_transpose_bf16")
    return out


class TransposePlan:
    """A fixed set of bf16 transposes run as ONE launch (vt_transpose_multi_bf16): the per-step operand packing of a model under full
    fine-tuning (W^T of every Linear, the input-gradient weight of every convolution).  Sources and destinations are persistent buffers
    (parameter views / operands allocated once); build the plan once, ``run()`` after every optimizer step.

    add(src [R, C] view, dst [C, R] contiguous) queues dst = src^T; add_conv_dx(ws [Cout, taps, Cin], dst [Cin, taps * Cout]) queues the
    taps of a convolution's input-gradient weight (tap t lands, transposed, at tap taps - 1 - t).  False: this operand does not meet the
    kernel's alignment (multiples of 8, 16-byte pointers) and stays with the caller's own path."""

    def __init__(self, device):
        self.device, self.jobs, self.blocks, self.table, self.keep = device, [], 0, None, []

    def _job(self, src_ptr, dst_ptr, src_ld, dst_ld, rows, cols):
        tx, ty = (cols + 63) // 64, (rows + 63) // 64
        self.jobs.append([src_ptr, dst_ptr, src_ld, dst_ld, rows, cols, self.blocks, tx])
        self.blocks += tx * ty
        self.table = None

    def add(self, src: torch.Tensor, dst: torch.Tensor) -> bool:
        _req(src, BF16, "src", 2); _req(dst, BF16, "dst", 2)
        R, C_ = src.shape
        if tuple(dst.shape) != (C_, R) or not dst.is_contiguous():
            raise ValueError(f"dst must be contiguous [{C_}, {R}]")
        if R % 8 or C_ % 8 or src.stride(0) % 8 or src.stride(0) < C_ or src.data_ptr() % 16 or dst.data_ptr() % 16:
            return False
        self._job(src.data_ptr(), dst.data_ptr(), src.stride(0), R, R, C_)
        self.keep += [src, dst]
        return True

    def add_conv_dx(self, ws: torch.Tensor, dst: torch.Tensor) -> bool:
        _req(ws, BF16, "ws", 3); _req(dst, BF16, "dst", 2)
        Cout, taps, Cin = ws.shape
        if tuple(dst.shape) != (Cin, taps * Cout) or not dst.is_contiguous():
            raise ValueError(f"dst must be contiguous [{Cin}, {taps * Cout}]")
        if not ws.is_contiguous() or Cout % 8 or Cin % 8 or ws.data_ptr() % 16 or dst.data_ptr() % 16:
            return False
        for t in range(taps):
            self._job(ws.data_ptr() + t * Cin * 2, dst.data_ptr() + (taps - 1 - t) * Cout * 2, taps * Cin, taps * Cout, Cout, Cin)
        self.keep += [ws, dst]
        return True

    def run(self):
        if not self.jobs:
            return
        if self.table is None:
            self.table = torch.tensor(self.jobs, dtype=torch.int64).to(self.device)
        check(load_library().vt_transpose_multi_bf16(self.table.data_ptr(), len(self.jobs), self.blocks, _stream()), "vt_transpose_multi_bf16")


def conv_weight_dx_from_storage(ws: torch.Tensor) -> torch.Tensor:
    """ws: a conv weight in its tap-major storage [Cout, taps, Cin] (contiguous) -> the weight of the input-gradient convolution of a
    stride-1 'same' conv, [Cin, taps * Cout] with the taps flipped (= pack_conv_weight_dx of the logical [Cout, Cin, *k] weight): one
    batched transpose, tap t of the source lands at tap taps-1-t of the result"""
    _req(ws, BF16, "ws", 3)
    Cout, taps, Cin = ws.shape
    if os.environ.get("VT355_TORCH_TRANSPOSE") == "1":         # A/B: the three strided torch copies this replaced
        return ws.flip(1).permute(2, 1, 0).reshape(Cin, taps * Cout).contiguous()
    if not ws.is_contiguous() or Cout % 8 or Cin % 8 or ws.data_ptr() % 16:
        raise ValueError("conv weight storage must be contiguous [Cout, taps, Cin] with Cout, Cin multiples of 8")
    out = torch.empty(Cin, taps * Cout, dtype=BF16, device=ws.device)
    check(load_library().vt_transpose_bf16(ws.data_ptr(), taps * Cin, Cin, out.data_ptr() + (taps - 1) * Cout * 2, taps * Cout, -Cout, Cout, Cin, taps,
                                           _stream()), "vt_transpose_bf16")
    return out


def pack_conv_weight_dx(w: torch.Tensor) -> torch.Tensor:
    """weight of the INPUT-gradient convolution of a stride-1 'same' conv: taps flipped, in / out channels swapped:
    [Cout, Cin, *k] -> [Cin, taps * Cout]"""
    dims = tuple(range(2, w.dim()))
    return pack_conv_weight_nd(w.flip(dims).transpose(0, 1))


def conv_cl(x, wk, y, kernel, padding, stride: int = 1, bias=None, sbias=None, residual=None):
    """x bf16 [N,T,H,W,Cin], wk bf16 [Cout, KT*KH*KW*Cin], y bf16 [N,T,Ho,Wo,Cout]; kernel = (KT,KH,KW), padding = (pt,ph,pw);
    bias bf16 [Cout]; sbias fp32 [N, >=Cout] per-sample bias; residual like y"""
    _req(x, BF16, "x", 5); _req(y, BF16, "y", 5); _req(wk, BF16, "wk", 2)
    N, T, H, W, Cin = x.shape
    Cout = y.shape[4]
    KT, KH, KW = kernel
    pt, ph, pw = padding
    Ho, Wo = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
    if tuple(y.shape[:4]) != (N, T, Ho, Wo) or tuple(wk.shape) != (Cout, KT * KH * KW * Cin) or not wk.is_contiguous():
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} wk {tuple(wk.shape)} y {tuple(y.shape)} (expected y {(N, T, Ho, Wo, Cout)})")
    _cl_check(x, "x"); _cl_check(y, "y")
    if residual is not None:
        _req(residual, BF16, "residual", 5); _cl_check(residual, "residual")
        if tuple(residual.shape) != tuple(y.shape):
            raise ValueError("residual must have the shape of y")
    if sbias is not None:
        _req(sbias, torch.float32, "sbias", 2)
        if sbias.shape[0] != N or sbias.shape[1] < Cout:
            raise ValueError(f"sbias must be [N, >=Cout], got {tuple(sbias.shape)}")
    with _timed("conv", 2.0 * N * T * Ho * Wo * Cout * KT * KH * KW * Cin):
        check(load_library().vt_conv_cl(x.data_ptr(), x.stride(3), wk.data_ptr(), _p(bias), _p(sbias), 0 if sbias is None else sbias.stride(0),
                                        _p(residual), 0 if residual is None else residual.stride(3), y.data_ptr(), y.stride(3),
                                        N, T, H, W, Cin, Cout, KT, KH, KW, pt, ph, pw, stride, _stream()), "vt_conv_cl")
    return y


def rows320(n_out: int, M: int, K: int) -> bool:
    """a Linear that the 128 x 320 persistent convolution kernel (as a 1x1 convolution) runs faster than vt_gemm_bf16: outputs a multiple of 320
    that is not a multiple of 128 (320: 2.5 GEMM tiles, 960: 7.5), enough rows to fill the chip (profiles/r03_lin320_kbench.txt: 149 -> 121 us at
    163 840 x 320 x 320 with a residual)"""
    if os.environ.get("VT355_ROWS320") == "0":        # A/B: always vt_gemm_bf16
        return False
    return n_out % 320 == 0 and n_out % 128 != 0 and K % 64 == 0 and M * (n_out // 320) >= 128 * 256


def linear_rows(x, w, y, bias=None, residual=None):
    """y[M, N] = x[M, K] w[N, K]^T + bias (+ residual) through vt_conv_cl as a 1x1 convolution over M positions (bit-identical to vt_gemm_bf16's
    result: same products, same fp32 sums)"""
    _req(x, BF16, "x", 2); _req(w, BF16, "w", 2); _req(y, BF16, "y", 2)
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or not w.is_contiguous() or tuple(y.shape) != (M, N):
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} w {tuple(w.shape)} y {tuple(y.shape)}")
    if residual is not None:
        _req(residual, BF16, "residual", 2)
    with _timed("gemm", 2.0 * M * N * K):
        check(load_library().vt_conv_cl(x.data_ptr(), x.stride(0), w.data_ptr(), _p(bias), None, 0, _p(residual), 0 if residual is None else residual.stride(0),
                                        y.data_ptr(), y.stride(0), 1, 1, 1, M, K, N, 1, 1, 1, 0, 0, 0, 1, _stream()), "vt_conv_cl")
    return y


def conv_dw_cl(dy, x, dw, kernel, padding, stride: int = 1, accumulate: bool = True, dbias: Optional[torch.Tensor] = None):
    """dw fp32 [Cout, taps*Cin] (+)= conv weight gradient; dy bf16 [N,T,Ho,Wo,Cout], x bf16 [N,T,H,W,Cin]; dbias fp32 [Cout] += column sums
    of dy (the bias gradient: out of the same pass over dy when Cout % 320 == 0)"""
    _req(x, BF16, "x", 5); _req(dy, BF16, "dy", 5); _req(dw, torch.float32, "dw", 2)
    N, T, H, W, Cin = x.shape
    Cout = dy.shape[4]
    KT, KH, KW = kernel
    pt, ph, pw = padding
    if tuple(dw.shape) != (Cout, KT * KH * KW * Cin) or not dw.is_contiguous():
        raise ValueError(f"dw must be contiguous [{Cout}, {KT * KH * KW * Cin}], got {tuple(dw.shape)}")
    _cl_check(x, "x"); _cl_check(dy, "dy")
    with _timed("conv_dw", 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * dy.shape[3] * Cout * KT * KH * KW * Cin):
        if dbias is not None:
            _req(dbias, torch.float32, "dbias", 1)
            if dbias.numel() != Cout or not dbias.is_contiguous():
                raise ValueError(f"dbias must be contiguous [{Cout}]")
            if os.environ.get("VT355_FUSED_DBIAS") == "0":      # A/B: the separate column-sum pass
                group_colsum(dy.as_strided((N * T * dy.shape[2] * dy.shape[3], Cout), (dy.stride(3), 1)), dbias, D=Cout)
                dbias = None
        check(load_library().vt_conv_dw_bias_cl(dy.data_ptr(), dy.stride(3), x.data_ptr(), x.stride(3), dw.data_ptr(), _p(dbias), N, T, H, W, Cin, Cout,
                                                KT, KH, KW, pt, ph, pw, stride, int(accumulate), _stream()), "vt_conv_dw_bias_cl")


def linear_dw(dy, x, dw, accumulate: bool = True, dbias: Optional[torch.Tensor] = None):
    """dw fp32 [N_out, K] (+)= dy[M, N_out]^T x[M, K] for any multiple-of-8 sizes (one-tap vt_conv_dw_cl); dbias fp32 [N_out] += column sums of dy"""
    _req(dy, BF16, "dy", 2); _req(x, BF16, "x", 2); _req(dw, torch.float32, "dw", 2)
    M, P = dy.shape
    Q = x.shape[1]
    if x.shape[0] != M or tuple(dw.shape) != (P, Q) or not dw.is_contiguous():
        raise ValueError(f"shape mismatch: dy {tuple(dy.shape)} x {tuple(x.shape)} dw {tuple(dw.shape)}")
    if dbias is not None:
        _req(dbias, torch.float32, "dbias", 1)
        if dbias.numel() != P or not dbias.is_contiguous():
            raise ValueError(f"dbias must be contiguous [{P}]")
        if os.environ.get("VT355_FUSED_DBIAS") == "0":
            group_colsum(dy, dbias, D=P)
            dbias = None
    check(load_library().vt_conv_dw_bias_cl(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), _p(dbias), 1, 1, 1, M, Q, P,
                                            1, 1, 1, 0, 0, 0, 1, int(accumulate), _stream()), "vt_conv_dw_bias_cl")


def groupnorm_fwd(x, gamma, beta, y, groups: int, eps: float, silu: bool):
    """like groupnorm_silu but returns the workspace (statistics) the backward needs"""
    N, P, C = x.shape
    ws = torch.empty(int(load_library().vt_groupnorm_ws_bytes(N, C)) // 4, dtype=torch.float32, device=x.device)
    groupnorm_silu(x, gamma, beta, y, groups, eps, silu, ws)
    return ws


def groupnorm_bwd(dy, x, gamma, ws_fwd, dx, dgamma, dbeta, groups: int, silu: bool, accumulate: bool = False):
    """dy, x, dx bf16 [N, P, C]; dgamma / dbeta fp32 [C] accumulated (or None)"""
    _req(dy, BF16, "dy", 3); _req(x, BF16, "x", 3); _req(dx, BF16, "dx", 3)
    N, P, C = x.shape
    for t_, nm in ((x, "x"), (dy, "dy"), (dx, "dx")):
        if t_.stride(0) != P * t_.stride(1):
            raise ValueError(f"{nm}: samples must be P positions apart")
    wsb = torch.empty_like(ws_fwd)
    check(load_library().vt_groupnorm_silu_bwd_cl(dy.data_ptr(), dy.stride(1), x.data_ptr(), x.stride(1), _p(gamma), ws_fwd.data_ptr(),
                                                  wsb.data_ptr(), wsb.numel() * 4, dx.data_ptr(), dx.stride(1), _p(dgamma), _p(dbeta),
                                                  N, P, C, groups, int(silu), int(accumulate), _stream()), "vt_groupnorm_silu_bwd_cl")


def dropout(x, y, p: float, seed: int, offset: int = 0, mask_out=None):
    """y = keep ? x / (1 - p) : 0 on bf16 rows [M, C] (y may alias x); keep is a pure function of (seed, offset, element index): the
    backward pass is the same call on the gradient.  mask_out: uint8 [M, C] keep flags (tests)."""
    _req(x, BF16, "x", 2); _req(y, BF16, "y", 2)
    _rows_cols(y, x.shape[0], x.shape[1], "y", "dropout")
    if mask_out is not None and (mask_out.dtype != torch.uint8 or not mask_out.is_contiguous() or tuple(mask_out.shape) != tuple(x.shape)):
        raise ValueError("mask_out must be a contiguous uint8 tensor of x's shape")
    check(load_library().vt_dropout_bf16(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), x.shape[0], x.shape[1], float(p),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, _p(mask_out), _stream()), "vt_dropout_bf16")


def geglu_fwd(h, y):
    _req(h, BF16, "h", 2); _req(y, BF16, "y", 2)
    if h.shape[1] != 2 * y.shape[1]:
        raise ValueError(f"geglu_fwd: h {tuple(h.shape)} is not (a | gate) of twice y's width {y.shape[1]}")
    _rows_cols(y, h.shape[0], y.shape[1], "y", "geglu_fwd")
    check(load_library().vt_geglu_fwd(h.data_ptr(), h.stride(0), y.data_ptr(), y.stride(0), h.shape[0], y.shape[1], _stream()), "vt_geglu_fwd")


def geglu_bwd(dy, h, dh):
    _req(h, BF16, "h", 2); _req(dy, BF16, "dy", 2); _req(dh, BF16, "dh", 2)
    if h.shape[1] != 2 * dy.shape[1]:
        raise ValueError(f"geglu_bwd: h {tuple(h.shape)} is not (a | gate) of twice dy's width {dy.shape[1]}")
    _rows_cols(dy, h.shape[0], dy.shape[1], "dy", "geglu_bwd"); _rows_cols(dh, h.shape[0], h.shape[1], "dh", "geglu_bwd")
    check(load_library().vt_geglu_bwd(dy.data_ptr(), dy.stride(0), h.data_ptr(), h.stride(0), dh.data_ptr(), dh.stride(0), h.shape[0],
                                      dy.shape[1], _stream()), "vt_geglu_bwd")


def add_rows(a, b, out):
    """out = a + b on 2-d bf16 row views (out may be a or b)"""
    _req(a, BF16, "a", 2); _req(b, BF16, "b", 2); _req(out, BF16, "out", 2)
    _rows_cols(b, a.shape[0], a.shape[1], "b", "add_rows"); _rows_cols(out, a.shape[0], a.shape[1], "out", "add_rows")
    check(load_library().vt_add_rows_bf16(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), a.shape[0],
                                          a.shape[1], _stream()), "vt_add_rows_bf16")


def row_map(src, out, mode: int, nb: int, d1: int, d2: int, accumulate: bool = False):
    """2-d bf16 row views; mode 0: [nb,d1,d2] -> [nb,d2,d1]; 1: nearest x2; 2: zero insertion; 3: 2x2 block sum (see vt355.h)"""
    _req(src, BF16, "src", 2); _req(out, BF16, "out", 2)
    rows_src = nb * d1 * d2 * (4 if mode == 3 else 1)
    rows_out = nb * d1 * d2 * (4 if mode in (1, 2) else 1)
    if src.shape[0] != rows_src or out.shape[0] != rows_out or src.shape[1] != out.shape[1]:
        raise ValueError(f"row_map mode {mode}: src {tuple(src.shape)} out {tuple(out.shape)} do not match nb={nb} d1={d1} d2={d2}")
    check(load_library().vt_row_map_bf16(src.data_ptr(), src.stride(0), out.data_ptr(), out.stride(0), mode, nb, d1, d2, src.shape[1],
                                         int(accumulate), _stream()), "vt_row_map_bf16")


def q_sample(x0, noise, sa, sb, scale, xt):
    _req(x0, torch.float32, "x0"); _req(noise, torch.float32, "noise"); _req(xt, BF16, "xt")
    B = x0.shape[0]
    _numel(noise, x0.numel(), "noise", "q_sample"); _numel(xt, x0.numel(), "xt", "q_sample")
    _numel(sa, B, "sa", "q_sample"); _numel(sb, B, "sb", "q_sample"); _numel(scale, B, "scale", "q_sample")
    check(load_library().vt_q_sample(x0.data_ptr(), noise.data_ptr(), sa.data_ptr(), sb.data_ptr(), _p(scale), xt.data_ptr(),
                                     x0.numel() // B, B, _stream()), "vt_q_sample")


def mse_loss(pred, target, loss, dpred=None, grad_scale: float = 1.0):
    _req(pred, BF16, "pred"); _req(target, torch.float32, "target"); _req(loss, torch.float32, "loss")
    _numel(target, pred.numel(), "target", "mse_loss"); _numel(dpred, pred.numel(), "dpred", "mse_loss"); _numel(loss, 1, "loss", "mse_loss")
    check(load_library().vt_mse_loss(pred.data_ptr(), target.data_ptr(), loss.data_ptr(), _p(dpred), pred.numel(), grad_scale, _stream()),
          "vt_mse_loss")


def attn_small_fwd(q, k, v, o, lse2, H: int, scale: float, mask_block: int = 0):
    """q, o: [NB, Sq, >=H*64]; k, v: [NB, Sk, >=H*64] views (mask_block > 0: NB == 1, one packed row space)"""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        _req(t, BF16, n, 3)
    NB, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    check(load_library().vt_attn_small_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _p(lse2), NB, H, Sq, Sk,
                                           q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0),
                                           o.stride(1), o.stride(0), scale, mask_block, _stream()), "vt_attn_small_fwd")


def attn_small_bwd(q, k, v, o, do, lse2, dq, dk, dv, H: int, scale: float, mask_block: int = 0):
    """mask_block > 0: dk, dv bf16 like k, v.  mask_block == 0: dk, dv fp32 [NB, Sk, H*64] contiguous, zeroed here, accumulated with atomics."""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o), ("do", do), ("dq", dq)):
        _req(t, BF16, n, 3)
    NB, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    if mask_block > 0:
        _req(dk, BF16, "dk", 3); _req(dv, BF16, "dv", 3)
        args = (dk.data_ptr(), dv.data_ptr(), None, None)
    else:
        _req(dk, torch.float32, "dk", 3); _req(dv, torch.float32, "dv", 3)
        if not (dk.is_contiguous() and dv.is_contiguous()):
            raise ValueError("dk / dv accumulators must be contiguous")
        dk.zero_(); dv.zero_()
        args = (None, None, dk.data_ptr(), dv.data_ptr())
    check(load_library().vt_attn_small_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse2.data_ptr(),
                                           dq.data_ptr(), *args, NB, H, Sq, Sk,
                                           q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0),
                                           o.stride(1), o.stride(0), do.stride(1), do.stride(0), dq.stride(1), dq.stride(0),
                                           dk.stride(1), dv.stride(1), scale, mask_block, _stream()), "vt_attn_small_bwd")


_RELPOS_WS = {}


def _relpos_args(H: int, T: int, rel_k, rel_v, rows):
    for n, t in rows:
        _req(t, BF16, n, 2)
        if t.stride(1) != 1 or t.shape[1] < H * 64:
            raise ValueError(f"attn_relpos: {n} must be a [R, >= H*64] view with unit column stride")
    _req(rel_k, BF16, "rel_k", 2); _req(rel_v, BF16, "rel_v", 2)
    if rel_k.shape != rel_v.shape or rel_k.shape[1] != 64 or rel_k.shape[0] % 2 != 1 or not (rel_k.is_contiguous() and rel_v.is_contiguous()):
        raise ValueError("attn_relpos: rel_k / rel_v must be contiguous [2P+1, 64] tables")
    return rows[0][1].shape[0], (rel_k.shape[0] - 1) // 2


def attn_relpos_fwd(q, k, v, rel_k, rel_v, o, lse2, H: int, T: int, scale: float):
    """packed temporal self-attention with relative-position tables: q, k, v, o [R, >= H*64] views of one row space (R / T sequences of
    T rows), rel_k / rel_v bf16 [2P+1, 64], lse2 fp32 [H, R]"""
    R, P = _relpos_args(H, T, rel_k, rel_v, (("q", q), ("k", k), ("v", v), ("o", o)))
    _req(lse2, torch.float32, "lse2")
    check(load_library().vt_attn_relpos_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), rel_k.data_ptr(), rel_v.data_ptr(), o.data_ptr(),
                                            lse2.data_ptr(), R, H, T, P, q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale,
                                            _stream()), "vt_attn_relpos_fwd")


def attn_relpos_bwd(q, k, v, rel_k, rel_v, o, do, lse2, dq, dk, dv, d_rel_k, d_rel_v, H: int, T: int, scale: float):
    """dq, dk, dv bf16 like q, k, v (written whole); d_rel_k / d_rel_v fp32 [2P+1, 64] or None: the table gradients are ADDED into them
    (fp32 atomics: not bitwise reproducible); both None (frozen tables) skips the table-gradient pass"""
    R, P = _relpos_args(H, T, rel_k, rel_v, (("q", q), ("k", k), ("v", v), ("o", o), ("do", do), ("dq", dq), ("dk", dk), ("dv", dv)))
    _req(lse2, torch.float32, "lse2")
    lib = load_library()
    for n, t in (("d_rel_k", d_rel_k), ("d_rel_v", d_rel_v)):
        if t is not None:
            _req(t, torch.float32, n, 2)
            if tuple(t.shape) != tuple(rel_k.shape) or not t.is_contiguous():
                raise ValueError(f"attn_relpos: {n} must be a contiguous fp32 [2P+1, 64] accumulator")
    ws = None
    if d_rel_k is not None or d_rel_v is not None:
        if q.device not in _RELPOS_WS:              # per-device scratch of the table-gradient reduction, reused across calls (stream-ordered)
            _RELPOS_WS[q.device] = torch.empty(lib.vt_attn_relpos_workspace_bytes() // 4, dtype=torch.float32, device=q.device)
        ws = _RELPOS_WS[q.device]
    check(lib.vt_attn_relpos_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), rel_k.data_ptr(), rel_v.data_ptr(), o.data_ptr(), do.data_ptr(),
                                 lse2.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _p(d_rel_k), _p(d_rel_v), _p(ws),
                                 R, H, T, P, q.stride(0), k.stride(0), v.stride(0), o.stride(0), do.stride(0), dq.stride(0),
                                 dk.stride(0), dv.stride(0), scale, _stream()), "vt_attn_relpos_bwd")


def attn_dual_ws_floats(B: int, H: int, Sq: int, rows_per_frame: int, Sa: int, Sb: int) -> int:
    n = load_library().vt_attn_dual_ws_floats(B, H, Sq, rows_per_frame, Sa, Sb)
    if n < 0:
        raise ValueError(f"attn_dual: rows_per_frame {rows_per_frame} does not divide Sq {Sq}")
    return n


def _attn_dual_shapes(q, k, k_ip, rows_per_frame):
    B, Sq, Sa, Sb = q.shape[0], q.shape[1], k.shape[1], k_ip.shape[1]
    if rows_per_frame <= 0 or Sq % rows_per_frame or k.shape[0] != B or k_ip.shape[0] != B * (Sq // rows_per_frame):
        raise ValueError(f"attn_dual: q {tuple(q.shape)}, k {tuple(k.shape)}, k_ip {tuple(k_ip.shape)} do not fit rows_per_frame={rows_per_frame}")
    return B, Sq, Sa, Sb


def attn_dual_fwd(q, k, v, k_ip, v_ip, o, lse2, H: int, scale: float, rows_per_frame: int, img_scale: float = 1.0):
    """q, o: [B, Sq, >=H*64]; text k, v: [B, Sa<=96, >=H*64]; image k_ip, v_ip: [B*Sq/rows_per_frame, Sb<=32, >=H*64]; lse2 fp32 [2, B, H, Sq]"""
    for n, t in (("q", q), ("k", k), ("v", v), ("k_ip", k_ip), ("v_ip", v_ip), ("o", o)):
        _req(t, BF16, n, 3)
    B, Sq, Sa, Sb = _attn_dual_shapes(q, k, k_ip, rows_per_frame)
    if v.shape[:2] != k.shape[:2] or v_ip.shape[:2] != k_ip.shape[:2] or o.shape[:2] != q.shape[:2]:
        raise ValueError("attn_dual_fwd: v / v_ip / o do not match k / k_ip / q")
    if lse2 is not None:
        _req(lse2, torch.float32, "lse2")
        if tuple(lse2.shape) != (2, B, H, Sq) or not lse2.is_contiguous():
            raise ValueError(f"attn_dual_fwd: lse2 must be contiguous [2, {B}, {H}, {Sq}]")
    check(load_library().vt_attn_dual_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), k_ip.data_ptr(), v_ip.data_ptr(), o.data_ptr(), _p(lse2),
                                          B, H, Sq, rows_per_frame, Sa, Sb,
                                          q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0),
                                          k_ip.stride(1), k_ip.stride(0), v_ip.stride(1), v_ip.stride(0), o.stride(1), o.stride(0),
                                          scale, img_scale, _stream()), "vt_attn_dual_fwd")


def attn_dual_bwd(q, k, v, k_ip, v_ip, do, lse2, dq, dk, dv, dk_ip, dv_ip, H: int, scale: float, rows_per_frame: int,
                  img_scale: float = 1.0, ws=None):
    """dq bf16 like q; dk, dv fp32 [B, Sa, H*64] and dk_ip, dv_ip fp32 [B*Sq/rows_per_frame, Sb, H*64], contiguous, fully written.
    ws: fp32 scratch of attn_dual_ws_floats(...) elements (allocated here when None)."""
    for n, t in (("q", q), ("k", k), ("v", v), ("k_ip", k_ip), ("v_ip", v_ip), ("do", do), ("dq", dq)):
        _req(t, BF16, n, 3)
    B, Sq, Sa, Sb = _attn_dual_shapes(q, k, k_ip, rows_per_frame)
    D = H * 64
    for n, t, shp in (("dk", dk, (B, Sa, D)), ("dv", dv, (B, Sa, D)), ("dk_ip", dk_ip, (k_ip.shape[0], Sb, D)), ("dv_ip", dv_ip, (k_ip.shape[0], Sb, D))):
        _req(t, torch.float32, n, 3)
        if tuple(t.shape) != shp or not t.is_contiguous():
            raise ValueError(f"attn_dual_bwd: {n} must be contiguous fp32 {shp}, got {tuple(t.shape)}")
    if do.shape[:2] != q.shape[:2] or dq.shape[:2] != q.shape[:2]:
        raise ValueError("attn_dual_bwd: do / dq do not match q")
    _req(lse2, torch.float32, "lse2")
    if tuple(lse2.shape) != (2, B, H, Sq) or not lse2.is_contiguous():
        raise ValueError(f"attn_dual_bwd: lse2 must be contiguous [2, {B}, {H}, {Sq}]")
    need = attn_dual_ws_floats(B, H, Sq, rows_per_frame, Sa, Sb)
    if ws is None and need > 0:
        ws = torch.empty(need, dtype=torch.float32, device=q.device)
    if need > 0:
        _req(ws, torch.float32, "ws")
        if ws.numel() < need or not ws.is_contiguous():
            raise ValueError(f"attn_dual_bwd: workspace of {ws.numel()} floats, {need} needed")
    check(load_library().vt_attn_dual_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), k_ip.data_ptr(), v_ip.data_ptr(), do.data_ptr(),
                                          lse2.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dk_ip.data_ptr(), dv_ip.data_ptr(),
                                          _p(ws) if need > 0 else None, ws.numel() if need > 0 else 0, B, H, Sq, rows_per_frame, Sa, Sb,
                                          q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0),
                                          k_ip.stride(1), k_ip.stride(0), v_ip.stride(1), v_ip.stride(0), do.stride(1), do.stride(0),
                                          dq.stride(1), dq.stride(0), scale, img_scale, _stream()), "vt_attn_dual_bwd")


def attn_gen_fwd(q, k, v, o, lse2, H: int, head_dim: int, hstride: int, scale: float, kv_len=None, mask_block: int = 0):
    """head_dim 80 | 128 (csrc/attn_gen.hip).  q, o [NB, Sq, >= H*hstride]; k, v [NB, Sk, ...]; kv_len int32 [NB] | None"""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        _req(t, BF16, n, 3)
    if kv_len is not None:
        _req(kv_len, torch.int32, "kv_len", 1)
    NB, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    check(load_library().vt_attn_gen_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _p(lse2), _p(kv_len), head_dim, hstride,
                                         NB, H, Sq, Sk, q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0),
                                         o.stride(1), o.stride(0), scale, mask_block, _stream()), "vt_attn_gen_fwd")


def attn_gen_bwd(q, k, v, o, do, lse2, dq, dk, dv, H: int, head_dim: int, hstride: int, scale: float, kv_len=None, mask_block: int = 0):
    """mask_block > 0: dk, dv bf16 like k, v.  Otherwise either bf16 [NB, Sk, .] (items Sk rows apart; written whole by the key-stationary
    pass) or fp32 [NB, Sk, H*hstride] contiguous accumulators (zeroed here; the query range may then be split and summed with atomics --
    few keys, many queries)"""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o), ("do", do), ("dq", dq)):
        _req(t, BF16, n, 3)
    NB, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    if mask_block > 0 or dk.dtype == BF16:
        _req(dk, BF16, "dk", 3); _req(dv, BF16, "dv", 3)
        if mask_block == 0 and NB > 1 and not (dk.stride(0) == Sk * dk.stride(1) and dv.stride(0) == Sk * dv.stride(1)):
            raise ValueError("bf16 dk / dv: items must lie Sk rows apart")
        args = (dk.data_ptr(), dv.data_ptr(), None, None)
    else:
        _req(dk, torch.float32, "dk", 3); _req(dv, torch.float32, "dv", 3)
        if not (dk.is_contiguous() and dv.is_contiguous()):
            raise ValueError("dk / dv accumulators must be contiguous")
        dk.zero_(); dv.zero_()
        args = (None, None, dk.data_ptr(), dv.data_ptr())
    check(load_library().vt_attn_gen_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse2.data_ptr(), _p(kv_len),
                                         dq.data_ptr(), *args, head_dim, hstride, NB, H, Sq, Sk,
                                         q.stride(1), q.stride(0), k.stride(1), k.stride(0), v.stride(1), v.stride(0),
                                         o.stride(1), o.stride(0), do.stride(1), do.stride(0), dq.stride(1), dq.stride(0),
                                         dk.stride(1), dv.stride(1), scale, mask_block, _stream()), "vt_attn_gen_bwd")


def opensora_loss(out, x0, noise, coef, loss3, dout=None, grad_scale: float = 1.0):
    """out fp32 [B, 2C, ...], x0 / noise fp32 [B, C, ...], coef fp64 [B, 8], loss3 fp64 [3] (loss, mse, vb), dout fp32 like out | None"""
    _req(out, torch.float32, "out"); _req(x0, torch.float32, "x0"); _req(noise, torch.float32, "noise")
    _req(coef, torch.float64, "coef", 2); _req(loss3, torch.float64, "loss3", 1)
    B, C = x0.shape[0], x0.shape[1]
    if out.shape[1] != 2 * C or not (out.is_contiguous() and x0.is_contiguous() and noise.is_contiguous()):
        raise ValueError("out must be contiguous [B, 2C, ...] next to contiguous x0 / noise [B, C, ...]")
    check(load_library().vt_opensora_loss(out.data_ptr(), x0.data_ptr(), noise.data_ptr(), coef.data_ptr(), loss3.data_ptr(), _p(dout),
                                          x0.numel() // (B * C), C, B, grad_scale, _stream()), "vt_opensora_loss")


FP8 = torch.float8_e4m3fn


def quantize_fp8(x, scale: Optional[torch.Tensor] = None):
    """x bf16 [M, K] -> (xq float8_e4m3fn [M, K], scale fp32 [1]) with scale = max|x| / 448 (or the given stored scale)"""
    _req(x, BF16, "x", 2)
    M, K = x.shape
    y = torch.empty(M, K, dtype=FP8, device=x.device)
    given = scale is not None
    if not given:
        scale = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(1, dtype=torch.int32, device=x.device)
    check(load_library().vt_quantize_fp8(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), M, K, scale.data_ptr(), ws.data_ptr(),
                                         int(given), _stream()), "vt_quantize_fp8")
    return y, scale


def gemm_fp8(aq, wq, out, scale_a, scale_w, bias=None):
    """out bf16 [M, N] = (aq [M, K] @ wq [N, K]^T) * scale_a * scale_w + bias on the fp8 matrix cores"""
    _req(aq, FP8, "aq", 2); _req(wq, FP8, "wq", 2); _req(out, BF16, "out", 2)
    check(load_library().vt_gemm_fp8(aq.data_ptr(), aq.stride(0), wq.data_ptr(), wq.stride(0), out.data_ptr(), out.stride(0), aq.shape[0],
                                     wq.shape[0], aq.shape[1], _p(bias), scale_a.data_ptr(), scale_w.data_ptr(), _stream()), "vt_gemm_fp8")
    return out


def _amax_slot(amax):
    """an amax slot: a 1-element view of an fp32 (non-negative float bits, max'ed atomically as uint32) or int32 device tensor"""
    if not amax.is_cuda or amax.dtype not in (torch.float32, torch.int32) or amax.numel() < 1:
        raise ValueError("amax: expected an fp32 / int32 device tensor")
    return amax.data_ptr()


def gemm_mxfp8(aq, wq, out, scale_a, scale_w, bias=None, *, epilogue: int = EPI_BIAS, residual: Optional[torch.Tensor] = None,
               gate_txt: Optional[torch.Tensor] = None, gate_vid: Optional[torch.Tensor] = None, gate_bstride: int = 0, S: int = 1, St: int = 0,
               pre_act_out: Optional[torch.Tensor] = None, tail=None, out_fp8=None):
    """out bf16 [M, N] = epilogue((aq [M, K] @ wq [N, K]^T) * scale_a * scale_w [+ At @ Wt^T] + bias) on the MX-scaled fp8 matrix cores
    (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales).  scale_a / scale_w: device fp32 scalars (views).  Epilogue keywords as gemm()
    (EPI_BIAS, EPI_BIAS_GELU, EPI_GATED_RES).  tail = (At bf16 [M, Kt], Wt bf16 [N, Kt]), Kt a multiple of 32 up to 384 (column slices of wider
    buffers allowed): a bf16 K segment added into the same accumulators after the scaled fp8 sum.  out_fp8 = (Cq float8_e4m3fn [M, N], scale, amax): Cq = e4m3(out / scale), max |out| into the amax slot."""
    _req(aq, FP8, "aq", 2); _req(wq, FP8, "wq", 2); _req(out, BF16, "out", 2)
    M, K, N = aq.shape[0], aq.shape[1], wq.shape[0]
    if wq.shape[1] != K or out.shape[0] != M or out.shape[1] < N:
        raise ValueError(f"gemm_mxfp8: aq {tuple(aq.shape)}, wq {tuple(wq.shape)}, out {tuple(out.shape)}")
    At = Wt = None
    Kt = 0
    if tail is not None:
        At, Wt = tail
        _req(At, BF16, "tail A", 2); _req(Wt, BF16, "tail W", 2)
        Kt = At.shape[1]
        if Wt.shape[1] != Kt or At.shape[0] != M or Wt.shape[0] != N:
            raise ValueError(f"gemm_mxfp8: tail {tuple(At.shape)} x {tuple(Wt.shape)}^T for a [{M}, {N}] product")
    cq = sq = am = None
    if out_fp8 is not None:
        cq, sq, am = out_fp8
        _req(cq, FP8, "out_fp8", 2)
        if cq.shape[0] != M or cq.shape[1] < N:
            raise ValueError(f"gemm_mxfp8: out_fp8 {tuple(cq.shape)} for a [{M}, {N}] product")
        am = _amax_slot(am)
    check(load_library().vt_gemm_mxfp8(aq.data_ptr(), aq.stride(0), wq.data_ptr(), wq.stride(0), out.data_ptr(), out.stride(0), M, N, K,
                                       _p(bias), scale_a.data_ptr(), scale_w.data_ptr(), epilogue,
                                       _p(residual), 0 if residual is None else residual.stride(0),
                                       _p(gate_txt), _p(gate_vid), gate_bstride, S, St,
                                       _p(pre_act_out), 0 if pre_act_out is None else pre_act_out.stride(0),
                                       _p(At), 0 if At is None else At.stride(0), _p(Wt), 0 if Wt is None else Wt.stride(0), Kt,
                                       _p(cq), 0 if cq is None else cq.stride(0), _p(sq), am, _stream()), "vt_gemm_mxfp8")
    return out


def cast_fp8_scaled(x, y, scale, amax, copy=None, rows=None):
    """y float8_e4m3fn [M, K] = satfinite(RNE(x / scale)), max |x| into the amax slot; rows = (L, Lj, off): row m reads x row
    (m // L) * Lj + off + m % L (one stream's rows of a joint buffer), else row m; copy: bf16 [M, K] that receives those rows of x"""
    _req(x, BF16, "x", 2); _req(y, FP8, "y", 2)
    if copy is not None:
        _req(copy, BF16, "copy", 2)
    M, K = y.shape
    L, Lj, off = rows if rows is not None else (0, 0, 0)
    if x.shape[1] < K or (rows is None and x.shape[0] < M) or (rows is not None and (M % L or x.shape[0] < M // L * Lj)):
        raise ValueError(f"cast_fp8_scaled: x {tuple(x.shape)} -> y {tuple(y.shape)}, rows {rows}")
    check(load_library().vt_cast_fp8_scaled(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), _p(copy), 0 if copy is None else copy.stride(0),
                                            M, K, L, Lj, off, scale.data_ptr(), _amax_slot(amax), _stream()), "vt_cast_fp8_scaled")
    return y


def ln_modulate_fwd_fp8(x, y, gamma, beta, mod, mean, rstd, D: int, S: int, St: int, eps: float, q, qscale, amax):
    """ln_modulate_fwd plus q float8_e4m3fn [M, D] = e4m3(y / qscale) and max |y| into the amax slot (y is the same as ln_modulate_fwd's)"""
    _req(x, BF16, "x", 2); _req(y, BF16, "y", 2); _req(q, FP8, "q", 2)
    sh_t, sc_t, sh_v, sc_v, bstride = mod if mod is not None else (None, None, None, None, 0)
    check(load_library().vt_ln_modulate_fwd_fp8(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), _p(gamma), _p(beta),
                                                _p(sh_t), _p(sc_t), _p(sh_v), _p(sc_v), bstride, _p(mean), _p(rstd),
                                                x.shape[0], D, S, St, eps, q.data_ptr(), q.stride(0), qscale.data_ptr(), _amax_slot(amax),
                                                _stream()), "vt_ln_modulate_fwd_fp8")


def fp8_scale_update(amax, history, scale):
    """delayed scaling, all sites in one launch: history [n, H] <- (amax, history[:, :-1]) (newest first), scale [n] = max(history) / 448
    (1 where that is 0), amax [n] cleared"""
    _req(history, torch.float32, "history", 2); _req(scale, torch.float32, "scale", 1)
    n, H = history.shape
    if amax.numel() != n or scale.numel() != n or not (amax.is_contiguous() and history.is_contiguous() and scale.is_contiguous()):
        raise ValueError("fp8_scale_update: amax [n], history [n, H], scale [n], contiguous")
    check(load_library().vt_fp8_scale_update(_amax_slot(amax), history.data_ptr(), scale.data_ptr(), n, H, _stream()), "vt_fp8_scale_update")


FP8_E5M2 = torch.float8_e5m2
FP8_FORMATS = {FP8: (0, 448.0), FP8_E5M2: (1, 57344.0)}      # dtype -> (format code of the C-ABI, largest finite value)


def _fp8_code(t, name: str) -> int:
    if t.dtype not in FP8_FORMATS:
        raise ValueError(f"{name}: expected float8_e4m3fn or float8_e5m2, got {t.dtype}")
    _req(t, t.dtype, name, 2)
    return FP8_FORMATS[t.dtype][0]


def gemm_mxfp8_dx(gq, wqt, out, scale_g, scale_w, *, epilogue: int = EPI_BIAS, residual: Optional[torch.Tensor] = None,
                  pre_act_in: Optional[torch.Tensor] = None, tail=None, out_fp8=None):
    """the input-gradient product of a Linear on the MX-scaled fp8 matrix cores: out bf16 [M, N] = epilogue((gq [M, K] @ wqt [N, K]^T)
    * scale_g * scale_w [+ At @ Wt^T]).  gq: the quantised output gradient, float8_e5m2 or float8_e4m3fn; wqt: float8_e4m3fn, the
    byte-transposed weight (row-strided slices allowed).  epilogue: EPI_BIAS (plain), EPI_DGELU (times gelu'(pre_act_in)) or
    EPI_GATED_RES (+ residual).  tail as gemm_mxfp8 (Kt a multiple of 32 up to 384).  out_fp8 = (Cq fp8 [M, N] of either format, scale, amax): EPI_DGELU only."""
    fg = _fp8_code(gq, "gq")
    _req(wqt, FP8, "wqt", 2); _req(out, BF16, "out", 2)
    M, K, N = gq.shape[0], gq.shape[1], wqt.shape[0]
    if wqt.shape[1] != K or out.shape[0] != M or out.shape[1] < N:
        raise ValueError(f"gemm_mxfp8_dx: gq {tuple(gq.shape)}, wqt {tuple(wqt.shape)}, out {tuple(out.shape)}")
    for t, name in ((residual, "residual"), (pre_act_in, "pre_act_in")):
        if t is not None:
            _req(t, BF16, name, 2)
            if t.shape[0] < M or t.shape[1] < N:
                raise ValueError(f"gemm_mxfp8_dx: {name} {tuple(t.shape)} for a [{M}, {N}] product")
    At = Wt = None
    Kt = 0
    if tail is not None:
        At, Wt = tail
        _req(At, BF16, "tail A", 2); _req(Wt, BF16, "tail W", 2)
        Kt = At.shape[1]
        if Wt.shape[1] != Kt or At.shape[0] != M or Wt.shape[0] != N:
            raise ValueError(f"gemm_mxfp8_dx: tail {tuple(At.shape)} x {tuple(Wt.shape)}^T for a [{M}, {N}] product")
    cq = sq = am = None
    fo = 0
    if out_fp8 is not None:
        cq, sq, am = out_fp8
        fo = _fp8_code(cq, "out_fp8")
        if cq.shape[0] != M or cq.shape[1] < N:
            raise ValueError(f"gemm_mxfp8_dx: out_fp8 {tuple(cq.shape)} for a [{M}, {N}] product")
        am = _amax_slot(am)
    check(load_library().vt_gemm_mxfp8_dx(gq.data_ptr(), gq.stride(0), fg, wqt.data_ptr(), wqt.stride(0), out.data_ptr(), out.stride(0), M, N, K,
                                          scale_g.data_ptr(), scale_w.data_ptr(), epilogue,
                                          _p(residual), 0 if residual is None else residual.stride(0),
                                          _p(pre_act_in), 0 if pre_act_in is None else pre_act_in.stride(0),
                                          _p(At), 0 if At is None else At.stride(0), _p(Wt), 0 if Wt is None else Wt.stride(0), Kt,
                                          _p(cq), 0 if cq is None else cq.stride(0), fo, _p(sq), am, _stream()), "vt_gemm_mxfp8_dx")
    return out


def cast_fp8_fmt(x, y, scale, amax, copy=None, rows=None):
    """cast_fp8_scaled into y's format (float8_e4m3fn or float8_e5m2: satfinite at 448 / 57344)"""
    _req(x, BF16, "x", 2)
    fmt = _fp8_code(y, "y")
    if copy is not None:
        _req(copy, BF16, "copy", 2)
    M, K = y.shape
    L, Lj, off = rows if rows is not None else (0, 0, 0)
    if x.shape[1] < K or (rows is None and x.shape[0] < M) or (rows is not None and (M % L or x.shape[0] < M // L * Lj)):
        raise ValueError(f"cast_fp8_fmt: x {tuple(x.shape)} -> y {tuple(y.shape)}, rows {rows}")
    check(load_library().vt_cast_fp8_fmt(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), _p(copy), 0 if copy is None else copy.stride(0),
                                         M, K, L, Lj, off, fmt, scale.data_ptr(), _amax_slot(amax), _stream()), "vt_cast_fp8_fmt")
    return y


def gate_mul_fp8(x, y, g_txt, g_vid, bstride: int, D: int, S: int, St: int, q, scale, amax):
    """gate_mul (y bit-equal to it) plus q fp8 [M, D] = satfinite(RNE(y / scale)) in q's format and max |y| into the amax slot"""
    _req(x, BF16, "x", 2); _req(y, BF16, "y", 2)
    fmt = _fp8_code(q, "q")
    if x.shape[1] < D or y.shape[1] < D or q.shape[1] < D or y.shape[0] < x.shape[0] or q.shape[0] < x.shape[0]:
        raise ValueError(f"gate_mul_fp8: x {tuple(x.shape)}, y {tuple(y.shape)}, q {tuple(q.shape)}, D {D}")
    check(load_library().vt_gate_mul_fp8(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), g_txt.data_ptr(), g_vid.data_ptr(), bstride,
                                         x.shape[0], D, S, St, q.data_ptr(), q.stride(0), fmt, scale.data_ptr(), _amax_slot(amax), _stream()),
          "vt_gate_mul_fp8")


def fp8_scale_update_fmax(amax, history, scale, fmax: float):
    """fp8_scale_update with the format's largest finite value as the divisor: scale [n] = max(history) / fmax (448 e4m3, 57344 e5m2)"""
    _req(history, torch.float32, "history", 2); _req(scale, torch.float32, "scale", 1)
    n, H = history.shape
    if amax.numel() != n or scale.numel() != n or not (amax.is_contiguous() and history.is_contiguous() and scale.is_contiguous()):
        raise ValueError("fp8_scale_update_fmax: amax [n], history [n, H], scale [n], contiguous")
    check(load_library().vt_fp8_scale_update_fmax(_amax_slot(amax), history.data_ptr(), scale.data_ptr(), n, H, float(fmax), _stream()),
          "vt_fp8_scale_update_fmax")


def qk_rmsnorm_rope128_fwd(qkv, out, gq, gk, rstd, H: int, L: int, Lout: int, row_off: int, rope=None, eps: float = 1e-6):
    """qkv bf16 [M, 3*H*128] -> out rows (m // L) * Lout + row_off + m % L: q^ | k^ | v.  rope = (cos, sin) fp32 [S_rope, 128] for the
    first S_rope positions of every sample"""
    _req(qkv, BF16, "qkv", 2); _req(out, BF16, "out", 2)
    cos, sin = (None, None) if rope is None else rope
    check(load_library().vt_qk_rmsnorm_rope128_fwd(qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), gq.data_ptr(), gk.data_ptr(),
                                                   rstd.data_ptr(), _p(cos), _p(sin), qkv.shape[0], H, L, Lout, row_off,
                                                   0 if cos is None else cos.shape[0], eps, _stream()), "vt_qk_rmsnorm_rope128_fwd")


def qk_rmsnorm_rope128_bwd(dout, qkv, dqkv, gq, gk, rstd, dgq, dgk, H: int, L: int, Lout: int, row_off: int, rope=None):
    _req(dout, BF16, "dout", 2); _req(qkv, BF16, "qkv", 2); _req(dqkv, BF16, "dqkv", 2)
    cos, sin = (None, None) if rope is None else rope
    check(load_library().vt_qk_rmsnorm_rope128_bwd(dout.data_ptr(), dout.stride(0), qkv.data_ptr(), qkv.stride(0), dqkv.data_ptr(), dqkv.stride(0),
                                                   gq.data_ptr(), gk.data_ptr(), rstd.data_ptr(), _p(cos), _p(sin), _p(dgq), _p(dgk),
                                                   qkv.shape[0], H, L, Lout, row_off, 0 if cos is None else cos.shape[0], _stream()),
          "vt_qk_rmsnorm_rope128_bwd")


def attn128_fwd(q, k, v, o, lse2, H: int, scale: float, kv_len=None):
    """head_dim 128, long sequences (csrc/attn128.hip).  q, k, v, o: [B, S, >= H*128] bf16 views; lse2 fp32 [B, H, S]; kv_len int32 [B] | None"""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        _req(t, BF16, n, 3)
    _req(lse2, torch.float32, "lse2", 3)
    if kv_len is not None:
        _req(kv_len, torch.int32, "kv_len", 1)
    B, S = q.shape[0], q.shape[1]
    if k.shape[1] != S or v.shape[1] != S:
        raise ValueError("attn128: self-attention over one joint sequence (queries and keys share S)")
    check(load_library().vt_attn128_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse2.data_ptr(), _p(kv_len), B, H, S,
                                        q.stride(1), k.stride(1), v.stride(1), o.stride(1), q.stride(0), k.stride(0), v.stride(0), o.stride(0),
                                        scale, _stream()), "vt_attn128_fwd")


def attn128_bwd(q, k, v, o, do, lse2, dq, dk, dv, H: int, scale: float, kv_len=None):
    """dq: bf16 view like q -> two-pass backward (dQ written once); fp32 [B, S, H*128] -> one-pass backward, dQ accumulated atomically (zeroed
    here); dk, dv bf16 views like k, v"""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o), ("do", do), ("dk", dk), ("dv", dv)):
        _req(t, BF16, n, 3)
    B, S = q.shape[0], q.shape[1]
    delta = torch.empty(B * H * S, dtype=torch.float32, device=q.device)
    two_pass = dq.dtype == BF16
    if not two_pass:
        _req(dq, torch.float32, "dq", 3)
        dq.zero_()
    with _timed("attn128_bwd", 8.0 * S * S * H * 128 * B):
        check(load_library().vt_attn128_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse2.data_ptr(), _p(kv_len),
                                            delta.data_ptr(), None if two_pass else dq.data_ptr(), dq.data_ptr() if two_pass else None,
                                            dk.data_ptr(), dv.data_ptr(), B, H, S,
                                            q.stride(1), k.stride(1), v.stride(1), o.stride(1), do.stride(1), dq.stride(1), dq.stride(1), dk.stride(1), dv.stride(1),
                                            q.stride(0), k.stride(0), v.stride(0), o.stride(0), do.stride(0), dq.stride(0), dq.stride(0), dk.stride(0), dv.stride(0),
                                            scale, _stream()), "vt_attn128_bwd")
