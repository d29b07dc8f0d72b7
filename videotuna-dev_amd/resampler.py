"""DynamiCrafter's image-context projector on the vt355 kernels: ``Resampler`` with the constructor keys and parameter names of
videotuna/models/lvdm/modules/encoders/ip_resampler.py:65-152 (``image_proj_stage_config`` of configs/002_dynamicrafter/dc_i2v_1024.yaml:
dim 1024, depth 4, 12 heads x 64, 16 queries x 16 frames, embedding_dim 1280).  It is trained by the recipe
(``image_proj_model_trainable: True``): forward and backward, flat fp32 masters like the other trainables.

Small and once per step (B x 257 image tokens, 256 learned queries), so it is built from existing entry points only and not tuned: the
tape of ``vt355.unet._Run`` (Linear = GEMM with bias / residual epilogues, LayerNorm forward / backward), the tanh-GELU GEMM epilogues of
the STDiT Mlp (the reference's nn.GELU is the erf form: |difference| <= 5e-4, below bf16 resolution of the activations) and ``vt_attn_gen``
at its head_dim-80 instantiation with the 64-wide heads zero-padded (plain strided copies).  PerceiverAttention: queries = the latents, keys =
cat(norm1(x), norm2(latents)), scale (64^-1/4)^2 = 1/8.  There is no CPU / eager fallback.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict

import torch

from . import ops
from .ops import BF16, EPI_BIAS_GELU, EPI_DGELU, EPI_GATED_RES
from .unet import F32, FlatParamModule, _Run, _Var

HP = 80          # head width of the vt_attn_gen instantiation the 64-wide heads are padded to


def _shapes(c) -> Dict[str, tuple]:
    """reference state_dict keys in registration order"""
    sh: Dict[str, tuple] = {"latents": (1, c.n_latents, c.dim), "proj_in.weight": (c.dim, c.embedding_dim), "proj_in.bias": (c.dim,),
                            "proj_out.weight": (c.output_dim, c.dim), "proj_out.bias": (c.output_dim,),
                            "norm_out.weight": (c.output_dim,), "norm_out.bias": (c.output_dim,)}
    inner = c.heads * c.dim_head
    for i in range(c.depth):
        a, f = f"layers.{i}.0.", f"layers.{i}.1."
        for n in ("norm1", "norm2"):
            sh[a + n + ".weight"] = (c.dim,); sh[a + n + ".bias"] = (c.dim,)
        sh[a + "to_q.weight"] = (inner, c.dim); sh[a + "to_kv.weight"] = (2 * inner, c.dim); sh[a + "to_out.weight"] = (c.dim, inner)
        sh[f + "0.weight"] = (c.dim,); sh[f + "0.bias"] = (c.dim,)
        sh[f + "1.weight"] = (c.ff_mult * c.dim, c.dim); sh[f + "3.weight"] = (c.dim, c.ff_mult * c.dim)
    return sh


class Resampler(FlatParamModule):
    def __init__(self, dim=1024, depth=8, dim_head=64, heads=16, num_queries=8, embedding_dim=768, output_dim=1024, ff_mult=4, video_length=None):
        super().__init__()
        if dim_head != 64:
            raise NotImplementedError("the Resampler's attention is built for dim_head = 64 (padded to vt_attn_gen's 80)")
        if dim % 64 or embedding_dim % 64 or output_dim % 64:
            raise ValueError("dim, embedding_dim and output_dim must be multiples of 64 (one K-tile of the GEMM kernels)")
        self.num_queries, self.video_length = num_queries, video_length
        self.config = SimpleNamespace(dim=dim, depth=depth, dim_head=dim_head, heads=heads, embedding_dim=embedding_dim, output_dim=output_dim,
                                      ff_mult=ff_mult, n_latents=num_queries * (video_length if video_length is not None else 1))
        self._setup_flat(_shapes(self.config))

    def init_weights(self, seed: int = 0):
        """seeded random init for synthetic runs (nothing at zero)"""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for n, p in self._plist.items():
                shp = self.shapes[n]
                if n == "latents":
                    w = torch.randn(shp, generator=g) / math.sqrt(shp[-1])
                elif len(shp) == 1:
                    w = torch.randn(shp, generator=g) * 0.1 + (1.0 if n.endswith("weight") else 0.0)
                else:
                    w = torch.randn(shp, generator=g) * (0.7 / math.sqrt(shp[1]))
                p.copy_(w.to(p.device, BF16))
        self._packed = None
        return self

    def forward(self, x):
        """x [B, n1, embedding_dim] bf16 (frozen image encoder tokens) -> [B, num_queries * video_length, output_dim] bf16"""
        if not x.is_cuda:
            raise RuntimeError("vt355 Resampler runs only on an MI355X device (no CPU fallback)")
        if x.dtype != BF16:
            raise TypeError(f"x must be bf16, got {x.dtype}")
        if torch.is_grad_enabled() and self.train_state is not None:
            anchor = torch.zeros(1, device=x.device, requires_grad=True)
            return _RSFn.apply(anchor, self, x)
        return _RSRun(self, save=False).forward(x)


class _RSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, x):
        run = _RSRun(model, save=True)
        out = run.forward(x)
        ctx.run = run
        return out

    @staticmethod
    def backward(ctx, dout):
        ctx.run.backward(dout)
        ctx.run = None
        return None, None, None


def _packed_rs(model: Resampler) -> SimpleNamespace:
    ver = -1 if model.train_state is None else model.train_state.version
    if model._packed is not None and model._packed_version == ver:
        return model._packed
    P = SimpleNamespace(wt={})
    if model.train_state is not None:
        with torch.no_grad():
            for n, shp in model.shapes.items():
                if len(shp) == 2:
                    P.wt[n] = ops.transpose(model.flat(model.flat_bf16, n))
    model._packed, model._packed_version = P, ver
    return P


class _RSRun(_Run):
    def __init__(self, model: Resampler, save: bool):
        self.m, self.save = model, save
        self.c = model.config
        self.P = _packed_rs(model)
        self.fb = model.flat_bf16
        self.ts = model.train_state
        self.frozen = self.ts is None
        self.tape = []
        self.dev = model.device

    def _pad(self, t, rows):
        """[rows, H*64] (row-strided view allowed) -> [rows, H*80], the 16 extra columns of every head zero"""
        H = self.c.heads
        p = torch.zeros(rows, H * HP, dtype=BF16, device=self.dev)
        p.view(rows, H, HP)[:, :, :64].copy_(t.reshape(rows, H, 64))
        return p

    def _unpad(self, p, out):
        H = self.c.heads
        out.view(out.shape[0], H, 64).copy_(p.view(p.shape[0], H, HP)[:, :, :64])

    def perceiver_attention(self, xn: _Var, ln: _Var, pre: str, B: int, n1: int, N: int, residual: _Var) -> _Var:
        c = self.c
        H, D = c.heads, c.dim
        I, IP, Sk = H * 64, H * HP, n1 + N
        q = self.linear(ln, pre + "to_q.weight", None)                                   # [B*N, I]
        kvin = self.E(B * Sk, D)
        k3 = kvin.view(B, Sk, D)
        k3[:, :n1].copy_(xn.d.view(B, n1, D)); k3[:, n1:].copy_(ln.d.view(B, N, D))       # torch.cat((x, latents), dim=-2)
        kvv = _Var(kvin)
        if self.save:
            def bwd_cat():
                g3 = kvv.g.view(B, Sk, D)
                self.acc(xn, g3[:, :n1].reshape(B * n1, D))
                self.acc(ln, g3[:, n1:].reshape(B * N, D))
            self.tape.append(bwd_cat)
        kv = self.linear(kvv, pre + "to_kv.weight", None)                                # [B*Sk, 2I]: k | v
        qp, kp, vp = self._pad(q.d, B * N), self._pad(kv.d[:, :I], B * Sk), self._pad(kv.d[:, I:], B * Sk)
        op = self.E(B * N, IP)
        lse = self.E(B, H, N, dt=F32)
        q3, kk3, v3, o3 = qp.view(B, N, IP), kp.view(B, Sk, IP), vp.view(B, Sk, IP), op.view(B, N, IP)
        ops.attn_gen_fwd(q3, kk3, v3, o3, lse, H, HP, HP, 0.125)
        o = self.E(B * N, I)
        self._unpad(op, o)
        ov = _Var(o)
        if self.save:
            def bwd_attention():
                gp = self._pad(ov.g, B * N)
                dqp = self.E(B * N, IP)
                dk = self.E(B, Sk, IP, dt=F32); dv = self.E(B, Sk, IP, dt=F32)
                ops.attn_gen_bwd(q3, kk3, v3, o3, gp.view(B, N, IP), lse, dqp.view(B, N, IP), dk, dv, H, HP, HP, 0.125)
                dq = self.E(B * N, I)
                self._unpad(dqp, dq)
                q.g = dq
                dkv = self.E(B * Sk, 2 * I)
                dkv.view(B * Sk, 2, H, 64)[:, 0].copy_(dk.view(B * Sk, H, HP)[:, :, :64])
                dkv.view(B * Sk, 2, H, 64)[:, 1].copy_(dv.view(B * Sk, H, HP)[:, :, :64])
                kv.g = dkv
            self.tape.append(bwd_attention)
        return self.linear(ov, pre + "to_out.weight", None, residual=residual)

    def feed_forward(self, x: _Var, pre: str, residual: _Var) -> _Var:
        """LayerNorm -> Linear -> GELU -> Linear (no biases) + residual; GELU and its derivative in the GEMM epilogues"""
        h = self.layernorm(x, pre + "0")
        M = h.d.shape[0]
        w1, w2 = self.W(pre + "1.weight"), self.W(pre + "3.weight")
        F4, D = w1.shape[0], w2.shape[0]
        u = self.E(M, F4); ga = self.E(M, F4)
        ops.gemm(h.d, w1, ga, None, epilogue=EPI_BIAS_GELU, pre_act_out=u)
        y = self.E(M, D)
        ops.gemm(ga, w2, y, None, epilogue=EPI_GATED_RES, residual=residual.d)
        yv = _Var(y)
        if self.save:
            def bwd_ff():
                g = yv.g
                self.acc(residual, g)
                self.dW(g, ga, self.G(pre + "3.weight"))
                du = self.E(M, F4)
                ops.gemm(g, self.P.wt[pre + "3.weight"], du, None, epilogue=EPI_DGELU, pre_act_in=u)          # (g W2) * gelu'(u)
                self.dW(du, h.d, self.G(pre + "1.weight"))
                dh = self.E(M, w1.shape[1])
                ops.gemm(du, self.P.wt[pre + "1.weight"], dh, None)
                self.acc(h, dh)
            self.tape.append(bwd_ff)
        return yv

    def forward(self, x):
        c = self.c
        B, n1, E_ = x.shape
        N, D = c.n_latents, c.dim
        xv = _Var(x.reshape(B * n1, E_).contiguous()); xv.g = False              # frozen image encoder: no gradient wanted
        xp = self.linear(xv, "proj_in.weight", "proj_in.bias")                     # [B*n1, D]
        lat = self.E(B * N, D)
        lat.view(B, N, D).copy_(self.W("latents").view(1, N, D).expand(B, N, D))  # latents.repeat(B, 1, 1)
        latv = _Var(lat)
        if self.save:
            def bwd_latents(latv=latv):
                self.G("latents").view(N, D).add_(latv.g.view(B, N, D).float().sum(0))
            self.tape.append(bwd_latents)
        for i in range(c.depth):
            a = f"layers.{i}.0."
            xn = self.layernorm(xp, a + "norm1")
            ln = self.layernorm(latv, a + "norm2")
            latv = self.perceiver_attention(xn, ln, a, B, n1, N, latv)
            latv = self.feed_forward(latv, f"layers.{i}.1.", latv)
        out = self.layernorm(self.linear(latv, "proj_out.weight", "proj_out.bias"), "norm_out")
        self._out = out
        return out.d.view(B, N, c.output_dim)

    def backward(self, dout):
        """dout [B, N, output_dim]"""
        self._out.g = dout.reshape(-1, dout.shape[-1]).to(BF16).contiguous()
        while self.tape:
            self.tape.pop()()
        self._out = None
