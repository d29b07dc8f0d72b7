"""The floor-derived per-parameter gradient bars (parity.grad_floor / floor_bars) on the CPU, with no device in the loop: for every model
family the GPU tests check, the fp64 oracle and its bf16 restatement are run on the tiny configuration and the goldens those tests use, and

  * the clean bf16 restatement passes the new bars with no parameter flagged (the reference alone stays within them);
  * wrong models -- the oracle with one function patched (a branch scaled, a residual branch weakened, a norm's eps changed, an attention
    head dropped, the LoRA scaling off by one rank), run in bf16 so that they carry realistic noise, and wrong gradients (one tensor scaled,
    an eighth of its rows zero, a bias that missed one sample of the batch) -- are flagged on the parameters the mutation touches.

The old flat bars are applied to the same mutants; what they flagged is recorded in each family's table (nothing is asserted about that).
The tables' columns: the mutant's worst per-parameter rel-L2 against the clean fp64 gradients; how many parameters the old flat bars and the
floor-derived bars flag; and how many of the parameters the mutation touches went unflagged because its exact effect on them is below their
bar.  A mutant the new bars cannot tell from noise on such a parameter is not deleted: it is listed in BLIND with its figures."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_io
from parity import floor_bars, grad_floor, grad_report, rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import cogvideox_oracle as CO            # noqa: E402
import dc_oracle as DC                   # noqa: E402
import hunyuan_oracle as HO              # noqa: E402
import stdit_oracle as SO                # noqa: E402
import unet_oracle as U                  # noqa: E402

BF = torch.bfloat16
F64 = torch.float64
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------ mutation tools
@contextlib.contextmanager
def patched(obj, name, new):
    old = getattr(obj, name)
    setattr(obj, name, new(old))
    try:
        yield
    finally:
        setattr(obj, name, old)


def scaled(s):
    """the function's result times s"""
    return lambda f: (lambda *a, **k: f(*a, **k) * s)


def residual_scaled(s):
    """for f(x, ...) = x + branch(x, ...): the branch times s"""
    return lambda f: (lambda x, *a, **k: x + s * (f(x, *a, **k) - x))


def head0_dropped_einsum(f):
    """torch.einsum whose attention-times-value product loses head 0"""
    def einsum(eq, *ops):
        o = f(eq, *ops)
        if eq == "bhij,bhjd->bhid":
            keep = torch.ones(o.shape[1], dtype=o.dtype); keep[0] = 0
            o = o * keep.view(1, -1, 1, 1)
        return o
    return einsum


def head0_dropped_sdpa(head_dim):
    def wrap(f):
        def sdpa(q, *a, **k):
            o = f(q, *a, **k)
            keep = torch.ones(o.shape[head_dim], dtype=o.dtype); keep[0] = 0
            shape = [1] * o.dim(); shape[head_dim] = -1
            return o * keep.view(shape)
        return sdpa
    return wrap


def with_eps(eps, pos):
    """the norm function with its eps (positional argument `pos`, or the keyword) replaced"""
    def wrap(f):
        def norm(*a, **k):
            a = list(a)
            if len(a) > pos:
                a[pos] = eps
            else:
                k["eps"] = eps
            return f(*a, **k)
        return norm
    return wrap


# ------------------------------------------------------------------ the families
class Family:
    """loss(dt, P, n): the oracle's training loss in dtype dt on the parameters P (leaves of dtype dt), over the first n samples of the batch
    but normalised by the whole batch B -- samples are independent, so loss(n=B-1)'s gradients are the full ones minus the last sample's.
    With dt = bf16 the network runs in bf16 and the loss is taken in fp32 from its bf16 output, as on the device."""
    cos_min, rel_max = 0.98, 0.2             # the flat bars of the family's GPU tests
    B = 2

    def grads(self, dt, n=None, params=None):
        P = {k: (v.detach().to(dt).requires_grad_(True) if isinstance(v, torch.Tensor) else v) for k, v in (params or self.params).items()}
        self.loss(dt, P, n or self.B).backward()
        return {k: v.grad for k, v in P.items() if isinstance(v, torch.Tensor)}

    def has(self, *parts):
        return [n for n in self.names if any(p in n for p in parts)]

    @property
    def names(self):
        return [k for k, v in self.params.items() if isinstance(v, torch.Tensor)]


def _ldt(dt):
    return F64 if dt == F64 else torch.float32


class UNetLoRA(Family):
    """VideoCrafter2 tiny UNet with the rank-4 adapters of test_unet_gpu.py's LoRA step (tests/golden/unet_train), base weights and adapters
    all trained.  bf16 floor: median 3.21e-02, worst 5.96e-02, overall 2.81e-02 over 806 parameters.

    | mutant                                         | worst rel | old 0.98,0.2 | new bars     | below bar  |
    |------------------------------------------------|-----------|--------------|--------------|------------|
    | cross_attention output x 0.95                  |     0.163 |    0 of 806  |  781 of 806  |   0 of 330 |
    | temporal-transformer branch x 0.9              |     0.398 |  606 of 806  |  804 of 806  |   0 of 304 |
    | GroupNorm32 eps 1e-2 for 1e-5                  |     0.144 |    0 of 806  |  739 of 806  |   1 of 32  |
    | attention head 0 dropped                       |     1.468 |  805 of 806  |  806 of 806  |   0 of 60  |
    | LoRA scaling alpha / (r + 1)                   |     0.225 |  149 of 806  |  183 of 806  |   0 of 180 |
    | one to_q weight gradient x 0.9                 |     0.104 |    0 of 806  |    1 of 806  |   0 of 1   |
    | first 1/8 rows of it zero                      |     0.327 |    1 of 806  |    1 of 806  |   0 of 1   |
    | a bias gradient without the last sample        |     0.787 |    1 of 806  |    1 of 806  |   0 of 1   |
    | the noisiest parameter's gradient x 0.95       |     0.057 |    0 of 806  |    0 of 806  |   1 of 1   |"""
    def __init__(self):
        self.cfg = U.tiny_config()
        g = golden_io.load("unet_train")
        self.r, self.alpha = int(g["lora.r"]), float(g["lora.alpha"])
        L = U.init_lora(self.cfg, r=self.r, lora_alpha=self.alpha, seed=3, zero_b=False)
        self.params = {**{k: v.to(BF) for k, v in U.init_params(self.cfg, seed=11).items()}, **{k: (v.to(BF) if isinstance(v, torch.Tensor) else v) for k, v in L.items()}}
        self.x, self.ctx, self.t, self.fps, self.noise = [torch.from_numpy(g["net." + k]) for k in ("x", "context", "t", "fps", "noise")]
        self.B = self.x.shape[0]
        tt = [pre for blk in U.structure(self.cfg)["input"] + [U.structure(self.cfg)["middle"]] + U.structure(self.cfg)["output"] for kind, pre, _ in blk if kind == "tt"]
        self.tt = tt + [U.structure(self.cfg)["init_attn"][1]]

    def loss(self, dt, P, n):
        out = U.unet_forward(P, self.cfg, self.x[:n].to(BF).to(dt), self.t[:n], self.ctx[:n].to(BF).to(dt), fps=self.fps[:n])
        return ((out.to(_ldt(dt)) - self.noise[:n].to(_ldt(dt))) ** 2).mean(dim=(1, 2, 3, 4)).sum() / self.B

    def mutants(self):
        q = self.has(".attn2.to_q.weight")[0]
        wrong_scale = dict(self.params); wrong_scale[U.LORA_SCALING_KEY] = self.alpha / (self.r + 1)
        return [("cross_attention output x 0.95", [(U, "cross_attention", scaled(0.95))], self.has(".attn1.", ".attn2.")),
                ("temporal-transformer branch x 0.9", [(U, "temporal_transformer", residual_scaled(0.9))], [n for n in self.names if any(n.startswith(p + ".") for p in self.tt)]),
                ("GroupNorm32 eps 1e-2 for 1e-5", [(U, "group_norm32", with_eps(1e-2, 3))], self.has(".in_layers.0.", ".out_layers.0.")),
                ("attention head 0 dropped", [(torch, "einsum", head0_dropped_einsum)], self.has(".to_v.weight", ".to_out.0.weight")),
                ("LoRA scaling alpha / (r + 1)", wrong_scale, self.has("lora_")),
                ("one to_q weight gradient x 0.9", ("scale", q), [q]),
                ("first 1/8 rows of it zero", ("rows", q), [q]),
                ("a bias gradient without the last sample", ("sample", q.replace(".attn2.to_q.weight", ".attn2.to_out.0.bias")), [q.replace(".attn2.to_q.weight", ".attn2.to_out.0.bias")])]


class DynamiCrafter(Family):
    """DynamiCrafter tiny UNet fed by the Resampler through dc_flow_loss, the setting of test_dc_gpu.py's flow test (v target, use_scale,
    conditioning frame 2): `unet.*` and `rs.*` parameters.  bf16 floor: median 3.02e-02, worst 5.44e-02, overall 2.88e-02 over 669 parameters.

    | mutant                                         | worst rel | old 0.98,0.2 | new bars     | below bar  |
    |------------------------------------------------|-----------|--------------|--------------|------------|
    | image branch of attn2 x 0.9                    |     0.128 |    0 of 669  |  662 of 669  |   0 of 43  |
    | feed_forward output x 1.05                     |     0.090 |    0 of 669  |  561 of 669  |   0 of 60  |
    | LayerNorm eps 1e-2 for 1e-5                    |     0.683 |  548 of 669  |  669 of 669  |   0 of 10  |
    | attention head 0 dropped                       |     1.519 |  669 of 669  |  669 of 669  |   0 of 71  |
    | Resampler output x 0.95                        |     0.107 |    0 of 669  |  344 of 669  |   0 of 29  |
    | one to_q weight gradient x 0.9                 |     0.106 |    0 of 669  |    1 of 669  |   0 of 1   |
    | first 1/8 rows of it zero                      |     0.362 |    1 of 669  |    1 of 669  |   0 of 1   |
    | a bias gradient without the last sample        |     0.411 |    1 of 669  |    1 of 669  |   0 of 1   |
    | the noisiest parameter's gradient x 0.95       |     0.071 |    0 of 669  |    0 of 669  |   1 of 1   |"""
    def __init__(self):
        self.cfg = DC.dc_tiny_config()
        self.params = {**{"unet." + k: v.to(BF) for k, v in DC.dc_init_params(self.cfg, seed=21).items()},
                       **{"rs." + k: v.to(BF) for k, v in DC.rs_init_params(DC.RS_FLOW, seed=33).items()}}
        g = torch.Generator().manual_seed(17)
        B, T, H, W = 2, self.cfg.temporal_length, 8, 8
        rb = lambda t: t.to(BF).float()
        self.z = torch.randn(B, 4, T, H, W, generator=g)
        self.ctx = rb(torch.randn(B, 77, self.cfg.context_dim, generator=g))
        self.tok = rb(torch.randn(B, 9, DC.RS_FLOW["embedding_dim"], generator=g))
        self.noise = torch.randn(B, 4, T, H, W, generator=g)
        self.t, self.fs = torch.tensor([37, 912]), torch.tensor([24, 3])
        self.abar = U.lddpm_alphas_cumprod()
        self.scale_arr = U.scale_arr(scale_b=0.3).double()
        self.rs = [n for n in self.params if n.startswith("rs.")]

    def loss(self, dt, P, n):
        Pu = {k[5:]: v for k, v in P.items() if k.startswith("unet.")}
        Pr = {k[3:]: v for k, v in P.items() if k.startswith("rs.")}
        ld = _ldt(dt)
        l = DC.dc_flow_loss(Pu, self.cfg, Pr, DC.RS_FLOW, self.z[:n].to(ld), self.ctx[:n].to(ld), self.tok[:n].to(ld), self.t[:n], self.noise[:n].to(ld),
                            self.fs[:n], 2, self.abar, self.scale_arr.to(ld), model_dtype=dt)
        return l * n / self.B

    def mutants(self):
        q = self.has(".attn2.to_q.weight")[0]
        b = "rs.proj_in.bias"
        return [("image branch of attn2 x 0.9", [(DC, "dc_cross_attention", lambda f: (lambda *a, **k: f(*a, **{**k, "img_scale": 0.9})))], self.has("to_k_ip", "to_v_ip") + self.rs),
                ("feed_forward output x 1.05", [(U, "feed_forward", scaled(1.05))], self.has(".ff.")),
                ("LayerNorm eps 1e-2 for 1e-5", [(F, "layer_norm", with_eps(1e-2, 4))], [n for n in self.rs if "norm" in n]),
                ("attention head 0 dropped", [(torch, "einsum", head0_dropped_einsum)], self.has(".to_v.weight", "to_v_ip.weight", "to_kv.weight", "to_out.0.weight", "to_out.weight")),
                ("Resampler output x 0.95", [(DC, "rs_forward", scaled(0.95))], self.rs),
                ("one to_q weight gradient x 0.9", ("scale", q), [q]),
                ("first 1/8 rows of it zero", ("rows", q), [q]),
                ("a bias gradient without the last sample", ("sample", b), [b])]


class STDiT(Family):
    """OpenSora STDiT, tiny configuration, the inputs of test_stdit_gpu.py's train step (t = 0, 250, 999; ragged caption mask).
    bf16 floor: median 3.74e-02, worst 7.26e-02, overall 4.38e-02 over 53 parameters.

    | mutant                                         | worst rel | old 0.98,0.2 | new bars     | below bar  |
    |------------------------------------------------|-----------|--------------|--------------|------------|
    | attention output x 0.95                        |     0.098 |    0 of 53   |   23 of 53   |   0 of 16  |
    | cross-attention branch x 0.9                   |     0.132 |    0 of 53   |   42 of 53   |   0 of 16  |
    | MLP hidden activation x 1.05                   |     0.147 |    0 of 53   |   24 of 53   |   0 of 3   |
    | LayerNorm eps 1e-2 for 1e-6                    |     0.072 |    0 of 53   |    0 of 53   |   3 of 3   |
    | attention head 0 dropped                       |     0.407 |   16 of 53   |   52 of 53   |   0 of 8   |
    | one qkv weight gradient x 0.9                  |     0.108 |    0 of 53   |    1 of 53   |   0 of 1   |
    | first 1/8 rows of it zero                      |     0.099 |    0 of 53   |    1 of 53   |   0 of 1   |
    | a bias gradient without the last sample        |     0.380 |    1 of 53   |    1 of 53   |   0 of 1   |
    | the noisiest parameter's gradient x 0.95       |     0.075 |    0 of 53   |    0 of 53   |   1 of 1   |"""
    B = 3

    def __init__(self):
        self.cfg = cfg = SO.tiny_config()
        self.params = {k: v.to(BF) for k, v in SO.init_params(cfg, seed=3).items()}
        gen = torch.Generator().manual_seed(21)
        self.x0 = torch.randn(3, 4, *cfg.input_size, generator=gen)
        self.noise = torch.randn(self.x0.shape, generator=gen)
        self.y = torch.randn(3, 1, cfg.model_max_length, cfg.caption_channels, generator=gen).to(BF).float()
        self.mask = torch.zeros(3, cfg.model_max_length, dtype=torch.int64); self.mask[0, :3] = 1; self.mask[1, :12] = 1; self.mask[2, :7] = 1
        self.t = torch.tensor([0, 250, 999])
        self.sch = SO.schedule(1000)
        self.x_t = SO.q_sample(self.x0, self.t, self.noise, self.sch).to(BF)

    def loss(self, dt, P, n):
        out = SO.stdit_forward(P, self.cfg, self.x_t[:n].to(dt), self.t[:n], self.y[:n].to(dt), self.mask[:n])
        if dt == F64:
            sch = {k: (v.double() if v.is_floating_point() else v) for k, v in self.sch.items()}
            return SO.opensora_loss(out.double(), self.x0[:n].double(), self.noise[:n].double(), self.t[:n], sch)[0] * n / self.B
        return SO.opensora_loss(out, self.x0[:n], self.noise[:n], self.t[:n], self.sch)[0] * n / self.B

    def mutants(self):
        q = "blocks.0.attn.qkv.weight"
        b = "blocks.1.mlp.fc2.bias"

        def head0(f):
            def attention(x, P, pre, heads):
                Bq, N, C = x.shape
                hd = C // heads
                qkv = SO._lin(x, P, pre + ".qkv").view(Bq, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
                a = ((qkv[0] * hd ** -0.5) @ qkv[1].transpose(-2, -1)).softmax(dim=-1)
                keep = torch.ones(heads, dtype=x.dtype); keep[0] = 0
                return SO._lin(((a @ qkv[2]) * keep.view(1, -1, 1, 1)).transpose(1, 2).reshape(Bq, N, C), P, pre + ".proj")
            return attention
        return [("attention output x 0.95", [(SO, "attention", scaled(0.95))], self.has(".attn.", ".attn_temp.")),
                ("cross-attention branch x 0.9", [(SO, "cross_attention", scaled(0.9))], self.has(".cross_attn.", "y_embedder")),
                ("MLP hidden activation x 1.05", [(SO, "gelu_tanh", scaled(1.05))], self.has(".mlp.fc2.weight", "y_proj.fc2.weight")),
                ("LayerNorm eps 1e-2 for 1e-6", [(F, "layer_norm", with_eps(1e-2, 4))], self.has("scale_shift_table")),
                ("attention head 0 dropped", [(SO, "attention", head0)], self.has(".attn.qkv.weight", ".attn.proj.weight", ".attn_temp.qkv.weight", ".attn_temp.proj.weight")),
                ("one qkv weight gradient x 0.9", ("scale", q), [q]),
                ("first 1/8 rows of it zero", ("rows", q), [q]),
                ("a bias gradient without the last sample", ("sample", b), [b])]


class HunyuanBlocks(Family):
    """HunyuanVideo: one double and one single block stacked on tests/golden/hunyuan_blocks.npz (text lengths 12 and 7 of 12) with the rank-4
    adapters of test_hunyuan_gpu.py's LoRA test, block weights and adapters all trained.  bf16 floor: median 6.84e-03, worst 1.45e-02, overall 6.62e-03 over 46 parameters.

    | mutant                                         | worst rel | old 0.98, 0.15| new bars     | below bar  |
    |------------------------------------------------|-----------|--------------|--------------|------------|
    | attention output x 0.95                        |     0.055 |    0 of 46   |   35 of 46   |   2 of 30  |
    | attention / block gate x 0.9                   |     0.105 |    0 of 46   |   46 of 46   |   0 of 8   |
    | MLP activation x 1.05                          |     0.051 |    0 of 46   |   24 of 46   |   0 of 7   |
    | RMSNorm eps 1e-2 for 1e-6                      |     0.032 |    0 of 46   |   24 of 46   |   0 of 6   |
    | attention head 0 dropped                       |     0.775 |   35 of 46   |   45 of 46   |   0 of 5   |
    | LoRA scaling alpha / (r + 1)                   |     0.208 |   14 of 46   |   30 of 46   |   0 of 14  |
    | one qkv weight gradient x 0.9                  |     0.101 |    0 of 46   |    1 of 46   |   0 of 1   |
    | first 1/8 rows of it zero                      |     0.277 |    1 of 46   |    1 of 46   |   0 of 1   |
    | a bias gradient without the last sample        |     0.805 |    1 of 46   |    1 of 46   |   0 of 1   |
    | the noisiest parameter's gradient x 0.95       |     0.053 |    0 of 46   |    1 of 46   |   0 of 1   |"""
    cos_min, rel_max = 0.98, 0.15
    D, H, r, alpha = 256, 2, 4, 2.0
    SITES = {"double_blocks.0.img_attn_qkv": ("q", "k", "v"), "double_blocks.0.img_attn_proj": ("",), "single_blocks.0.linear1": ("q", "k", "v")}

    def __init__(self):
        g = np.load(os.path.join(G, "hunyuan_blocks.npz"))
        self.T = T = lambda k: torch.from_numpy(g[k])
        D, H = self.D, self.H
        P = {**HO.init(HO.double_block_shapes(D, H, pre="double_blocks.0."), 1), **HO.init(HO.single_block_shapes(D, H, pre="single_blocks.0."), 2)}
        gen = torch.Generator().manual_seed(5)
        for mod, tags in self.SITES.items():
            for t in tags:
                dot = "." + t if t else ""
                P[f"lora.{mod}.lora_A{dot}.weight"] = torch.randn(self.r, D, generator=gen) * D ** -0.5
                P[f"lora.{mod}.lora_B{dot}.weight"] = torch.randn(D, self.r, generator=gen) * 0.05
        self.params = {k: v.to(BF) for k, v in P.items()}
        self.scaling = self.alpha / self.r
        self.img, self.txt, self.vec = [T(k).to(BF) for k in ("img", "txt", "vec")]
        self.tv, self.gx = T("txt_valid"), T("s_gx").to(BF)

    def loss(self, dt, P, n):
        Pe = {k: v for k, v in P.items() if not k.startswith("lora.")}
        for mod, tags in self.SITES.items():
            w = Pe[mod + ".weight"].clone()
            for j, t in enumerate(tags):
                dot = "." + t if t else ""
                w[j * self.D:(j + 1) * self.D] = w[j * self.D:(j + 1) * self.D] + self.scaling * P[f"lora.{mod}.lora_B{dot}.weight"] @ P[f"lora.{mod}.lora_A{dot}.weight"]
            Pe[mod + ".weight"] = w
        T, Lt = self.T, self.txt.shape[1]
        cos, sin = (T("cos").double(), T("sin").double()) if dt == F64 else (T("cos"), T("sin"))
        vec = self.vec[:n].to(dt)
        io, to = HO.double_block(self.img[:n].to(dt), self.txt[:n].to(dt), vec, Pe, "double_blocks.0.", self.H, self.tv[:n], cos, sin)
        xo = HO.single_block(torch.cat([io, to], 1), vec, Pe, "single_blocks.0.", self.H, Lt, self.tv[:n], cos, sin)
        return (xo.to(_ldt(dt)) * self.gx[:n].to(_ldt(dt))).sum()

    def mutants(self):
        q = "double_blocks.0.img_attn_qkv.weight"
        b = "single_blocks.0.linear2.bias"

        def gates(f):
            def mod(vec, P, name, n):
                c = list(f(vec, P, name, n))
                c[2] = c[2] * 0.9                    # the gate of the attention branch (double) / of the whole block (single)
                return c
            return mod

        @contextlib.contextmanager
        def wrong_scaling():
            old, self.scaling = self.scaling, self.alpha / (self.r + 1)
            try:
                yield
            finally:
                self.scaling = old
        return [("attention output x 0.95", [(HO, "varlen_attention", scaled(0.95))], self.has("attn_qkv", "attn_proj", "linear1", "_norm")),
                ("attention / block gate x 0.9", [(HO, "_mod", gates)], self.has("attn_proj", "linear2")),
                ("MLP activation x 1.05", [(F, "gelu", scaled(1.05))], self.has("mlp.fc2.weight", "mlp.fc1", "linear2.weight")),
                ("RMSNorm eps 1e-2 for 1e-6", [(HO, "rms_norm", with_eps(1e-2, 2))], self.has("_norm.weight")),
                ("attention head 0 dropped", [(F, "scaled_dot_product_attention", head0_dropped_sdpa(0))], self.has("attn_proj.weight", "linear2.weight", "attn_qkv.weight")),
                ("LoRA scaling alpha / (r + 1)", wrong_scaling, self.has("lora.")),
                ("one qkv weight gradient x 0.9", ("scale", q), [q]),
                ("first 1/8 rows of it zero", ("rows", q), [q]),
                ("a bias gradient without the last sample", ("sample", b), [b])]


class CogVideoX(Family):
    """CogVideoX DiT, tiny configuration (2 blocks, sincos positions), the inputs of test_model_gpu.py's full fine-tune step, with rank-4
    adapters on the attention projections, base weights and adapters all trained; the norm_k biases, whose exact gradient is zero, stay
    out as in the GPU test.  bf16 floor: median 5.83e-03, worst 2.09e-02, overall 4.44e-03 over 78 parameters.

    | mutant                                         | worst rel | old 0.99, 0.15| new bars     | below bar  |
    |------------------------------------------------|-----------|--------------|--------------|------------|
    | attention output x 0.95                        |     0.059 |    0 of 78   |   46 of 78   |   2 of 38  |
    | feed-forward activation x 0.9                  |     0.102 |    0 of 78   |   17 of 78   |   0 of 6   |
    | final layers' output x 1.05                    |     0.100 |    0 of 78   |   78 of 78   |   0 of 8   |
    | LayerNorm eps 1e-2 for 1e-5 / 1e-6             |     1.354 |   38 of 78   |   74 of 78   |   0 of 14  |
    | attention head 0 dropped                       |     1.095 |   45 of 78   |   50 of 78   |   0 of 4   |
    | LoRA scaling alpha / (r + 1)                   |     0.207 |   16 of 78   |   25 of 78   |   0 of 16  |
    | one to_q weight gradient x 0.9                 |     0.093 |    0 of 78   |    1 of 78   |   0 of 1   |
    | first 1/8 rows of it zero                      |     0.308 |    1 of 78   |    1 of 78   |   0 of 1   |
    | a bias gradient without the last sample        |     0.545 |    1 of 78   |    1 of 78   |   0 of 1   |
    | the noisiest parameter's gradient x 0.95       |     0.043 |    0 of 78   |    1 of 78   |   0 of 1   |"""
    cos_min, rel_max = 0.99, 0.15
    lora_scale = 0.25                                # lora_alpha 1 / r 4

    def __init__(self):
        self.cfg = cfg = CO.tiny_config()
        L = CO.init_lora(cfg, r=4, seed=1, zero_b=False)
        self.params = {**{k: v.to(BF) for k, v in CO.init_params(cfg, seed=11).items()}, **{"lora." + k: v.to(BF) for k, v in L.items()}}
        g = torch.Generator().manual_seed(77)
        B, Fr = 2, (cfg.sample_frames - 1) // 4 + 1
        self.x0 = torch.randn(B, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g)
        self.text = (torch.randn(B, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(BF)
        self.noise = torch.randn(self.x0.shape, generator=g)
        self.t = torch.tensor([150, 650])
        self.abar = CO.alphas_cumprod_cogvideox()
        self.noisy = CO.add_noise(self.x0, self.noise, self.t, self.abar.float()).to(BF)

    def grads(self, dt, n=None, params=None):
        return {k: v for k, v in super().grads(dt, n, params).items() if not k.endswith("norm_k.bias")}

    @property
    def names(self):
        return [k for k in self.params if not k.endswith("norm_k.bias")]

    def loss(self, dt, P, n):
        lora = {k[5:]: v for k, v in P.items() if k.startswith("lora.")}
        out = CO.dit_forward(P, self.cfg, self.noisy[:n].to(dt), self.text[:n].to(dt), self.t[:n], lora=lora, lora_scale=self.lora_scale)
        ld = _ldt(dt)
        pred = CO.get_velocity(out.to(ld), self.noisy[:n].to(ld), self.t[:n], self.abar)
        w = (1.0 / (1.0 - self.abar[self.t[:n]])).to(ld).view(-1, 1, 1, 1, 1)
        return torch.mean((w * (pred - self.x0[:n].to(ld)) ** 2).reshape(n, -1), dim=1).sum() / self.B

    def mutants(self):
        q = "transformer_blocks.0.attn1.to_q.weight"
        b = "transformer_blocks.1.ff.net.2.bias"

        @contextlib.contextmanager
        def wrong_scaling():
            old, self.lora_scale = self.lora_scale, 1.0 / 5
            try:
                yield
            finally:
                self.lora_scale = old
        return [("attention output x 0.95", [(F, "scaled_dot_product_attention", scaled(0.95))], self.has(".attn1.")),
                ("feed-forward activation x 0.9", [(CO, "gelu_tanh", scaled(0.9))], self.has(".ff.net.2.weight", ".ff.net.0.")),
                ("final layers' output x 1.05", [(CO, "dit_final", scaled(1.05))], self.has("proj_out", "norm_out", "norm_final")),
                ("LayerNorm eps 1e-2 for 1e-5 / 1e-6", [(F, "layer_norm", with_eps(1e-2, 4))], self.has("norm_q.", "norm_k.weight", "norm1.norm.", "norm2.norm.")),
                ("attention head 0 dropped", [(F, "scaled_dot_product_attention", head0_dropped_sdpa(1))], self.has("to_v.weight", "to_out.0.weight")),
                ("LoRA scaling alpha / (r + 1)", wrong_scaling, self.has("lora.")),
                ("one to_q weight gradient x 0.9", ("scale", q), [q]),
                ("first 1/8 rows of it zero", ("rows", q), [q]),
                ("a bias gradient without the last sample", ("sample", b), [b])]


FAMILIES = {"unet": UNetLoRA, "dynamicrafter": DynamiCrafter, "stdit": STDiT, "hunyuan": HunyuanBlocks, "cogvideox": CogVideoX}

# mutants the floor-derived bars cannot tell from bf16 noise on some parameter they touch: (family, mutant) -> (one such parameter -- None: the
# one with the largest floor, whichever it is --, its exact fp64 rel-L2 under the mutation, its floor and its bar).  They stay in the run; the
# test checks that each entry is still a blind spot, so that the list cannot outlive its cause.  Two kinds: a 5 % scale where 1.5 x floor is
# above 5 % (the UNets' and STDiT's floor is 3 % and more), and a "touched" bias that sits behind the mutated product and hardly moves.
BLIND = {
    ("unet", "GroupNorm32 eps 1e-2 for 1e-5"): ('output_blocks.3.0.out_layers.0.bias', "signal 3.72e-02, floor 1.61e-02, bar 4.81e-02"),
    ("unet", "the noisiest parameter's gradient x 0.95"): (None, "signal 5.00e-02, floor 5.96e-02, bar 8.94e-02"),
    ("dynamicrafter", "the noisiest parameter's gradient x 0.95"): (None, "signal 5.00e-02, floor 5.44e-02, bar 8.16e-02"),
    ("stdit", "LayerNorm eps 1e-2 for 1e-6"): ('final_layer.scale_shift_table', "signal 1.69e-02, floor 3.11e-02, bar 5.60e-02"),
    ("stdit", "the noisiest parameter's gradient x 0.95"): (None, "signal 5.00e-02, floor 7.26e-02, bar 1.09e-01"),
    ("hunyuan", "attention output x 0.95"): ('double_blocks.0.txt_attn_proj.bias', "signal 2.10e-03, floor 3.89e-03, bar 1.02e-02"),
    ("cogvideox", "attention output x 0.95"): ('transformer_blocks.1.attn1.to_out.0.bias', "signal 6.47e-05, floor 4.48e-03, bar 8.74e-03"),
}


def _mutant_grads(fam, how, clean, dt):
    """the gradients of one mutant in dtype dt: the oracle run with functions patched / other parameters / another setting, or the clean
    gradients of that dtype with one tensor spoiled"""
    if isinstance(how, tuple):
        kind, name = how
        out = dict(clean)
        if kind == "scale":
            out[name] = clean[name] * 0.9
        elif kind == "scale95":
            out[name] = clean[name] * 0.95
        elif kind == "rows":
            out[name] = clean[name].clone(); out[name][: max(1, out[name].shape[0] // 8)] = 0
        else:
            out[name] = fam.grads(dt, n=fam.B - 1)[name]
        return out
    if isinstance(how, dict):
        return fam.grads(dt, params=how)
    with contextlib.ExitStack() as stack:
        if callable(how):
            stack.enter_context(how())
        else:
            for obj, name, new in how:
                stack.enter_context(patched(obj, name, new))
        return fam.grads(dt)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_floor_bars_accept_the_clean_restatement_and_flag_every_mutant(family):
    """Every mutant is computed in bf16 (what a wrong device would hand the GPU test, noise included) and must be flagged on every parameter
    it touches.  Where one is not, the mutant is computed in fp64 too: its exact effect on that parameter, the `signal`, against the clean fp64
    gradient.  A signal at or above the bar that went unflagged fails the test; a signal below the bar is a blind spot of the bars, and
    the mutant must then be listed in BLIND with one such parameter and its figures."""
    fam = FAMILIES[family]()
    ref = fam.grads(F64)
    noisy = fam.grads(BF)
    assert all(g.dtype == BF for g in noisy.values()) and set(noisy) == set(fam.names)
    floor, ofloor = grad_floor(noisy, ref)
    bars = floor_bars(floor, fam.rel_max)
    fl = sorted(floor.values())
    print(f"[{family}] {len(floor)} parameters; bf16 floor median {fl[len(fl) // 2]:.2e}, worst {fl[-1]:.2e}, overall {ofloor:.2e}")
    pairs = lambda d: [(n, d[n], ref[n]) for n in fam.names]
    # the reference alone stays within its bars, and the fp64 run against itself is exact
    _, _, bad = grad_report(pairs(noisy), fam.cos_min, bars)
    assert not bad, bad[:8]
    assert grad_report(pairs(ref), fam.cos_min, bars)[1] == 0.0
    noisiest = max(floor, key=floor.get)
    mutants = fam.mutants() + [("the noisiest parameter's gradient x 0.95", ("scale95", noisiest), [noisiest])]
    assert len(mutants) >= 6
    assert {k[1] for k in BLIND if k[0] == family} <= {m[0] for m in mutants}, "BLIND lists mutants that no longer exist"
    problems = []
    for label, how, touched in mutants:
        assert touched and set(touched) <= set(fam.names), label
        mg = _mutant_grads(fam, how, noisy, BF)
        _, worst, bad_new = grad_report(pairs(mg), fam.cos_min, bars)
        _, _, bad_old = grad_report(pairs(mg), fam.cos_min, fam.rel_max)
        flagged = {b[0] for b in bad_new}
        unflagged = [n for n in touched if n not in flagged]
        signal = {n: rel_l2(g, ref[n]) for n, g in _mutant_grads(fam, how, ref, F64).items() if n in unflagged} if unflagged else {}
        blind = sorted((n for n in unflagged if signal[n] < bars[n]), key=lambda n: signal[n] / bars[n])
        missed = sorted(set(unflagged) - set(blind))
        print(f"    | {label:<46} | {worst:9.3f} | {len(bad_old):>4} of {len(fam.names):<4} | {len(flagged):>4} of {len(fam.names):<4} | {len(blind):>3} of {len(touched):<3} |"
              + (f"   blind e.g. {blind[0]} signal {signal[blind[0]]:.2e} floor {floor[blind[0]]:.2e} bar {bars[blind[0]]:.2e}" if blind else ""))
        if missed:
            problems.append(f"{label}: not flagged on " + ", ".join(
                f"{n} (rel {rel_l2(mg[n], ref[n]):.3e}, signal {signal[n]:.3e}, bar {bars[n]:.3e})" for n in missed[:6]))
        if blind and (family, label) not in BLIND:
            problems.append(f"{label}: {len(blind)} touched parameters below their bar (e.g. {blind[0]}): list it in BLIND")
        if (family, label) in BLIND and not (BLIND[(family, label)][0] in blind if BLIND[(family, label)][0] else blind):
            problems.append(f"{label}: {BLIND[(family, label)][0] or 'the noisiest parameter'} is no longer a blind spot")
    assert not problems, f"{family}: " + "; ".join(problems)


def test_every_patched_function_is_put_back():
    """the mutants patch oracle functions and torch functions in place: after a family's run they are the originals again"""
    before = (U.cross_attention, torch.einsum, F.layer_norm, F.scaled_dot_product_attention, F.gelu, HO._mod, SO.attention)
    fam = HunyuanBlocks()
    noisy = fam.grads(BF)
    for _, how, _ in fam.mutants()[:6]:
        _mutant_grads(fam, how, noisy, BF)
    assert fam.scaling == fam.alpha / fam.r
    assert before == (U.cross_attention, torch.einsum, F.layer_norm, F.scaled_dot_product_attention, F.gelu, HO._mod, SO.attention)
